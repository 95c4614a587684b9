#!/bin/bash
# scratch/build_variant.sh <tag> [-Dflag ...]: builds scratch/bin/libsmsut_<tag>.so with conv_mfma.hip (forward / data-gradient) and
# conv_mfma_wgrad.hip (weight gradient: the WG_* / WTS_STRIDE_VALUE / PLANE_WGRAD_MAX_HW macros live there) compiled under the
# given defines (the other objects come from the product build) -- for in-process A/B runs (scratch/wgrad_ab2.py, conv_ab.py).
set -e
tag=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
pkg=$root/smsut-medicalimgsegmentation_amd
mkdir -p $root/scratch/bin
pids=
for f in conv_mfma conv_mfma_wgrad; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast -I $root/include "$@" -c $pkg/csrc/$f.hip -o $root/scratch/bin/${f}_$tag.o 2>/dev/null &
  pids="$pids $!"
done
for p in $pids; do wait $p; done
objs=$(ls $pkg/lib/*.o | grep -v -e conv_mfma.o -e conv_mfma_wgrad.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $root/scratch/bin/libsmsut_$tag.so $root/scratch/bin/conv_mfma_$tag.o $root/scratch/bin/conv_mfma_wgrad_$tag.o $objs
echo built $root/scratch/bin/libsmsut_$tag.so
