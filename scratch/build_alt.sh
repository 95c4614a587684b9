#!/bin/bash
# scratch/build_alt.sh NAME "-DFLAG ..." : alternate build of conv_mfma.hip (forward / data-gradient: SMSUT_F16_X32, SMSUT_STAMPS) and
# conv_mfma_wgrad.hip (weight gradient: WG_RR_UNROLL, WG_KS_UNROLL, WG11_MIN_BLOCKS, WTS_STRIDE_VALUE, PLANE_WGRAD_MAX_HW,
# SMSUT_DBG_SUM, SMSUT_F16_X32, SMSUT_STAMPS) under the flags, linked with the product's other objects
# -> scratch/bin/libsmsut_NAME.so (for the in-process A/B harnesses)
set -e
cd "$(dirname "$0")/.."
P=smsut-medicalimgsegmentation_amd
mkdir -p scratch/bin
pids=
for f in conv_mfma conv_mfma_wgrad; do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast $2 -I include -c $P/csrc/$f.hip -o scratch/bin/${f}_$1.o &
  pids="$pids $!"
done
for p in $pids; do wait $p; done
objs=$(ls $P/lib/*.o | grep -v -e conv_mfma.o -e conv_mfma_wgrad.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o scratch/bin/libsmsut_$1.so scratch/bin/conv_mfma_$1.o scratch/bin/conv_mfma_wgrad_$1.o $objs
echo built scratch/bin/libsmsut_$1.so
