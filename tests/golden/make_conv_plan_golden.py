"""Writes tests/golden/conv_plan.npz: what the host-side planning queries of csrc/conv_mfma.hip answer over a grid of layer shapes.

The queries take integers only and launch nothing, so they run without a device.  They mirror the selection tables behind every
3x3 / 1x1 MFMA conv entry point (select_fwd_p, dispatch_fwd, fwd_p_eligible, wino_l_shape): a change of the host plumbing that moves
one of these answers has changed which kernel a shape runs or how many statistics tiles it writes.  tests/test_conv_plan_cpu.py
requires the built library to give exactly these answers.

Grid (``shapes()``): N x (H, W) x Kdim x Ndim of the constants below.  Columns (``COLUMNS``), per shape:
  tiles_f{f}_k{KS}, persistent_f{f}_k{KS}   smsut_conv2d_mfma_tiles / _persistent, f16 = f, kernel size KS
  form_sc{s}                                 smsut_conv2d_mfma_form, sc_dgrad = s
  fwd_sc_{c}, fwd_sc_f16_{c}, f16_hs_{c}     smsut_conv2d_fwd_sc_supported / _fwd_sc_f16_supported / _f16_hs_supported, cat = c
  dgrad_sc_{c}, dgrad_sc_f16_{c}             smsut_conv2d_dgrad_sc_supported / _dgrad_sc_f16_supported (Cout = Kdim, Cin = Ndim), split = c
  cat                                        smsut_conv2d_mfma_cat_supported
  split_{c}                                  smsut_conv2d_mfma_split_supported, split = c
Stored once per setting of SMSUT_WINOGRAD (``SETTINGS``: unset, and "0"), as ``plan_<setting>`` [shapes, columns] int32.  The library
reads the variable once per process, so each setting is recorded by a fresh child process (``record``).

    python tests/golden/make_conv_plan_golden.py        # rewrites tests/golden/conv_plan.npz from the built library
"""
import ctypes
import itertools
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(ROOT, "smsut-medicalimgsegmentation_amd", "lib", "libsmsut_hip.so")
OUT = os.path.join(HERE, "conv_plan.npz")

NS = (1, 2, 16, 32)
PLANES = ((4, 4), (8, 8), (16, 16), (24, 16), (20, 48), (64, 64), (128, 128), (256, 256))
CHANNELS = (4, 8, 16, 32, 48, 64, 80, 128, 256)
CATS = (0, 16, 32)
SETTINGS = {"unset": None, "off": "0"}          # value of SMSUT_WINOGRAD (None: not in the environment)

COLUMNS = ([f"{q}_f{f}_k{ks}" for q in ("tiles", "persistent") for f in (0, 1) for ks in (1, 3)] +
           [f"form_sc{s}" for s in (0, 1)] +
           [f"{q}_{c}" for q in ("fwd_sc", "fwd_sc_f16", "f16_hs", "dgrad_sc", "dgrad_sc_f16") for c in CATS] +
           ["cat"] + [f"split_{c}" for c in CATS])


def shapes():
    return [(n, h, w, k, nd) for n, (h, w), k, nd in itertools.product(NS, PLANES, CHANNELS, CHANNELS)]


def answers(lib_path):
    """[shapes, columns] int32 from the library at lib_path, under this process's SMSUT_WINOGRAD."""
    lib = ctypes.CDLL(lib_path)
    rows = []
    for n, h, w, k, nd in shapes():
        s = (n, h, w, k, nd)
        row = [getattr(lib, f"smsut_conv2d_mfma_{q}")(*s, ks, f) for q in ("tiles", "persistent") for f in (0, 1) for ks in (1, 3)]
        row += [lib.smsut_conv2d_mfma_form(*s, sc) for sc in (0, 1)]
        row += [getattr(lib, f"smsut_conv2d_{q}_supported")(*s, c)
                for q in ("fwd_sc", "fwd_sc_f16", "f16_hs", "dgrad_sc", "dgrad_sc_f16") for c in CATS]
        row.append(lib.smsut_conv2d_mfma_cat_supported(*s))
        row += [lib.smsut_conv2d_mfma_split_supported(*s, c) for c in CATS]
        rows.append(row)
    out = np.array(rows, dtype=np.int32)
    assert out.shape == (len(shapes()), len(COLUMNS))
    return out


def record(setting, lib_path=LIB):
    """``answers`` of a fresh child process whose SMSUT_WINOGRAD is SETTINGS[setting]."""
    env = {k: v for k, v in os.environ.items() if k != "SMSUT_WINOGRAD"}
    if SETTINGS[setting] is not None:
        env["SMSUT_WINOGRAD"] = SETTINGS[setting]
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "plan.npy")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path, path], env=env, check=True)
        return np.load(path, allow_pickle=False)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        np.save(sys.argv[3], answers(sys.argv[2]))
        sys.exit(0)
    lib_path = sys.argv[1] if len(sys.argv) > 1 else LIB
    data = {"columns": np.array(COLUMNS), "shapes": np.array(shapes(), dtype=np.int32)}
    for name in SETTINGS:
        data[f"plan_{name}"] = record(name, lib_path)
    assert not np.array_equal(data["plan_unset"], data["plan_off"]), "SMSUT_WINOGRAD=0 changes no answer: the grid misses the Winograd shapes"
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes,", len(data), "arrays")
