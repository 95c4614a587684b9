"""Writes tests/golden/wgrad_plan.npz: what the weight-gradient planning queries of csrc/conv_mfma.hip answer over a grid of layer shapes.

The queries take integers only and launch nothing, so they run without a device, and none of them reads the environment: one
recording.  They answer from the same plan the launches use (wgrad_select, plan_rr, plan_wgrad_f16): which kernel family a shape runs
and how many split slabs it writes.  A workspace query that drifts from its launch lets the launch write more slabs than its caller
allocated, so tests/test_wgrad_plan_cpu.py requires the built library to give exactly these answers.

Grid: ``shapes()`` of make_conv_plan_golden.py, N x (H, W) x Cin x Cout.  Columns (``COLUMNS``), per shape, int64:
  mfma_ws_k{KS}                      smsut_conv2d_wgrad_mfma_ws, KS = 1, 3
  sc, sc_ws                          smsut_conv2d_wgrad_sc_supported / _sc_ws
  f16, f16_ws, sc_f16, sc_f16_ws     smsut_conv2d_wgrad_f16_supported / _f16_ws / _sc_f16_supported / _sc_f16_ws
  pair_{c}{a}{s}, pair_ws_{c}{a}{s}  smsut_conv2d_wgrad_pair_supported / _pair_ws with NA = NB = N and (cat, aff, sc) = (c, a, s):
                                     the five forms of ``PAIR_FORMS`` and the two rejected ones of ``PAIR_REJECTED``

    python tests/golden/make_wgrad_plan_golden.py        # rewrites tests/golden/wgrad_plan.npz from the built library
"""
import ctypes
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(ROOT, "smsut-medicalimgsegmentation_amd", "lib", "libsmsut_hip.so")
OUT = os.path.join(HERE, "wgrad_plan.npz")

_spec = importlib.util.spec_from_file_location("make_conv_plan_golden", os.path.join(HERE, "make_conv_plan_golden.py"))
_conv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_conv)
shapes = _conv.shapes                            # the conv-plan grid: NS x PLANES x CHANNELS x CHANNELS

PAIR_FORMS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1))      # (cat, aff, sc)
PAIR_REJECTED = ((1, 1, 0), (0, 1, 1))

COLUMNS = (["mfma_ws_k1", "mfma_ws_k3", "sc", "sc_ws", "f16", "f16_ws", "sc_f16", "sc_f16_ws"] +
           [f"{q}_{c}{a}{s}" for c, a, s in PAIR_FORMS + PAIR_REJECTED for q in ("pair", "pair_ws")])
SUPPORTED = ["sc", "f16", "sc_f16"] + [f"pair_{c}{a}{s}" for c, a, s in PAIR_FORMS]      # must hold a 0 and a 1 over the grid
REJECTED = [f"pair_{c}{a}{s}" for c, a, s in PAIR_REJECTED]                             # 0 everywhere


def answers(lib_path=LIB):
    """[shapes, columns] int64 from the library at lib_path."""
    lib = ctypes.CDLL(lib_path)

    def q(name, ws):
        f = getattr(lib, "smsut_conv2d_wgrad_" + name)
        f.restype = ctypes.c_int64 if ws else ctypes.c_int
        return f
    mfma_ws, sc, sc_ws = q("mfma_ws", True), q("sc_supported", False), q("sc_ws", True)
    f16, f16_ws, sc_f16, sc_f16_ws = q("f16_supported", False), q("f16_ws", True), q("sc_f16_supported", False), q("sc_f16_ws", True)
    pair, pair_ws = q("pair_supported", False), q("pair_ws", True)
    rows = []
    for n, h, w, ci, co in shapes():
        s = (n, h, w, ci, co)
        row = [mfma_ws(*s, 1), mfma_ws(*s, 3), sc(*s), sc_ws(*s), f16(*s), f16_ws(*s), sc_f16(*s), sc_f16_ws(*s)]
        for form in PAIR_FORMS + PAIR_REJECTED:
            row += [pair(n, n, h, w, ci, co, *form), pair_ws(n, n, h, w, ci, co, *form)]
        rows.append(row)
    out = np.array(rows, dtype=np.int64)
    assert out.shape == (len(shapes()), len(COLUMNS))
    return out


if __name__ == "__main__":
    plan = answers(sys.argv[1] if len(sys.argv) > 1 else LIB)
    for name in SUPPORTED:
        col = plan[:, COLUMNS.index(name)]
        assert set(np.unique(col).tolist()) == {0, 1}, f"{name}: the grid misses a family (values {np.unique(col).tolist()})"
    for name in REJECTED:
        assert not plan[:, COLUMNS.index(name)].any(), f"{name}: a rejected form is reported as supported"
    np.savez_compressed(OUT, columns=np.array(COLUMNS), shapes=np.array(shapes(), dtype=np.int32), plan=plan)
    print(OUT, os.path.getsize(OUT), "bytes")
