"""CPU checks of the dual-task-consistency references (tests/dtc_ref.py) and of the fixture tests/golden/dtc.npz: the separable numpy
distance transform against brute force and scipy, the inner-boundary identity, the fixture's arrays, and the workspace query of the
library (no device work)."""
import ctypes

import numpy as np
import pytest
import torch

import dtc_ref as R


def small_masks():
    rs = np.random.RandomState(3)
    out = []
    for h, w in ((1, 1), (1, 9), (9, 1), (5, 7), (16, 16), (24, 24), (13, 24)):
        for dens in (0.05, 0.5, 0.95):
            out.append(rs.uniform(size=(h, w)) < dens)
        out.append(np.zeros((h, w), dtype=bool))
        out.append(np.ones((h, w), dtype=bool))
        one = np.zeros((h, w), dtype=bool); one[h - 1, w - 1] = True
        out.append(one)
    return out


def test_separable_edt_equals_brute_force():
    for p in small_masks():
        assert np.array_equal(R.edt_sq_masks(p), R.edt_sq_brute(p)), p.shape
    lab = R.label_pattern("blobs", 2, 3, 20, 23)
    d2 = R.edt_sq(lab, 3)
    for b in range(2):
        for c in range(3):
            assert np.array_equal(d2[b, c], R.edt_sq_brute(lab[b] == c))


def test_inner_boundary_is_members_at_distance_one():
    for p in small_masks():
        d2 = R.edt_sq_masks(p)
        assert np.array_equal(p & (d2 == 1), R.inner_boundary_morph(p)), p.shape
    for name in R.PATTERNS:
        lab = R.label_pattern(name, 2, 4, 33, 47)
        p = R.class_masks(lab, 4)
        d2 = R.edt_sq_masks(p)
        for b in range(2):
            for c in range(4):
                assert np.array_equal(p[b, c] & (d2[b, c] == 1), R.inner_boundary_morph(p[b, c])), (name, b, c)


def test_sdf_rules():
    lab = R.label_pattern("absent", 2, 4, 30, 30)
    d2, sdf = R.sdf(lab, 4)
    p = R.class_masks(lab, 4)
    assert np.all(sdf[:, 1] == 1.0) and np.all(d2[:, 1] == 0)                       # class 1 absent
    assert np.all(sdf[-1, 0] == -1.0) and np.all(sdf[-1, 1:] == 1.0)               # the all-background slice: full and empty
    assert np.all(sdf[p] <= 0.0) and np.all(sdf[~p] > 0.0) and np.all(np.abs(sdf) <= 1.0)
    assert sdf[0, 0].min() == -1.0 and sdf[0, 0].max() == 1.0                      # both sides reach their maximum
    lab = R.label_pattern("checker", 1, 2, 8, 9)
    d2, sdf = R.sdf(lab, 2)
    assert np.all(d2 == 1) and np.all(sdf[R.class_masks(lab, 2)] == 0.0) and np.all(sdf[~R.class_masks(lab, 2)] == 1.0)
    lab = R.label_pattern("corner", 1, 2, 12, 7)
    assert R.edt_sq(lab, 2)[0, 1, 0, 0] == 11 * 11 + 6 * 6


def test_fixture_reproduces_from_dtc_ref(golden):
    g = golden("dtc")
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for i, (pat, b, c, h, w) in enumerate(R.SDF_FIXTURE):
        lab = R.label_pattern(pat, b, c, h, w, seed=50 + i)
        assert np.array_equal(lab.astype(np.uint8), g[f"sdf{i}_labels"])
        d2, sdf = R.sdf(lab, c)
        st = R.SDF_STRIDE if h * w > 128 * 128 else 1
        assert np.array_equal(d2[:, :, ::st, ::st], g[f"sdf{i}_d2"]), i
        assert np.abs(sdf[:, :, ::st, ::st] - g[f"sdf{i}_sdf"].astype(np.float64)).max() <= 2.0 ** -24, i   # stored rounded to fp32
        if ndimage is not None:
            for bi in range(b):
                for ci in range(c):
                    p = lab[bi] == ci
                    if p.any() and not p.all():
                        ref = np.where(p, ndimage.distance_transform_edt(p), ndimage.distance_transform_edt(~p)) ** 2
                        assert np.array_equal(np.rint(ref).astype(np.int32), d2[bi, ci]), (i, bi, ci)
    assert list(g["keys"]) == list(R.shapes().keys())
    for row, shp in zip(g["shapes"], R.shapes().values()):
        assert tuple(int(v) for v in row[:len(shp)]) == tuple(shp)
    assert g["fwd_tanh"].shape == (2, R.C, R.SIZE, R.SIZE) and np.abs(g["fwd_tanh"]).max() <= 1.0
    assert g["scalars32"].shape == (2, 3) and np.abs(g["scalars32"] - g["scalars64"]).max() < 1e-4


def test_loss_restatement_and_case_draw():
    """The fp64 restatement is finite at t = +-1 (k t = +-1500), and the draw of the GPU test exercises the unsaturated sigmoid: the
    gradient of the consistency term to t is non-zero on at least a quarter of the pixels."""
    for shape in R.LOSS_SHAPES[:4]:
        n, b, c, h, w = shape
        t, z, s = R.loss_case(n, b, c, h, w, 5)
        td = t.double().requires_grad_(True)
        out = R.dtc_loss(td, z.double(), s.double(), R.K)
        out[1].backward()
        assert torch.isfinite(out).all()
        assert float((td.grad != 0).double().mean()) >= 0.25, shape
    t = torch.tensor([1.0, -1.0, 0.0]).reshape(1, 1, 1, 3).double()
    out = R.dtc_loss(t, torch.zeros_like(t), t.clone(), R.K)
    assert torch.isfinite(out).all() and out[0].item() == 0.0
    want = ((torch.sigmoid(-R.K * t) - 1.0) ** 2).mean().item()                  # softmax over one channel is 1
    assert abs(out[1].item() - want) < 1e-15


def test_sdf_workspace_query_without_gpu():
    import __graft_entry__ as ge
    ge.build()
    lib = ctypes.CDLL(ge.LIB)
    f = lib.smsut_sdf_ws
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int] * 4
    base = (2, 3, 100, 100)
    assert f(*base) > 0
    for axis, values in enumerate(((1, 2, 8, 64), (1, 2, 5, 16), (1, 17, 256, 512), (1, 64, 65, 300, 512))):
        sizes = []
        for v in values:
            args = list(base); args[axis] = v
            sizes.append(f(*args))
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1], (axis, sizes)
    assert f(8, 5, 256, 256) * 4 < 1 << 20                                          # the workload: under 1 MB
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 17, 8, 8), (1, 3, 0, 8), (1, 3, 513, 8), (1, 3, 8, 0), (1, 3, 8, 513)):
        assert f(*bad) == -1, bad
    g = lib.smsut_dtc_ws
    g.restype = ctypes.c_int64
    g.argtypes = [ctypes.c_int, ctypes.c_int64]
    assert 0 < g(1, 64) <= g(2, 64) <= g(2, 65536) <= g(16, 65536)
