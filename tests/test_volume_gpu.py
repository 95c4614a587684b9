"""The volume-preparation kernels (csrc/volume.hip, ``ops.bspline_coefficients`` / ``resample_volume`` / ``resample_labels`` /
``order_statistics`` / ``window_u8``) and the pipeline of data_pprocess/volume.py against the fp64 oracle of tests/volume_ref.py.

Bars (none taken from the kernels' output): floating-point results |gpu - ref64| <= 16 max|ref32 - ref64| over the tensor, ref32
the fp32 restatement of the oracle on the same inputs; outside points exactly 0.0; labels, order statistics and the 8-bit window
exact.  The float data is not integer-valued: see ``volume_ref.volume``."""
import ctypes

import numpy as np
import pytest
import torch

import volume_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def check(got, ref64, ref32, what):
    got = np.asarray(got, dtype=np.float64)
    err, bar = float(np.abs(got - ref64).max()), R.bar(ref32, ref64)
    print(f"{what}: max|gpu-ref64| {err:.3e}  bar {bar:.3e}  max|ref32-ref64| {bar / 16:.3e}  max|ref64| {np.abs(ref64).max():.3e}")
    assert err <= bar, (what, err, bar)


# every axis takes the lengths {1, 2, 3, 7, 67, 300} while the others stay small; the last shape has more than one tile along the
# line AND across it on both strided passes (csrc/volume.hip: 64 x 64 tiles, 256 outputs a row tile)
PREFILTER_SHAPES = [(5, 7, 300), (300, 3, 5), (4, 300, 6), (1, 2, 67), (2, 1, 3), (3, 5, 1), (7, 3, 2), (2, 67, 7), (67, 2, 3),
                    (70, 130, 70)]


@pytest.mark.parametrize("shape", PREFILTER_SHAPES, ids=["x".join(map(str, s)) for s in PREFILTER_SHAPES])
def test_prefilter(shape):
    from smsut_amd import ops
    v = R.volume(shape, sum(shape))
    got = ops.bspline_coefficients(dev(v))
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == shape
    check(got.cpu().numpy(), R.coefficients(v), R.coefficients(v, np.float32), f"prefilter {shape}")


def test_prefilter_of_a_constant_is_the_constant():
    from smsut_amd import ops
    for shape, c in (((3, 5, 9), 3.7), ((1, 70, 300), -1000.0), ((66, 2, 65), 1e-3)):
        v = np.full(shape, c, dtype=np.float32)
        got = ops.bspline_coefficients(dev(v)).cpu().numpy()
        print(f"constant {c} {shape}: min {got.min()!r} max {got.max()!r}")
        assert (got == np.float32(c)).all()


@pytest.mark.parametrize("shape", [(5, 7, 300), (1, 1, 1), (1, 9, 1), (67, 2, 3)], ids=str)
def test_prefilter_raw_abi_leaves_the_padding_untouched(shape):
    from smsut_amd import _hip as H
    lib, s = H.load(), H.stream_ptr()
    d, h, w = shape
    n, guard = d * h * w, 64
    v = R.volume(shape, 4)
    nbytes = lib.smsut_bspline_ws(d, h, w)
    assert nbytes == n * 4
    vin = torch.full((n + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    vin[:n] = dev(v).reshape(-1)
    out = torch.full((n + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    ws = torch.full((n + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    assert lib.smsut_bspline_coefficients(p(vin), p(out), p(ws), d, h, w, s) == 0
    got = out.cpu().numpy()
    assert (got[n:] == SENTINEL).all() and (ws[n:].cpu().numpy() == SENTINEL).all() and (vin[n:].cpu().numpy() == SENTINEL).all()
    assert np.array_equal(vin[:n].cpu().numpy(), v.reshape(-1))
    check(got[:n].reshape(shape), R.coefficients(v), R.coefficients(v, np.float32), f"raw prefilter {shape}")
    for bad in ((0, h, w), (d, 4097, w)):
        assert lib.smsut_bspline_coefficients(p(vin), p(out), p(ws), *bad, s) == -1


def test_interpolation_returns_the_input():
    from smsut_amd import ops
    for shape in ((9, 40, 37), (1, 5, 130)):
        v = R.volume(shape, 6)
        got = ops.resample_volume(ops.bspline_coefficients(dev(v)), shape, shape, shape, (0, 0, 0))
        ref64, ok = R.resample(R.coefficients(v), shape, shape, shape, (0, 0, 0))
        ref32, _ = R.resample(R.coefficients(v, np.float32), shape, shape, shape, (0, 0, 0), dtype=np.float32)
        assert ok.all() and np.abs(ref64 - v).max() <= 1e-11 * np.abs(v).max()
        check(got.cpu().numpy(), ref64, ref32, f"interpolation {shape}")


# coefficient volume [9, 40, 37] -> window (13, 24, 24): (out_size, num, den, start, offset)
RESAMPLE_CASES = {
    # z up 13/9; y down 40/31 (not an integer ratio) from start 3; x up 160/37 > 2x from start 136: the last two samples are outside
    "forward": ((13, 24, 24), (9, 40, 37), (13, 31, 160), (0, 3, 136), (0, 0, 0)),
    # the restore form: x = i num / den - offset; z starts outside (i = 0: -1) and passes through [-0.5, 0); x runs off the end
    "offset": ((13, 24, 24), (1, 3, 2), (2, 2, 1), (0, 0, 0), (1, 0, 5)),
    "ties": ((13, 24, 24), (1, 1, 1), (2, 2, 2), (0, 0, 0), (0, 0, 0)),
    "one-voxel": ((1, 1, 1), (3, 3, 3), (3, 3, 3), (2, 5, 7), (0, 0, 0)),
}
SRC = (9, 40, 37)


@pytest.mark.parametrize("case", list(RESAMPLE_CASES))
def test_resample_volume(case):
    from smsut_amd import ops
    out_size, num, den, start, off = RESAMPLE_CASES[case]
    coef = (np.random.default_rng(11).standard_normal(SRC) * 500).astype(np.float32)
    got = ops.resample_volume(dev(coef), out_size, num, den, start, off)
    assert got.dtype == torch.float32 and tuple(got.shape) == out_size
    got = got.cpu().numpy()
    ref64, ok = R.resample(coef, out_size, num, den, start, off)
    ref32, _ = R.resample(coef, out_size, num, den, start, off, dtype=np.float32)
    print(f"{case}: {int((~ok).sum())} of {ok.size} points outside")
    check(got, ref64, ref32, f"resample {case}")
    assert (got[~ok] == 0.0).all()
    if case == "forward":
        assert ok[:, :, :22].all() and not ok[:, :, 22:].any()             # x = (i + 136) * 37 / 160 >= 36.5 from i = 22
    if case == "offset":
        assert not ok[0].any() and ok[1:, :, 3:21].all() and not ok[:, :, :3].any() and not ok[:, :, 21:].any()   # x = 2 i - 5
    if case == "one-voxel":
        assert got[0, 0, 0] != 0.0


@pytest.mark.parametrize("case", list(RESAMPLE_CASES))
def test_resample_labels(case):
    from smsut_amd import ops
    out_size, num, den, start, off = RESAMPLE_CASES[case]
    lab = np.random.default_rng(12).integers(0, 256, size=SRC, dtype=np.uint8)
    lut = R.chaos_lut()
    got = ops.resample_labels(dev(lab), out_size, num, den, start, off)
    assert got.dtype == torch.uint8 and tuple(got.shape) == out_size
    want = R.nearest(lab, out_size, num, den, start, off)
    assert np.array_equal(got.cpu().numpy(), want), case
    got_lut = ops.resample_labels(dev(lab), out_size, num, den, start, off, lut=dev(lut))
    assert np.array_equal(got_lut.cpu().numpy(), R.nearest(lab, out_size, num, den, start, off, lut=lut)), case
    if case == "ties":                                                        # x = i / 2: odd i is a tie and takes the upper index
        assert np.array_equal(want[:, 0, 0], lab[(np.arange(13) + 1) // 2, 0, 0])


def test_resample_raw_abi_leaves_the_padding_untouched():
    from smsut_amd import _hip as H
    lib, s = H.load(), H.stream_ptr()
    out_size, num, den, start, off = RESAMPLE_CASES["forward"]
    n, guard = int(np.prod(out_size)), 64
    coef = (np.random.default_rng(11).standard_normal(SRC) * 500).astype(np.float32)
    lab = np.random.default_rng(12).integers(0, 5, size=SRC, dtype=np.uint8)
    nbytes = lib.smsut_resample_ws(*out_size)
    ws = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((n + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    out8 = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    args = (*SRC, *out_size, *num, *den, *start, *off)
    assert lib.smsut_resample_volume(p(dev(coef)), p(out), p(ws), *args, s) == 0
    assert lib.smsut_resample_labels(p(dev(lab)), p(out8), p(ws), None, *args, s) == 0
    assert (out[n:].cpu().numpy() == SENTINEL).all() and (out8[n:].cpu().numpy() == 0xA5).all()
    assert (ws[nbytes:].cpu().numpy() == 0xA5).all()
    assert np.array_equal(out8[:n].cpu().numpy().reshape(out_size), R.nearest(lab, out_size, num, den, start, off))
    bad = list(args)
    bad[9] = 0                                                                # den_z
    before = out.clone()
    assert lib.smsut_resample_volume(p(dev(coef)), p(out), p(ws), *bad, s) == -1
    assert torch.equal(out, before)


def order_data(family, n, rng):
    if family == "mixed":
        return (rng.standard_normal(n) * 1000).astype(np.float32)
    if family == "constant":
        return np.full(n, -7.25, dtype=np.float32)
    if family == "duplicates":                                                # 90 % of the values are one value
        v = (rng.standard_normal(n) * 100).astype(np.float32)
        v[rng.random(n) < 0.9] = np.float32(12.5)
        return v
    v = rng.choice(np.array([0.0, -0.0, 1e-30, -1e-30, 3.0, -3.0], dtype=np.float32), size=n)      # zeros of both signs
    return v


@pytest.mark.parametrize("n", [1, 2, 255, 65537, 300001])
def test_order_statistics_are_exact(n):
    from smsut_amd import ops
    rng = np.random.default_rng(n)
    t = int(np.floor(0.995 * (n - 1)))
    ranks = [0, t, min(t + 1, n - 1), n - 1]
    for family in ("mixed", "constant", "duplicates", "zeros"):
        v = order_data(family, n, rng)
        got = ops.order_statistics(dev(v), ranks)
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (4,)
        want = np.partition(v, ranks)[ranks]
        print(f"order {family} n={n}: gpu {got.cpu().numpy().tolist()} numpy {want.tolist()}")
        assert (got.cpu().numpy() == want).all(), (family, n)
    v = order_data("mixed", n, rng)
    eight = sorted({int(r) for r in rng.integers(0, n, size=8)})
    assert (ops.order_statistics(dev(v).reshape(1, -1), eight).cpu().numpy() == np.sort(v)[eight]).all()
    assert (ops.order_statistics(dev(v), [n - 1]).cpu().numpy() == v.max()).all()


@pytest.mark.parametrize("n", [2, 255, 65537, 300001])
def test_percentile_bounds_within_one_ulp(n):
    from smsut_amd.data_pprocess import volume as V
    rng = np.random.default_rng(n + 1)
    for family in ("mixed", "duplicates"):
        v = order_data(family, n, rng)
        got = V.window_bounds(dev(v), "t2")
        assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (2,)
        want = np.percentile(v.astype(np.float64), [0.05, 99.5])
        got = got.cpu().numpy()
        print(f"percentile {family} n={n}: gpu {got.tolist()} numpy {want.tolist()}")
        for g, w in zip(got, want):
            assert abs(float(g) - w) <= float(np.spacing(np.float32(abs(w)))), (family, n, g, w)
    v = (rng.standard_normal(n) * 900).astype(np.float32)
    ct = V.window_bounds(dev(v), "ct").cpu().numpy()
    assert ct.tolist() == [max(float(v.min()), -1000.0), min(float(v.max()), 400.0)]


def test_window_is_byte_exact():
    from smsut_amd import ops
    rng = np.random.default_rng(21)
    v = (rng.standard_normal(100003) * 300 + 50).astype(np.float32)
    v[:6] = [-120.5, 333.25, -120.49, 333.26, 0.0, -0.0]
    for lo, hi in ((-120.5, 333.25), (-1000.0, 400.0), (0.05, 0.07), (-5000.0, 5000.0)):
        b = np.array([lo, hi], dtype=np.float32)
        want = R.window(v, b[0], b[1], np.float32)
        got = ops.window_u8(dev(v), dev(b))
        assert got.dtype == torch.uint8 and tuple(got.shape) == v.shape
        assert np.array_equal(got.cpu().numpy(), want), (lo, hi)
        assert np.array_equal(ops.window_u8(dev(v)[1:], dev(b)).cpu().numpy(), want[1:])          # a view that is not 16-byte aligned
        vol = ops.window_u8(dev(v[:99999]).reshape(3, 33333), dev(b))
        assert tuple(vol.shape) == (3, 33333) and np.array_equal(vol.cpu().numpy().reshape(-1), want[:99999])
        print(f"window [{lo}, {hi}]: levels used {len(np.unique(want))}, fp64 statement differs in "
              f"{int((R.window(v, b[0], b[1], np.float64) != want).sum())} of {v.size} bytes")
        if (lo, hi) == (-120.5, 333.25):
            assert want[:6].tolist() == [0, 255, 0, 255, 67, 67] and (want.min(), want.max()) == (0, 255)
    for c in (0.0, 17.5):
        assert not ops.window_u8(dev(v), dev(np.array([c, c], dtype=np.float32))).any()            # hi == lo: zeros


def test_window_raw_abi_leaves_the_padding_untouched():
    from smsut_amd import _hip as H
    lib, s = H.load(), H.stream_ptr()
    n, guard = 1027, 64
    v = (np.random.default_rng(22).standard_normal(n) * 300).astype(np.float32)
    b = np.array([-200.0, 250.0], dtype=np.float32)
    out = torch.full((n + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.smsut_window_u8(p(dev(v)), p(dev(b)), p(out), n, s) == 0
    assert (out[n:].cpu().numpy() == 0xA5).all()
    assert np.array_equal(out[:n].cpu().numpy(), R.window(v, b[0], b[1], np.float32))
    assert lib.smsut_window_u8(p(dev(v)), p(dev(b)), p(out), 0, s) == -1


OLD, OLD_SPACING, CROP = (9, 40, 37), (7.7, 1.89, 1.89), 24       # -> new (13, 50, 46), start (0, 13, 11), window (13, 24, 24)


@pytest.mark.parametrize("modality", ["t2", "ct"])
def test_pipeline_is_the_chain_of_its_ops(modality):
    from smsut_amd import ops
    from smsut_amd.data_pprocess import volume as V
    img = R.volume(OLD, 31) - (1024.0 if modality == "ct" else 0.0)              # CT: -1024 .. 3071 spans [-1000, 400]
    raw = np.random.default_rng(32).integers(0, 256, size=OLD, dtype=np.uint8)
    image_u8, label_u8, plan = V.prepare_volume(img, raw, OLD_SPACING, modality, crop_size=CROP, label_lut=V.chaos_label_lut())
    assert plan.new_size == (13, 50, 46) and plan.start == (0, 13, 11) and plan.out_size == (13, 24, 24)
    assert image_u8.dtype == torch.uint8 and image_u8.is_cuda and tuple(image_u8.shape) == plan.out_size
    vol = ops.resample_volume(ops.bspline_coefficients(dev(img)), plan.out_size, OLD, plan.new_size, plan.start)
    n = vol.numel()
    if modality == "ct":
        s = ops.order_statistics(vol, [0, n - 1]).cpu().numpy()
        bounds = np.array([max(s[0], -1000.0), min(s[1], 400.0)], dtype=np.float32)
        assert s[1] > 400.0 and bounds[1] == 400.0
    else:
        bounds = np.percentile(vol.cpu().numpy().astype(np.float64), [0.05, 99.5])
        mine = V.window_bounds(vol, modality).cpu().numpy()
        assert all(abs(float(g) - w) <= float(np.spacing(np.float32(abs(w)))) for g, w in zip(mine, bounds))
        bounds = mine
    want = ops.window_u8(vol, dev(bounds))
    assert torch.equal(image_u8, want)
    assert np.array_equal(image_u8.cpu().numpy(), R.window(vol.cpu().numpy(), bounds[0], bounds[1], np.float32))
    assert torch.equal(label_u8, ops.resample_labels(dev(raw), plan.out_size, OLD, plan.new_size, plan.start, lut=dev(R.chaos_lut())))
    alone, none, plan2 = V.prepare_volume(dev(img), None, OLD_SPACING, modality, crop_size=CROP)
    assert none is None and plan2 == plan and torch.equal(alone, image_u8)
    print(f"pipeline {modality}: bounds {bounds.tolist()}, levels used {len(torch.unique(image_u8))}")


def test_restore_labels_is_the_oracles_two_steps():
    from smsut_amd.data_pprocess import volume as V
    lab = R.blocky_labels(OLD, 41)
    img = R.volume(OLD, 42)
    _, label_u8, plan = V.prepare_volume(img, lab, OLD_SPACING, "t2", crop_size=CROP)
    there = R.nearest(lab, plan.out_size, OLD, plan.new_size, plan.start)
    assert np.array_equal(label_u8.cpu().numpy(), there)
    back = V.restore_labels(label_u8, plan, OLD)
    assert back.dtype == torch.uint8 and tuple(back.shape) == OLD
    want = R.nearest(there, OLD, plan.new_size, OLD, (0, 0, 0), plan.start)
    assert np.array_equal(back.cpu().numpy(), want)
    inside = want != 0
    assert inside.any() and not want[:, :8].any() and not want[:, :, :7].any()      # outside the crop: 0
    print(f"restore: {int(inside.sum())} labelled voxels back, {int((want[inside] == lab[inside]).sum())} equal to the original")
    with pytest.raises(ValueError):
        V.restore_labels(label_u8[:, :-1], plan, OLD)
