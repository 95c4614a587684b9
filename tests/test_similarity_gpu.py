"""The translation-metric kernel (csrc/similarity.hip, ``ops.image_similarity``) against the fp64 reference of tests/ssim_ref.py.

Bars (none of them taken from the kernel's output):
  SSIM   per-slice mean = out[:, 0] / ((H-10)(W-10)); |gpu - ref64| <= max(16 |ref32 - ref64|, 16 * 2^-23), where ref32 is the
         float32 restatement of the same expression evaluated on the same inputs: 16 times the reference's own rounding.
  SE, AE relative error <= H W 2^-52 against the fp64 sums (both sides add fp64 values of the same differences; only the order
         of the additions differs); exactly 0.0 for identical inputs."""
import ctypes

import numpy as np
import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def p(t):
    return ctypes.c_void_p(t.data_ptr())


def check_rows(got, h, w, s64, s32, se, ae, what):
    got = np.asarray(got)
    assert got.shape == (len(s64), 3) and got.dtype == np.float64
    for n in range(len(s64)):
        ssim = got[n, 0] / ((h - 10) * (w - 10))
        err, bar = abs(ssim - s64[n]), R.ssim_bar(s32[n], s64[n])
        print(f"{what} slice {n}: ssim {ssim:.9f} ref64 {s64[n]:.9f} |err| {err:.2e} bar {bar:.2e} |ref32-ref64| {abs(s32[n] - s64[n]):.2e}")
        assert err <= bar, (what, n, ssim, s64[n], s32[n])
        tol = h * w * 2.0 ** -52
        assert abs(got[n, 1] - se[n]) <= tol * se[n], (what, n, got[n, 1], se[n])
        assert abs(got[n, 2] - ae[n]) <= tol * ae[n], (what, n, got[n, 2], ae[n])
        if se[n] == 0.0:
            assert got[n, 1] == 0.0 and got[n, 2] == 0.0


@pytest.mark.parametrize("hw", R.shapes(), ids=[f"{h}x{w}" for h, w in R.shapes()])
def test_every_family_at_every_shape(hw):
    from smsut_amd import ops
    h, w = hw
    for family in R.FAMILIES:
        for n in (1, 3) + ((8,) if hw == (256, 256) else ()):
            a, b, s64, s32, se, ae = R.batch(family, h, w, n)
            out = ops.image_similarity(dev(a), dev(b), 1.0)
            assert out.dtype == torch.float64 and out.is_cuda and tuple(out.shape) == (n, 3)
            check_rows(out.cpu().numpy(), h, w, s64, s32, se, ae, f"{family} {h}x{w} N={n}")
            if family in ("identical", "constant"):
                assert (out[:, 0].cpu().numpy() == float((h - 10) * (w - 10))).all()      # SSIM exactly 1 at every centre


@pytest.mark.parametrize("hw", R.SCALED_SHAPES, ids=[f"{h}x{w}" for h, w in R.SCALED_SHAPES])
def test_data_range_255(hw):
    from smsut_amd import ops
    h, w = hw
    for family in R.FAMILIES:
        a, b, s64, s32, se, ae = R.batch(family, h, w, 3, 255.0)
        out = ops.image_similarity(dev(a), dev(b), 255.0)
        check_rows(out.cpu().numpy(), h, w, s64, s32, se, ae, f"{family} {h}x{w} x255")


def test_every_pixel_is_owned_by_exactly_one_workgroup():
    """a = b except ONE pixel per slice; the pixel sits at every corner, at the edge midpoints and around each boundary between the
    tiles' own regions (similarity.hip: the own rows of tile ty are 5 + ty TH .. 5 + (ty+1) TH - 1, the edge tiles take the 5-pixel
    frame; columns alike): SE is that pixel's squared difference -- not 0, not twice it."""
    from smsut_amd import ops
    h, w = 2 * R.TH + 13, 2 * R.TW + 13                       # 3 x 3 tiles
    ys_b = [5 + R.TH - 1, 5 + R.TH, 5 + 2 * R.TH - 1, 5 + 2 * R.TH]
    xs_b = [5 + R.TW - 1, 5 + R.TW, 5 + 2 * R.TW - 1, 5 + 2 * R.TW]
    pos = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2), (h // 2, 0), (h // 2, w - 1)]
    pos += [(y, x) for y in ys_b for x in xs_b]
    pos += [(y, x) for y in ys_b for x in (0, 4, 5, w // 2, w - 6, w - 5, w - 1)]
    pos += [(y, x) for x in xs_b for y in (0, 4, 5, h // 2, h - 6, h - 5, h - 1)]
    base, _ = R.make_pair("independent", h, w, 11)
    a = np.repeat(base[None], len(pos), 0)
    b = a.copy()
    for n, (y, x) in enumerate(pos):
        b[n, y, x] = np.float32(1.0) - b[n, y, x] * np.float32(0.5)
    out = ops.image_similarity(dev(a), dev(b), 1.0).cpu().numpy()
    for n, (y, x) in enumerate(pos):
        d = float(a[n, y, x]) - float(b[n, y, x])
        assert d != 0.0
        assert out[n, 1] == d * d and out[n, 2] == abs(d), (y, x, out[n], d * d)
        s64, s32 = R.ssim_mean(a[n], b[n]), R.ssim_mean(a[n], b[n], np.float32)
        assert abs(out[n, 0] / ((h - 10) * (w - 10)) - s64) <= R.ssim_bar(s32, s64), (y, x)


def test_a_nan_stays_in_its_slice():
    from smsut_amd import ops
    h, w = R.TH + 11, R.TW + 11                                # four workgroups per slice
    a, b, *_ = R.batch("perturbed", h, w, 3)
    clean = ops.image_similarity(dev(a), dev(b), 1.0).cpu().numpy()
    for bad in (np.nan, np.inf):
        a2 = a.copy()
        a2[1, h // 2, w // 2] = bad
        got = ops.image_similarity(dev(a2), dev(b), 1.0).cpu().numpy()
        assert np.isnan(got[1, 0]) and not np.isfinite(got[1, 1]) and not np.isfinite(got[1, 2])
        assert got[0].tobytes() == clean[0].tobytes() and got[2].tobytes() == clean[2].tobytes()


@pytest.mark.parametrize("nhw", [(3, 13, 13), (2, R.TH + 11, R.TW + 11), (3, 43, 42)])
def test_raw_abi_writes_only_its_rows_and_repeats_bitwise(nhw):
    from smsut_amd import _hip as H
    n, h, w = nhw
    lib, s = H.load(), H.stream_ptr()
    a, b, s64, s32, se, ae = R.batch("grid8", h, w, n)
    ad, bd = dev(a), dev(b)
    nbytes = lib.smsut_image_similarity_ws(n, h, w)
    assert nbytes > 0 and nbytes % 24 == 0
    guard = 64
    ws = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = []
    for fill in (SENTINEL, 7.0):                               # two different pre-fills: the result is written, not accumulated
        out = torch.full((n * 3 + guard,), fill, dtype=torch.float64, device="cuda")
        assert lib.smsut_image_similarity(p(ad), p(bd), p(out), p(ws), n, h, w, 1.0, s) == 0
        got = out.cpu().numpy()
        assert (got[n * 3:] == fill).all()
        assert (ws[nbytes:].cpu().numpy() == 0xA5).all()
        outs.append(got[:n * 3].copy())
    assert outs[0].tobytes() == outs[1].tobytes()
    check_rows(outs[0].reshape(n, 3), h, w, s64, s32, se, ae, f"raw {nhw}")


def test_invalid_arguments_leave_out_untouched():
    from smsut_amd import _hip as H
    lib, s = H.load(), H.stream_ptr()
    a = torch.zeros(2 * 4097 * 11, dtype=torch.float32, device="cuda")
    out = torch.full((6,), SENTINEL, dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    for n, h, w, dr in ((2, 10, 64, 1.0), (2, 11, 4097, 1.0), (0, 16, 16, 1.0), (2, 16, 16, 0.0)):
        assert lib.smsut_image_similarity(p(a), p(a), p(out), p(ws), n, h, w, dr, s) == -1, (n, h, w, dr)
        assert lib.smsut_image_similarity_ws(n, h, w) == (-1 if dr else 2 * 24)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()


def test_python_entry_shapes_and_the_utils_functions():
    from smsut_amd import ops
    from smsut_amd.misc import utils
    h, w = 43, 42
    a, b, s64, s32, se, ae = R.batch("perturbed", h, w, 3)
    want = ops.image_similarity(dev(a), dev(b), 1.0)
    assert torch.equal(ops.image_similarity(dev(a)[:, None], dev(b)[:, None], 1.0), want)             # [N, 1, H, W]
    wide_a, wide_b = dev(np.concatenate([a, a], 2)), dev(np.concatenate([b, b], 2))
    assert torch.equal(ops.image_similarity(wide_a[:, :, :w], wide_b[:, :, w:], 1.0), want)           # made contiguous
    bar = max(R.ssim_bar(x, y) for x, y in zip(s32, s64))
    assert abs(utils.ssim(a, b, 1.0) - float(np.mean(s64))) <= bar                                    # a volume: mean of its slices
    assert abs(utils.ssim(dev(a[0]), dev(b[0]), 1.0) - s64[0]) <= R.ssim_bar(s32[0], s64[0])          # one image, device tensors
    tol = 3 * h * w * 2.0 ** -52
    mse = sum(se) / (3 * h * w)
    assert utils.psnr(a, b, 1.0) == pytest.approx(10 * np.log10(1.0 / mse), rel=1e-9)
    assert utils.psnr(a * 255, b * 255, 255.0) == pytest.approx(10 * np.log10(1.0 / mse), rel=1e-6)
    assert utils.mae(a, b) == pytest.approx(sum(ae) / (3 * h * w), rel=tol)
    assert utils.psnr(a, a, 1.0) == float("inf") and utils.mae(a, a) == 0.0 and utils.ssim(a, a, 1.0) == 1.0
    with pytest.raises(TypeError):
        utils.ssim(torch.from_numpy(a), torch.from_numpy(b), 1.0)                                     # a CPU tensor is not moved silently
    with pytest.raises(ValueError):
        utils.mae(a, b[:, :, :-1])
