"""``k_warp_joint`` and ``k_elastic_nearest`` (csrc/pointwise.hip, through data_loader/gpu_augment.py) against the fp64 references of
``augment_cases.py``, pixel by pixel: no pixel is exempt in any test.  The bounds are derived in that module's docstring, and
``test_augment_cases_cpu.py`` proves what the cases claim (exactness, band shares, that planted faults break the bounds).
Each test prints its worst image error beside its bound and the share of pixels in its band."""
import random

import numpy as np
import pytest
import torch

import augment_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ga():
    import smsut_amd  # noqa: F401
    from smsut_amd.data_loader import gpu_augment
    return gpu_augment


def run_warp(ga, img, msk, aff, ctrl, ho, wo):
    gi, gm = ga.warp_joint(torch.from_numpy(img)[:, None].cuda(), None if msk is None else torch.from_numpy(msk).cuda(),
                           torch.from_numpy(aff), None if ctrl is None else torch.from_numpy(ctrl), ho, wo)
    assert (gm is None) == (msk is None)
    return gi[:, 0].cpu().numpy(), None if gm is None else gm.cpu().numpy()


def run_elastic(ga, img, msk, ctrl):
    gi, gm = ga.elastic_deform(torch.from_numpy(img)[:, None].cuda(), None if msk is None else torch.from_numpy(msk).cuda(),
                               torch.from_numpy(ctrl))
    assert (gm is None) == (msk is None)
    return gi[:, 0].cpu().numpy(), None if gm is None else gm.cpu().numpy()


def bits(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).view(np.int32))


def odd_values(rs, shape):
    """fp32 values that only a bit-for-bit copy keeps: negative ones, subnormals of both signs, ordinary ones"""
    v = rs.standard_normal(shape).astype(np.float32) * 100
    sub = (rs.randint(1, 2 ** 23, shape).astype(np.uint32) | (rs.randint(0, 2, shape).astype(np.uint32) << np.uint32(31))).view(np.float32)
    v = np.where(rs.rand(*shape) < 0.4, sub, v).astype(np.float32)
    assert (v < 0).any() and (np.abs(v) < 2.0 ** -126).mean() > 0.2 and not (v == 0).any()
    return v


# ---- part 1: exact cases, every pixel equal ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.EXACT))
def test_warp_exact_cases(ga, name):
    img, msk, aff, ctrl, ho, wo = C.exact_case(name)
    n, h, w = img.shape
    ri, rm, _ = C.ref_warp(img, msk, aff, ctrl, ho, wo)
    gi, gm = run_warp(ga, img, msk, aff, ctrl, ho, wo)
    # with control displacements the coordinates are exact but the four weight products are not: 8 u max|img| (augment_cases (2))
    bar = 0.0 if ctrl is None else 8 * C.U * float(img.max())
    err = float(np.abs(gi.astype(np.float64) - ri).max())
    print(f"{name}: worst image error {err:.3e} (bar {bar:.3e}), labels differing {int((gm != rm).sum())} of {rm.size}, band share 0 (exact case)")
    assert np.array_equal(gm, rm), np.argwhere(gm != rm)[:5]
    assert err <= bar, np.argwhere(np.abs(gi - ri) > bar)[:5]
    # unlabelled batch: the image is bit-identical; every sample alone: bit-identical to its place in the batch
    ni, _ = run_warp(ga, img, None, aff, ctrl, ho, wo)
    assert torch.equal(bits(ni), bits(gi))
    if 1 < n <= 6:
        for k in range(n):
            sl = slice(k, k + 1)
            for m in (msk[sl], None):
                oi, om = run_warp(ga, img[sl], m, aff[sl], None if ctrl is None else ctrl[sl], ho, wo)
                assert torch.equal(bits(oi), bits(gi[sl])) and (m is None or np.array_equal(om, gm[sl])), (name, k)


def test_warp_copies_values_bit_for_bit(ga):
    """integer translations, flips and the turn have weights 0 and 1: labels up to 2^40 and negative / subnormal image values arrive as
    they are, at the positions the index mask names"""
    H, W = C._H, C._W
    aff = np.asarray([C._t(-1, 0), C._t(3, -2), C.HFLIP, C.VFLIP, C.TURN], dtype=np.float32)
    rs = np.random.RandomState(40)
    img, lab = odd_values(rs, (5, H, W)), rs.randint(-2 ** 40, 2 ** 40, (5, H, W)).astype(np.int64)
    _, idx = run_warp(ga, img, C.index_mask(5, H, W), aff, None, H, W)
    assert np.array_equal(idx, C.ref_warp(img, C.index_mask(5, H, W), aff, None, H, W)[1])
    inside, y, x = C.decode(idx, W)
    n = np.arange(5)[:, None, None]
    gi, gm = run_warp(ga, img, lab, aff, None, H, W)
    assert inside.mean() > 0.8 and np.abs(lab).max() > 2 ** 39
    assert torch.equal(torch.from_numpy(gm), torch.from_numpy(np.where(inside, lab[n, y, x], 0)))
    assert torch.equal(bits(gi), bits(np.where(inside, img[n, y, x], np.float32(0))))


# ---- part 2: drawn rotations and crops, every pixel bounded ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.DRAWN))
def test_warp_drawn_cases(ga, name):
    img, msk, aff, ho, wo = C.drawn_case(name)
    n, h, w = img.shape
    ri, rm, coords = C.ref_warp(img, msk, aff, None, ho, wo)
    gi, gm = run_warp(ga, img, msk, aff, None, ho, wo)
    bound = C.warp_image_bound(img, aff, ho, wo)            # dx Gx + dy Gy + 8 u max|img|, per pixel (augment_cases (1), (2))
    err = np.abs(gi.astype(np.float64) - ri)
    dy, dx = C.warp_label_delta(aff, ho, wo)
    ok, band = C.check_sources(gm, coords, dy, dx, h, w, False)
    print(f"{name}: worst image error {err.max():.3e} (bound there {bound.flat[err.argmax()]:.3e}, worst error / bound {(err / bound).max():.3f}), "
          f"band share {band.mean():.5f}, labels differing from the reference {int((gm != rm).sum())} of {rm.size}, outside the band "
          f"{int((gm != rm)[~band].sum())}")
    assert (err <= bound).all(), np.argwhere(err > bound)[:5]
    assert band.mean() <= 0.01
    assert np.array_equal(gm[~band], rm[~band]) and ok.all(), np.argwhere(~ok)[:5]
    ni, _ = run_warp(ga, img, None, aff, None, ho, wo)
    assert torch.equal(bits(ni), bits(gi))


# ---- part 3: the elastic kernel, every pixel decoded ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(C.ELASTIC))
def test_elastic_cases(ga, name):
    img, msk, ctrl = C.elastic_case(name)
    n, h, w = msk.shape
    coef = ga.spline_prefilter(torch.from_numpy(ctrl)).numpy()
    ri, rm, coords = C.ref_elastic(img, msk, coef)
    gi, gm = run_elastic(ga, img, msk, ctrl)
    d = C.elastic_delta(coef, h, w)                         # u (64 max|coef| + 2 size + 1) per sample and axis (augment_cases (4))
    ok, band = C.check_sources(gm, coords, d[:, 0, None, None], d[:, 1, None, None], h, w, True)
    print(f"{name}: image pixels differing from the reference {int((gi != ri).sum())}, labels {int((gm != rm).sum())} of {rm.size}, outside the "
          f"band {int((gm != rm)[~band].sum())}; delta up to {d.max():.3e}, band share {band.mean():.5f}")
    assert band.mean() <= 0.01
    assert np.array_equal(gi, gm.astype(np.float32)), "image and labels are read at the same source pixel"
    assert np.array_equal(gm[~band], rm[~band]) and np.array_equal(gi[~band], ri[~band]) and ok.all(), np.argwhere(~ok)[:5]
    if name == "zero-samples-0-and-2":
        assert np.array_equal(gm[[0, 2]], msk[[0, 2]]) and np.array_equal(gi[[0, 2]], img[[0, 2]])
    if name == "const+3-2":
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        want = C.index_value(yy + 3, xx - 2, h, w)
        assert np.array_equal(gm[0][~band[0]], want[~band[0]])
    if n > 1:                                                # a sample alone: bit-identical to its place in the batch
        oi, om = run_elastic(ga, img[1:2], msk[1:2], ctrl[1:2])
        assert np.array_equal(oi, gi[1:2]) and np.array_equal(om, gm[1:2])
    if name in C.ELASTIC_NO_MASK:
        ni, _ = run_elastic(ga, img, None, ctrl)
        assert torch.equal(bits(ni), bits(gi))


def test_elastic_copies_values_bit_for_bit(ga):
    img, msk, ctrl = C.elastic_case("P3-64x96")
    n, h, w = msk.shape
    rs = np.random.RandomState(41)
    val, lab = odd_values(rs, (n, h, w)), rs.randint(-2 ** 40, 2 ** 40, (n, h, w)).astype(np.int64)
    _, idx = run_elastic(ga, img, msk, ctrl)
    inside, y, x = C.decode(idx, w)
    k = np.arange(n)[:, None, None]
    gi, gm = run_elastic(ga, val, lab, ctrl)
    assert 0.3 < inside.mean() < 1.0 and np.abs(lab).max() > 2 ** 39
    assert torch.equal(torch.from_numpy(gm), torch.from_numpy(np.where(inside, lab[k, y, x], 0)))
    assert torch.equal(bits(gi), bits(np.where(inside, val[k, y, x], np.float32(0))))
    ni, _ = run_elastic(ga, val, None, ctrl)
    assert torch.equal(bits(ni), bits(gi))


# ---- part 4: the augmenter ------------------------------------------------------------------------------------------------------------------

def _draws(ga, n, hw, out, who_draws, seed):
    """parameters as ``GpuJointAugment.draw`` returns them, with the deformation drawn by the samples in ``who_draws``"""
    state = random.getstate()
    random.seed(seed)
    angs = [random.uniform(-15, 15) for _ in range(n)]
    crops = [ga.resized_crop_params(*hw) for _ in range(n)]
    random.setstate(state)
    ctrl = None
    if who_draws:
        ctrl = torch.zeros(n, 2, 3, 3)
        g = torch.Generator().manual_seed(seed)
        for k in who_draws:
            ctrl[k] = torch.randn(2, 3, 3, generator=g) * 11.0
    return angs, crops, ctrl, (out, out)


@pytest.mark.parametrize("who", [pytest.param((), id="nobody-drew"), pytest.param((0, 1, 2, 3), id="everybody-drew"),
                                 pytest.param((1, 3), id="mixed")])
def test_augmenter_without_a_mask(ga, who):
    """the three branch choices of ``GpuJointAugment.__call__`` on an unlabelled batch: the image is bit-identical to the labelled call's,
    the returned mask is None"""
    from smsut_amd import config as cfg
    aug = ga.GpuJointAugment(dict(cfg.data_aug, resizeCrop_size=48), 48)
    params = _draws(ga, 4, (56, 72), 48, who, 21)
    g = torch.Generator().manual_seed(22)
    x = torch.rand(4, 1, 56, 72, generator=g).cuda()
    y = torch.randint(0, 5, (4, 56, 72), generator=g).cuda()
    xi, yi = aug(x, y, params=params)
    xn, yn = aug(x, None, params=params)
    assert yn is None and tuple(xi.shape) == (4, 1, 48, 48) and tuple(yi.shape) == (4, 48, 48) and yi.dtype == torch.int64
    assert torch.equal(xn.view(torch.int32), xi.view(torch.int32))
    assert float(xi.min()) >= 0.0 and float(xi.max()) <= 1.0 + 1e-6 and int(yi.min()) >= 0 and int(yi.max()) <= 4 and float(xi.std()) > 0.05
    for k in range(4):                                       # and a slice alone, unlabelled, is what it was in the batch
        one = aug(x[k:k + 1], None, params=([params[0][k]], [params[1][k]], params[2][k:k + 1] if k in who else None, params[3]))
        assert one[1] is None and torch.equal(one[0][0], xi[k]), (who, k)


def test_augmenter_three_steps_past_the_grid_cap(ga):
    """N = 9 at 256 x 256 -> 256 x 256, every slice deformed: rotate, elastic, crop + resize each run 589 824 > 524 288 work items; each
    slice is bit-identical to the same slice run alone with the same draws"""
    from smsut_amd import config as cfg
    aug = ga.GpuJointAugment(dict(cfg.data_aug, resizeCrop_size=256), 256)
    params = _draws(ga, 9, (256, 256), 256, tuple(range(9)), 23)
    assert 9 * 256 * 256 > C.EW_CAP_ITEMS
    g = torch.Generator().manual_seed(24)
    x = torch.rand(9, 1, 256, 256, generator=g).cuda()
    y = torch.randint(0, 5, (9, 256, 256), generator=g).cuda()
    xi, yi = aug(x, y, params=params)
    assert float(xi.std()) > 0.05 and int(yi.max()) == 4
    for k in range(9):
        oi, om = aug(x[k:k + 1], y[k:k + 1], params=([params[0][k]], [params[1][k]], params[2][k:k + 1], params[3]))
        assert torch.equal(oi[0].view(torch.int32), xi[k].view(torch.int32)) and torch.equal(om[0], yi[k]), k
