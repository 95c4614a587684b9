"""The reference of the translation metrics (tests/ssim_ref.py) checked against itself and against the filter form skimage uses;
also that the package carries the feature's public names (the flag, the utils functions, ``ops.image_similarity``)."""
import numpy as np
import pytest

import ssim_ref as R

SHAPES = ((11, 11), (12, 37), (23, 31), (43, 42), (64, 64))


@pytest.mark.parametrize("family", R.FAMILIES)
def test_valid_window_form_equals_the_reflect_filter_form_cropped(family):
    for h, w in SHAPES:
        a, b = R.make_pair(family, h, w, 3)
        assert abs(R.ssim_mean(a, b) - R.ssim_scipy(a, b)) <= 1e-14, (family, h, w)
        a255, b255 = a.astype(np.float64) * 255, b.astype(np.float64) * 255
        assert abs(R.ssim_mean(a255, b255, data_range=255.0) - R.ssim_scipy(a255, b255, 255.0)) <= 1e-14, (family, h, w)


def test_identical_and_constant_pairs_give_exactly_one():
    for h, w in SHAPES:
        for family in ("identical", "constant"):
            a, b = R.make_pair(family, h, w, 1)
            for dt in (np.float64, np.float32):
                m = R.ssim_map(a, b, dt)
                assert m.shape == (h - 10, w - 10) and (m == 1.0).all(), (family, h, w, dt)
            assert R.se_ae(a, b) == (0.0, 0.0)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_symmetric_in_its_arguments(family):
    for h, w in SHAPES:
        a, b = R.make_pair(family, h, w, 5)
        assert R.ssim_mean(a, b) == R.ssim_mean(b, a)
        assert R.se_ae(a, b) == R.se_ae(b, a)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_scaling_images_and_range_by_255_keeps_ssim(family):
    for h, w in SHAPES:
        a, b = R.make_pair(family, h, w, 7)
        a, b = a.astype(np.float64), b.astype(np.float64)
        assert abs(R.ssim_mean(a * 255, b * 255, data_range=255.0) - R.ssim_mean(a, b)) < 1e-12, (family, h, w)


def test_one_window_closed_form():
    """11 x 11: ONE window.  a = a0 + p u (x) v, b = b0 + q u (x) v with u, v of window-weighted mean 0: then mu_a = a0, mu_b = b0,
    s_a^2 = p^2 E, s_b^2 = q^2 E, s_ab = p q E with E = (sum w u^2)(sum w v^2), all by hand."""
    w = R.window()
    assert w.shape == (11,) and abs(w.sum() - 1.0) < 1e-15 and (w == w[::-1]).all()
    k = np.arange(-5, 6, dtype=np.float64)
    u, v = k.copy(), np.sign(k)                       # odd sequences: their weighted mean under the symmetric window is 0
    a0, b0, p, q = 0.4, 0.55, 0.03, -0.02
    a, b = a0 + p * np.outer(u, v), b0 + q * np.outer(u, v)
    e = (w * u * u).sum() * (w * v * v).sum()
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    want = ((2 * a0 * b0 + c1) * (2 * p * q * e + c2)) / ((a0 * a0 + b0 * b0 + c1) * (p * p * e + q * q * e + c2))
    m = R.ssim_map(a, b)
    # (E_w[a^2] - mu_a^2 cancels 0.3 down to 3e-3: 2^-53 * 0.3 / 3e-3 = 1e-14 relative per moment, a few of them: 1e-12 is the bar)
    assert m.shape == (1, 1) and abs(m[0, 0] - want) < 1e-12
    assert -1.0 < want < 0.0                          # p q < 0: the two images are anti-correlated
    se, ae = R.se_ae(a, b)
    d = (a0 - b0) + (p - q) * np.outer(u, v)
    assert abs(se - (d * d).sum()) <= 1e-13 * se and abs(ae - np.abs(d).sum()) <= 1e-13 * ae


def test_float32_restatement_stays_near_fp64_and_the_bar_has_a_floor():
    worst = 0.0
    for family in R.FAMILIES:
        for h, w in SHAPES:
            _, _, s64, s32, _, _ = R.case(family, h, w, 0)
            worst = max(worst, abs(s32 - s64))
            assert R.ssim_bar(s32, s64) >= 16 * 2.0 ** -23
    assert worst < 1e-5


def test_shape_table_covers_the_tile_edges():
    import os
    import re
    import __graft_entry__ as ge
    src = open(os.path.join(ge.CSRC, "similarity.hip")).read()
    m = re.search(r"constexpr int TH = (\d+), TW = (\d+);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (R.TH, R.TW)
    sh = R.shapes()
    assert len(sh) == len(set(sh)) and all(11 <= h <= 256 and 11 <= w <= 300 for h, w in sh)
    for s in ((R.TH + 10, R.TW + 10), (R.TH + 11, R.TW + 9), (2 * R.TH + 13, 2 * R.TW + 13), (11, 11), (13, 13), (21, 300), (256, 256)):
        assert s in sh


def test_package_carries_the_feature():
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg, ops
    from smsut_amd.misc import utils
    assert cfg.test_translation is False and tuple(cfg.test_translation_pairs) == (("t1in", "t1out"),)
    for name in ("ssim", "psnr", "mae", "TranslationMeter", "translation_tables", "translation_text"):
        assert callable(getattr(utils, name))
    assert callable(ops.image_similarity)
