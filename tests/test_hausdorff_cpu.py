"""tests/golden/hausdorff.npz (Hausdorff / HD95 fixture): it is self-consistent, its designed cases say what they were built to
say, its generator reproduces it where scipy is installed; and the host side of the feature without a device."""
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def fx(golden):
    return golden("hausdorff")


def test_fixture_is_self_consistent(fx):
    assert set(str(n) for n in fx["own"]) <= set(str(n) for n in fx["names"])
    for n in fx["names"]:
        six, hd, hd95 = fx[f"hd6_{n}"], fx[f"hd_{n}"], fx[f"hd95_{n}"]
        assert six.shape == (4, 6) and hd.shape == (4,) and hd95.shape == (4,)
        assert np.array_equal(six, np.rint(six))
        for l in range(4):
            n_pg, n_gp, m_pg, m_gp, lo2, hi2 = six[l]
            if n_pg == 0 or n_gp == 0:
                assert (six[l, 2:] == -1).all() and np.isnan(hd[l]) and np.isnan(hd95[l]), (n, l)
                continue
            assert 0 <= lo2 <= hi2 <= max(m_pg, m_gp), (n, l)
            assert hd[l] == np.sqrt(max(m_pg, m_gp)), (n, l)
            assert np.sqrt(lo2) <= hd95[l] <= np.sqrt(hi2) and hd95[l] <= hd[l], (n, l)


def test_designed_cases_are_what_they_claim(fx):
    assert fx["hd6_blobs_a"][1, 4:].tolist() == [66, 67] and fx["hd6_blobs_a"][1, :2].sum() == 5244
    assert fx["hd6_blobs_b"][2, 4:].tolist() == [77, 78]                       # two ranks, two values: the lerp matters
    assert fx["hd6_pair3"][0].tolist() == [1, 1, 9, 9, 9, 9] and fx["hd_pair3"][0] == 3.0 and fx["hd95_pair3"][0] == 3.0
    assert fx["hd6_far_pair"][0].tolist() == [1, 1, 25601, 25601, 25601, 25601] and 25601 >= 1 << 13
    assert fx["hd_far_pair"][0] == np.sqrt(25601.0) and fx["hd95_far_pair"][0] == np.sqrt(25601.0)
    s = fx["hd6_straddle"][0]
    assert s.tolist() == [1, 2, 0, 16389, 0, 16389] and int(s[4]) >> 13 != int(s[5]) >> 13      # ranks in different buckets
    assert abs(fx["hd95_straddle"][0] - 0.9 * np.sqrt(16389.0)) < 1e-9 and abs(fx["hd_straddle"][0] - 128.0195) < 1e-4
    s = fx["hd6_slant"][0]
    assert all(8192 <= v < 16384 for v in s[2:]) and s[4] != s[5]              # second level inside a high bucket
    assert fx["hd6_long_line"][0].tolist() == [1, 1] + [4095 ** 2] * 4 and fx["hd_long_line"][0] == 4095.0
    assert fx["hd6_nested"][0, 2:4].tolist() == [25, 50] and fx["hd_nested"][0] == np.sqrt(50.0)
    o = fx["hd6_one_sided"]
    assert o[1].tolist() == [9, 0, -1, -1, -1, -1] and o[2].tolist() == [0, 9, -1, -1, -1, -1] and o[0, 2] > 0
    for m in ("hdm_hd", "hdm_hd95"):
        assert fx[m].shape == (5, 5) and np.isfinite(fx[m]).all()
    assert (fx["hdm_hd95"] <= fx["hdm_hd"]).all()


def test_fixture_is_small():
    from conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "hausdorff.npz")) < 100 * 1024


def test_generator_reproduces_fixture(fx):
    pytest.importorskip("scipy")
    import importlib.util
    from conftest import GOLDEN
    spec = importlib.util.spec_from_file_location("make_hausdorff_golden", os.path.join(GOLDEN, "make_hausdorff_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    data = gen.build()
    assert sorted(data) == sorted(fx.files)
    for k, v in data.items():
        np.testing.assert_array_equal(np.asarray(v), fx[k], err_msg=k)


def test_config_switch_exists_and_is_off():
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    assert cfg.test_hausdorff is False


def test_host_side_formulas():
    """hd and the percentile from one row of six integers: the square root of the larger maximum; numpy's linear interpolation
    between the two order statistics."""
    import smsut_amd  # noqa: F401
    from smsut_amd.misc import utils
    assert utils._hd_of(np.array([1, 121, 25, 50, 50, 50.0])) == np.sqrt(50.0)
    row = np.array([1, 2, 0, 16389, 0, 16389.0])                    # the pool {0, 0, 16389}
    want = np.percentile(np.sqrt([0.0, 0.0, 16389.0]), 95)
    assert abs(utils._percentile_of(row, 0.95) - want) <= 1e-9 * want
    assert utils._percentile_of(np.array([1, 1, 9, 9, 9, 9.0]), 0.95) == 3.0


def test_metrics_fail_loudly_without_a_device():
    import torch
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    from smsut_amd.misc import utils
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    m = np.zeros((4, 4), np.uint8)
    m[1, 1] = 1
    for f in (utils.hd, utils.hd95, utils.asd):
        with pytest.raises(_hip.SmsutHipError):
            f(m, m)
    with pytest.raises(_hip.SmsutHipError):
        utils.get_hd_matrix({"ct_000": m[None]}, {"ct_000": m[None]})
