"""Voxel spacing of the surface metrics, the host side without a device: the spacing normalisation and the per-volume lookup raise
or return as specified before anything touches the GPU; tests/golden/spacing.npz says what it was built to say and its
generator reproduces it where scipy is installed."""
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def fx(golden):
    return golden("spacing")


def test_voxelspacing_normalisation():
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip, ops
    from smsut_amd.misc import utils
    assert utils._voxelspacing(None, 3) is None
    assert utils._voxelspacing(2.5, 3) == (2.5, 2.5, 2.5) and utils._voxelspacing(np.float32(0.5), 2) == (0.5, 0.5)
    assert utils._voxelspacing([5, 1.25, 0.7], 3) == (5.0, 1.25, 0.7) and utils._voxelspacing(np.array([2.0, 3.0]), 2) == (2.0, 3.0)
    assert all(type(v) is float for v in utils._voxelspacing(np.array([1, 2, 3]), 3))
    assert ops.check_spacing((1e-100, 1.0, 1e100), 3) == (1e-100, 1.0, 1e100)
    for sp, nd in (((1.0, 2.0), 3), ((1.0, 2.0, 3.0), 2), ((1.0,), 3), ((), 2)):
        with pytest.raises(RuntimeError, match="length equal to input rank") as e:
            utils._voxelspacing(sp, nd)
        assert not isinstance(e.value, _hip.SmsutHipError)
        with pytest.raises(RuntimeError, match="length equal to input rank"):
            ops.check_spacing(sp, nd)
    with pytest.raises(RuntimeError):
        ops.check_spacing(2.0, 3)                                  # ops takes a sequence; the scalar form is medpy's, in utils
    for bad in (0.0, -1.0, float("inf"), -float("inf"), float("nan"), 1e-101, 1e101):
        with pytest.raises(ValueError):
            utils._voxelspacing(bad, 3)
        with pytest.raises(ValueError):
            utils._voxelspacing((1.0, bad, 1.0), 3)
        with pytest.raises(ValueError):
            ops.check_spacing((1.0, bad), 2)


def test_metric_functions_check_the_spacing_before_the_device():
    """A bad ``voxelspacing`` raises its own error with or without a device: here, without one, it must not be the 'no HIP
    device' error, which comes from the first upload."""
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    from smsut_amd.misc import utils
    m2 = np.zeros((4, 5), np.uint8)
    m2[1, 1] = 1
    m3 = np.zeros((2, 4, 5), np.uint8)
    m3[1, 1, 1] = 1
    for f in (utils.assd, utils.asd, utils.hd, utils.hd95):
        for m, sp in ((m2, (1.0, 2.0, 3.0)), (m3, (1.0, 2.0)), (m3, [1.0])):
            with pytest.raises(RuntimeError, match="length equal to input rank") as e:
                f(m, m, voxelspacing=sp)
            assert not isinstance(e.value, _hip.SmsutHipError)
        for bad in (0.0, -0.5, float("inf"), float("nan")):
            with pytest.raises(ValueError):
                f(m3, m3, voxelspacing=(1.0, 1.0, bad))
            with pytest.raises(ValueError):
                f(m2, m2, bad)                                     # medpy's keyword position: the third argument


def test_spacing_lookup_by_volume_then_modality():
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    from smsut_amd.misc import utils
    keys = ["ct_000", "ct_001", "t2_004"]
    assert utils._spacings_for(None, keys) == {k: None for k in keys}
    assert utils._spacings_for((5, 1.25, 0.7), keys) == {k: (5.0, 1.25, 0.7) for k in keys}
    assert utils._spacings_for(2.0, keys)["t2_004"] == (2.0, 2.0, 2.0)
    table = {"ct": (2.5, 0.8, 0.8), "ct_001": (3.0, 0.7, 0.7), "t2": [7.7, 1.4, 1.4], "t1in": (1.0, 1.0)}      # t1in: unused, unchecked
    assert utils._spacings_for(table, keys) == {"ct_000": (2.5, 0.8, 0.8), "ct_001": (3.0, 0.7, 0.7), "t2_004": (7.7, 1.4, 1.4)}
    with pytest.raises(KeyError, match="t1out_003"):
        utils._spacings_for(table, keys + ["t1out_003"])
    with pytest.raises(RuntimeError, match="length equal to input rank"):
        utils._spacings_for(table, ["t1in_002"])
    with pytest.raises(ValueError):
        utils._spacings_for({"ct": (1.0, 0.0, 1.0)}, ["ct_000"])
    with pytest.raises(RuntimeError, match="length equal to input rank"):
        utils._spacings_for((1.0, 1.0), keys)
    # through the matrix functions, before any upload
    v = np.zeros((2, 4, 4), np.uint8)
    for f in (utils.get_all_matrix, utils.get_hd_matrix):
        with pytest.raises(KeyError, match="t2_004") as e:
            f({"t2_004": v}, {"t2_004": v}, spacings={"ct": (1.0, 1.0, 1.0)})
        assert not isinstance(e.value, _hip.SmsutHipError)
        with pytest.raises(ValueError):
            f({"t2_004": v}, {"t2_004": v}, spacings=(1.0, -1.0, 1.0))


def test_config_spacing_is_off():
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    assert cfg.test_spacing is None


def test_fixture_is_small_and_self_consistent(fx):
    from conftest import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "spacing.npz")) < 100 * 1024
    assert fx["spacings"].shape[1] == 3 and (fx["spacings"] > 0).all()
    stored = {k[2:] for k in fx.files if k.startswith("p_")}
    assert stored == {str(n) for n in fx["own"]}                   # only the designed volumes are stored
    for r in fx["runs"]:
        c, s = str(r).split()
        st, six, r2, hd, hd95 = (fx[f"{k}_{c}_s{s}"] for k in ("st", "hd6", "hd2r", "hd", "hd95"))
        assert st.shape == (4, 7) and six.shape == (4, 6) and r2.shape == (4, 4) and hd.shape == (4,) and hd95.shape == (4,)
        for l in range(4):
            if six[l, 0] == 0 or six[l, 1] == 0:
                assert (six[l, 2:] == -1).all() and (r2[l] == -1).all() and np.isnan(hd[l]) and np.isnan(hd95[l]), (c, l)
                continue
            assert six[l, 0] == st[l, 3] and six[l, 1] == st[l, 5]
            assert 0 <= six[l, 4] <= six[l, 5] <= max(six[l, 2], six[l, 3]) == hd[l] and six[l, 4] <= hd95[l] <= six[l, 5], (c, l)
            np.testing.assert_allclose(np.sqrt(r2[l]), six[l, 2:], rtol=1e-15, atol=0)      # scipy against the restated passes
            assert st[l, 4] <= six[l, 2] * st[l, 3] * (1 + 1e-12) and st[l, 6] <= six[l, 3] * st[l, 5] * (1 + 1e-12)


def test_designed_cases_are_what_they_claim(fx):
    sp = [tuple(v) for v in fx["spacings"]]
    assert sp[0] == (1.0, 1.0, 1.0) and sp[1] == (5.0, 1.25, 0.7) and sp[2] == (0.7, 1.25, 5.0) and sp[6] == (3.0, 0.9, 1.1)
    ax = [fx[f"hd6_axis_order_s{s}"][0, 2] for s in (0, 1, 2)]
    assert ax[0] == 2.0 and abs(ax[1] - 4.2) < 1e-14 and abs(ax[2] - 1.4) < 1e-14
    same = fx["hd2r_sel_same_s6"][0]
    assert fx["hd6_sel_same_s6"][0, :2].sum() == 42 and len(set(same.tolist())) == 1 and same[0] > 0
    nxt = fx["hd2r_sel_next_s6"][0]
    assert nxt[2] < nxt[3] and nxt[3] - nxt[2] < 1e-14 * nxt[2] and fx["hd6_sel_next_s6"][0, :2].tolist() == [1, 2]
    far = fx["hd2r_straddle_s6"][0]
    assert far[2] == 0.0 and far[3] > 1e4                          # the two ranks: a zero key and a large exponent
    assert fx["hd6_far_pair_s6"][0, :2].tolist() == [1, 1]
    assert (fx["hd2r_sel_zero_s6"][:2] == 0).all()
    assert fx["p_long_2x600"].shape == (2, 600) and fx["p_long_5x37x300"].shape == (5, 37, 300)
    for m in ("spm_assd", "spm_hd", "spm_hd95"):
        assert fx[m].shape == (5, 5) and np.isfinite(fx[m]).all()
    assert (fx["spm_hd95"] <= fx["spm_hd"]).all() and (fx["spm_assd"] <= fx["spm_hd"]).all()
    assert [str(k) for k in fx["spm_keys"]] == ["ct", "ct_001", "t1in", "t1out", "t2"] and fx["spm_vals"].shape == (5, 3)


def test_generator_reproduces_fixture(fx):
    pytest.importorskip("scipy")
    import importlib.util
    from conftest import GOLDEN
    spec = importlib.util.spec_from_file_location("make_spacing_golden", os.path.join(GOLDEN, "make_spacing_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    data = gen.build()
    assert sorted(data) == sorted(fx.files)
    for k, v in data.items():
        np.testing.assert_array_equal(np.asarray(v), fx[k], err_msg=k)
