"""Test-phase metrics on the MI355X (csrc/metrics.hip through ops.cc_filter / ops.surface_stats and misc.utils'
connected_components / assd / get_all_matrix) against tests/golden/metrics.npz, scipy where installed, stress shapes, argument
checks, and the `-p test` table the trainers write."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden):
    return golden("metrics")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def assert_stats(got, want):
    """counts exact; distance sums to 1e-9 relative where defined (the other mask non-empty)."""
    assert got.shape == want.shape
    cols = [0, 1, 2, 3, 5]
    np.testing.assert_array_equal(got[:, cols], want[:, cols])
    for c in (4, 6):
        ok = ~np.isnan(want[:, c])
        np.testing.assert_allclose(got[ok, c], want[ok, c], rtol=1e-9, atol=0)


def test_cleanup_matches_fixture_both_modes(fx):
    from smsut_amd import ops
    from smsut_amd.misc import utils
    for n in fx["names"]:
        p = fx[f"p_{n}"]
        np.testing.assert_array_equal(ops.cc_filter(dev(p), 4, False).cpu().numpy(), fx[f"cc3_{n}"], err_msg=n)
        np.testing.assert_array_equal(ops.cc_filter(dev(p), 4, True).cpu().numpy(), fx[f"ccs_{n}"], err_msg=n)
        np.testing.assert_array_equal(utils.connected_components(p.astype(np.int64)), fx[f"cc3_{n}"], err_msg=n)
    p = fx["p_d1"][0]                                            # 2-D input: 8-neighbour labelling of the image
    np.testing.assert_array_equal(utils.connected_components(p), fx["cc3_d1"][0])


def test_surface_stats_and_assd_match_fixture(fx):
    from smsut_amd import ops
    from smsut_amd.misc import utils
    for n in fx["names"]:
        got = ops.surface_stats(dev(fx[f"p_{n}"]), dev(fx[f"g_{n}"]), 4)
        assert_stats(got, fx[f"st_{n}"])
    assert utils.assd(fx["p_pair3"], fx["g_pair3"]) == 3.0
    assert utils.assd(fx["p_pair3"][0], fx["g_pair3"][0]) == 3.0          # 2-D masks
    st = fx["st_blobs_a"]
    for lab in range(1, 5):
        want = 0.5 * (st[lab - 1, 4] / st[lab - 1, 3] + st[lab - 1, 6] / st[lab - 1, 5])
        got = utils.assd(fx["p_blobs_a"] == lab, fx["g_blobs_a"] == lab)
        assert abs(got - want) <= 1e-9 * want


def test_get_all_matrix_matches_fixture(fx):
    from smsut_amd.misc import utils
    keys = [str(k) for k in fx["gam_keys"]]
    prd = {k: fx[f"gam_p_{k}"].astype(np.int64) for k in keys}
    gt = {k: fx[f"gam_g_{k}"].astype(np.int64) for k in keys}
    dc, hd, assd = utils.get_all_matrix(prd, gt)
    np.testing.assert_array_equal(dc, fx["gam_dc"])
    np.testing.assert_array_equal(hd, fx["gam_hd"])
    np.testing.assert_allclose(assd, fx["gam_assd"], rtol=1e-9, atol=0)


def test_empty_masks_raise(fx):
    from smsut_amd.misc import utils
    p = fx["p_pair3"]
    with pytest.raises(RuntimeError):
        utils.assd(np.zeros_like(p), p)
    with pytest.raises(RuntimeError):
        utils.assd(p, np.zeros_like(p))
    g = fx["gam_g_ct_000"].copy()
    g[g == 2] = 0                                                 # prediction holds organ 2, the ground truth does not
    with pytest.raises(RuntimeError):
        utils.get_all_matrix({"ct_000": fx["gam_p_ct_000"]}, {"ct_000": g})


def test_bitwise_reproducible(fx):
    from smsut_amd import ops
    p, g = dev(fx["p_blobs_b"]), dev(fx["g_blobs_b"])
    a = ops.surface_stats(p, g, 4)
    b = ops.surface_stats(p, g, 4)
    assert a.tobytes() == b.tobytes()
    assert torch.equal(ops.cc_filter(p, 4, False), ops.cc_filter(p, 4, False))


def snake(d, h, w):
    """One 1-voxel-wide path through every slice (rows y % 2 == 0, joined at alternating ends), stacked along z."""
    y, x = np.mgrid[0:h, 0:w]
    s = (y % 2 == 0) | ((y % 4 == 1) & (x == w - 1)) | ((y % 4 == 3) & (x == 0))
    return np.broadcast_to(s, (d, h, w)).astype(np.uint8)


def test_stress_long_chains_and_root_contention():
    from smsut_amd import ops
    v = snake(24, 256, 256)
    t = dev(v)
    for per_slice in (False, True):                              # one component (per slice: one per slice): nothing dropped
        assert torch.equal(ops.cc_filter(t, 4, per_slice), t)
    z, y, x = np.mgrid[0:24, 0:256, 0:256]
    lat = ((x + y + z) % 2 == 0).astype(np.uint8) * 3             # checkerboard: connected only through edges / diagonals
    t = dev(lat)
    for per_slice in (False, True):
        assert torch.equal(ops.cc_filter(t, 4, per_slice), t)


def test_invalid_arguments_return_minus_one_and_raise():
    from smsut_amd import _hip as H, ops
    from smsut_amd.misc import utils
    lib = H.load()
    a = dev(np.zeros((2, 8, 8)))
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, 7, dtype=torch.float64, device="cuda")
    s = H.stream_ptr()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.smsut_cc_ws(0, 8, 8, 4, 0) == -1 and lib.smsut_cc_ws(2, 8, 8, 0, 0) == -1
    assert lib.smsut_cc_ws(2, 8, 8, 256, 0) == -1 and lib.smsut_cc_ws(2, 8, 8, 4, 2) == -1
    assert lib.smsut_cc_ws(2048, 1024, 1024, 4, 0) == -1                                  # D*H*W >= 2^31
    assert lib.smsut_cc_filter(p(a), p(a), p(ws), 2048, 1024, 1024, 4, 0, s) == -1
    assert lib.smsut_cc_filter(p(a), p(a), p(ws), 2, -8, 8, 4, 0, s) == -1
    assert lib.smsut_cc_filter(p(a), p(a), p(ws), 2, 8, 8, 0, 0, s) == -1
    assert lib.smsut_surface_ws(1, 8, 4097, 4, 0) == -1 and lib.smsut_surface_ws(2, 8, 8, 4, 1) == -1
    assert lib.smsut_surface_ws(2, 8, 8, 256, 0) == -1 and lib.smsut_surface_ws(2, 8, 8, 4, 0) > 0
    assert lib.smsut_surface_stats(p(a), p(a), p(out), p(ws), 2, 8, 8, 0, 0, s) == -1
    assert lib.smsut_surface_stats(p(a), p(a), p(out), p(ws), 4097, 8, 8, 2, 0, s) == -1
    with pytest.raises(H.SmsutHipError):
        ops.cc_filter(a, 0, False)
    with pytest.raises(H.SmsutHipError):
        ops.surface_stats(a, a, 256)
    with pytest.raises(ValueError):
        utils.connected_components(np.full((2, 4, 4), 256))
    with pytest.raises(ValueError):
        utils.connected_components(np.full((2, 4, 4), -1))
    torch.cuda.synchronize()                                     # and the device is fine afterwards
    assert torch.equal(ops.cc_filter(a, 4, False), a)


def test_scipy_cross_check_random_volumes():
    pytest.importorskip("scipy")
    import importlib.util
    from conftest import GOLDEN
    from smsut_amd import ops
    from smsut_amd.misc import utils
    spec = importlib.util.spec_from_file_location("make_metrics_golden", os.path.join(GOLDEN, "make_metrics_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rng = np.random.default_rng(7)
    vols = [(gen.blobs(s, shp), gen.blobs(s + 50, shp)) for s, shp in ((1, (32, 256, 256)), (2, (7, 129, 77)), (3, (1, 512, 512)))]
    noise = rng.integers(0, 6, size=(6, 64, 96)).astype(np.uint8)
    vols.append((noise, rng.integers(0, 5, size=noise.shape).astype(np.uint8)))
    for p, g in vols:
        np.testing.assert_array_equal(utils.connected_components(p), gen.cc_ref(p))
        np.testing.assert_array_equal(ops.cc_filter(dev(p), 4, True).cpu().numpy(), gen.cc_slices_ref(p))
        assert_stats(ops.surface_stats(dev(p), dev(g), 4), gen.stats_ref(p, g))
    prd = {"ct_000": vols[0][0], "t2_001": vols[1][0]}
    gt = {"ct_000": vols[0][1], "t2_001": vols[1][1]}
    want = gen.get_all_matrix_ref(prd, gt)
    got = utils.get_all_matrix(prd, gt)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_allclose(got[2], want[2], rtol=1e-9, atol=0)


def test_cli_test_phase_writes_the_reference_table(tmp_path, monkeypatch):
    """``-p train`` then ``-p test`` (unetTrainer): all_trois_matrix.csv holds the Dice rows, an empty line and the ASSD rows
    ('%.4f', ','); its Dice block is dice_matrix.csv's and its ASSD block is get_all_matrix of validate_epoch's predictions."""
    import smsut_amd
    from smsut_amd import config as cfg
    from smsut_amd.misc import utils
    from smsut_amd.trainer import baseTrainer, unetTrainer as T
    seen = []

    def spy(prd, gt):
        seen.append(({k: v.copy() for k, v in prd.items()}, {k: v.copy() for k, v in gt.items()}))
        return utils.get_all_matrix(prd, gt)

    monkeypatch.setattr(baseTrainer, "get_all_matrix", spy)
    for name, val in (("input_size", 64), ("batch_size", 4), ("num_iter_per_epoch", 4), ("max_epoch", 2), ("expr_root", str(tmp_path))):
        monkeypatch.setattr(cfg, name, val)
    T.main(["-p", "train", "-nm", "u"])
    T.main(["-p", "test", "-nm", "u", "-i", "000", "-wh", "best"])
    root = os.path.join(str(tmp_path), "u", "000")
    text = open(os.path.join(root, "all_trois_matrix.csv")).read()
    lines = text.split("\n")
    assert len(lines) == 12 and lines[5] == "" and lines[11] == ""
    rows = [ln.split(",") for ln in lines[:5] + lines[6:11]]
    assert all(len(r) == cfg.n_label + 1 and all(len(v.split(".")[1]) == 4 for v in r) for r in rows)
    dice = np.array([[float(v) for v in r] for r in rows[:5]])
    mo = np.loadtxt(os.path.join(root, "dice_matrix.csv"), delimiter=",")
    assert np.abs(dice - mo).max() <= 5.1e-5                      # dice_matrix.csv holds 6 decimals
    assert len(seen) == 1
    _, _, assd = utils.get_all_matrix(*seen[0])
    assert [["%.4f" % v for v in r] for r in assd] == rows[5:]
