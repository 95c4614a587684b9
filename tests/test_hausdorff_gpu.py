"""Hausdorff / HD95 on the MI355X (smsut_surface_hd of csrc/metrics.hip through ops.surface_hd and misc.utils' hd / hd95 / asd /
get_hd_matrix) against tests/golden/hausdorff.npz, scipy where installed, argument checks, and the `-p test` table.

The six numbers per label are integers and compared exactly; ``hd`` is the square root of an integer on both sides and compared
exactly; ``hd95`` is compared with numpy.percentile at rtol 1e-9 (the bar of tests/test_metrics_gpu.py for surface distances):
numpy forms its fractional index by another fp64 expression than (n - 1) * q, a few ulp of the index apart (about n * 2^-52,
below 1e-10 for any n here), and the interpolation error is that difference times the gap between the two neighbours."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL = 1e-9


@pytest.fixture(scope="module")
def fx(golden):
    return golden("hausdorff")


@pytest.fixture(scope="module")
def mx(golden):
    return golden("metrics")


@pytest.fixture(scope="module")
def vols(fx, mx):
    own = {str(n) for n in fx["own"]}
    return {str(n): ((fx if str(n) in own else mx)[f"p_{n}"], (fx if str(n) in own else mx)[f"g_{n}"]) for n in fx["names"]}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def load_generator():
    from conftest import GOLDEN
    spec = importlib.util.spec_from_file_location("make_hausdorff_golden", os.path.join(GOLDEN, "make_hausdorff_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def check_case(name, p, g, six, hd, hd95):
    """ops.surface_hd on the whole volume, then utils.hd / utils.hd95 on every label both masks hold."""
    from smsut_amd import ops
    from smsut_amd.misc import utils
    got = ops.surface_hd(dev(p), dev(g), 4)
    assert got.dtype == np.float64
    np.testing.assert_array_equal(got, six, err_msg=name)
    for lab in range(1, 5):
        if six[lab - 1, 2] < 0:
            continue
        assert utils.hd(p == lab, g == lab) == hd[lab - 1], (name, lab)
        np.testing.assert_allclose(utils.hd95(p == lab, g == lab), hd95[lab - 1], rtol=RTOL, atol=0, err_msg=f"{name} {lab}")


def test_surface_hd_hd_and_hd95_match_fixture(fx, vols):
    from smsut_amd.misc import utils
    for n, (p, g) in vols.items():
        check_case(n, p, g, fx[f"hd6_{n}"], fx[f"hd_{n}"], fx[f"hd95_{n}"])
    p, g = vols["pair3"]
    assert utils.hd(p, g) == 3.0 and utils.hd95(p, g) == 3.0
    assert utils.hd(p[0], g[0]) == 3.0 and utils.hd95(p[0], g[0]) == 3.0          # 2-D masks
    p, g = vols["far_pair"]
    assert utils.hd(p, g) == np.sqrt(25601.0) and utils.hd95(p, g) == np.sqrt(25601.0)
    p, g = vols["nested"]
    assert utils.hd(p, g) == np.sqrt(50.0) and utils.hd(g, p) == np.sqrt(50.0)   # the larger directed maximum, either way round
    p, g = vols["straddle"]
    np.testing.assert_allclose(utils.hd95(p, g), 0.9 * np.sqrt(16389.0), rtol=RTOL, atol=0)


def test_counts_are_those_of_surface_stats(vols):
    from smsut_amd import ops
    for n in ("blobs_a", "odd_5x37x53", "one_sided", "nested"):
        p, g = vols[n]
        st, six = ops.surface_stats(dev(p), dev(g), 4), ops.surface_hd(dev(p), dev(g), 4)
        np.testing.assert_array_equal(six[:, 0], st[:, 3], err_msg=n)
        np.testing.assert_array_equal(six[:, 1], st[:, 5], err_msg=n)


def test_other_quantiles(vols):
    """q = 100 selects the maximum for both ranks; q = 50 on the pool {0, 0, 16389} selects its middle 0 and the top."""
    from smsut_amd import ops
    p, g = vols["blobs_b"]
    six = ops.surface_hd(dev(p), dev(g), 4, q=100.0)
    np.testing.assert_array_equal(six[:, 4], np.maximum(six[:, 2], six[:, 3]))
    np.testing.assert_array_equal(six[:, 5], six[:, 4])
    p, g = vols["straddle"]
    assert ops.surface_hd(dev(p), dev(g), 1, q=50.0)[0].tolist() == [1, 2, 0, 16389, 0, 16389]
    assert ops.surface_hd(dev(p), dev(g), 1, q=49.0)[0].tolist() == [1, 2, 0, 16389, 0, 0]


def test_asd_matches_surface_stats_fixture(mx):
    from smsut_amd.misc import utils
    st = mx["st_blobs_a"]
    p, g = mx["p_blobs_a"], mx["g_blobs_a"]
    for lab in range(1, 5):
        np.testing.assert_allclose(utils.asd(p == lab, g == lab), st[lab - 1, 4] / st[lab - 1, 3], rtol=RTOL, atol=0)
        np.testing.assert_allclose(utils.asd(g == lab, p == lab), st[lab - 1, 6] / st[lab - 1, 5], rtol=RTOL, atol=0)
    assert utils.asd(mx["p_pair3"], mx["g_pair3"]) == 3.0


def test_get_hd_matrix_matches_fixture(fx, mx):
    from smsut_amd.misc import utils
    keys = [str(k) for k in mx["gam_keys"]]
    prd = {k: mx[f"gam_p_{k}"].astype(np.int64) for k in keys}
    gt = {k: mx[f"gam_g_{k}"].astype(np.int64) for k in keys}
    hd, hd95 = utils.get_hd_matrix(prd, gt)
    np.testing.assert_allclose(hd, fx["hdm_hd"], rtol=RTOL, atol=0)
    np.testing.assert_allclose(hd95, fx["hdm_hd95"], rtol=RTOL, atol=0)


def test_empty_masks(vols, mx):
    from smsut_amd import ops
    from smsut_amd.misc import utils
    p, g = vols["one_sided"]
    got = ops.surface_hd(dev(p), dev(g), 4)
    assert got[1].tolist() == [9, 0, -1, -1, -1, -1] and got[2].tolist() == [0, 9, -1, -1, -1, -1]
    assert got[3].tolist() == [0, 0, -1, -1, -1, -1]
    for f in (utils.hd, utils.hd95, utils.asd):                 # medpy's two messages
        with pytest.raises(RuntimeError, match="The second supplied array does not contain any binary object"):
            f(p == 2, g == 2)                                     # label 2: empty reference
        with pytest.raises(RuntimeError, match="The first supplied array does not contain any binary object"):
            f(p == 3, g == 3)                                     # label 3: empty result
        with pytest.raises(RuntimeError, match="The first supplied array"):
            f(p == 4, g == 4)                                     # both empty: medpy checks the result first
    g = mx["gam_g_ct_000"].copy()
    g[g == 2] = 0                                                 # prediction holds organ 2, the ground truth does not
    with pytest.raises(RuntimeError, match="The second supplied array does not contain any binary object"):
        utils.get_hd_matrix({"ct_000": mx["gam_p_ct_000"]}, {"ct_000": g})


def test_bitwise_reproducible_and_surface_stats_undisturbed(vols):
    from smsut_amd import ops
    p, g = (dev(v) for v in vols["blobs_b"])
    st0 = ops.surface_stats(p, g, 4)
    a = ops.surface_hd(p, g, 4)
    b = ops.surface_hd(p, g, 4)
    assert a.tobytes() == b.tobytes()
    st1 = ops.surface_stats(p, g, 4)
    assert st0.tobytes() == st1.tobytes()


def test_invalid_arguments_return_minus_one_and_raise():
    from smsut_amd import _hip as H, ops
    lib = H.load()
    a = dev(np.zeros((2, 8, 8)))
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, 6, dtype=torch.float64, device="cuda")
    s = H.stream_ptr()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for args in ((1, 8, 4097, 4, 0), (2, 8, 8, 4, 1), (2, 8, 8, 256, 0), (2, 8, 8, 0, 0), (0, 8, 8, 4, 0), (2, 8, 8, 4, 2),
                 (4097, 8, 8, 2, 0), (2048, 1024, 1024, 4, 0)):
        assert lib.smsut_surface_ws(*args) == -1 and lib.smsut_surface_hd_ws(*args) == -1, args
    need = lib.smsut_surface_hd_ws(2, 8, 8, 2, 0)
    assert 0 < need <= ws.numel() and need >= lib.smsut_surface_ws(2, 8, 8, 2, 0) + 8 * 2 * 8 * 8
    assert lib.smsut_surface_hd_ws(1, 8, 8, 4, 1) > 0
    for q in (0.0, 1.5, float("nan"), -0.5):
        assert lib.smsut_surface_hd(p(a), p(a), p(out), p(ws), 2, 8, 8, 2, 0, q, s) == -1, q
    assert lib.smsut_surface_hd(p(a), p(a), p(out), p(ws), 2, 8, 8, 0, 0, 0.95, s) == -1
    assert lib.smsut_surface_hd(p(a), p(a), p(out), p(ws), 4097, 8, 8, 2, 0, 0.95, s) == -1
    assert lib.smsut_surface_hd(p(a), p(a), p(out), None, 2, 8, 8, 2, 0, 0.95, s) == -1
    with pytest.raises(H.SmsutHipError):
        ops.surface_hd(a, a, 256)
    with pytest.raises(H.SmsutHipError):
        ops.surface_hd(a, a, 4, q=0.0)
    with pytest.raises(ValueError):
        ops.surface_hd(a, a[:1], 4)
    with pytest.raises(ValueError):
        ops.surface_hd(a.float(), a.float(), 4)
    torch.cuda.synchronize()                                     # and the device is fine afterwards
    assert lib.smsut_surface_hd(p(a), p(a), p(out), p(ws), 2, 8, 8, 2, 0, 1.0, s) == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [[0, 0, -1, -1, -1, -1]] * 2


def test_scipy_cross_check_random_volumes():
    pytest.importorskip("scipy")
    gen = load_generator()
    rng = np.random.default_rng(7)
    cases = [(gen.mg.blobs(s, shp), gen.mg.blobs(s + 50, shp)) for s, shp in ((2, (7, 129, 77)), (3, (1, 512, 512)))]
    noise = rng.integers(0, 6, size=(6, 64, 96)).astype(np.uint8)     # every label everywhere: nearly all distances 0 or 1
    cases.append((noise, rng.integers(0, 5, size=noise.shape).astype(np.uint8)))
    for k, (p, g) in enumerate(cases):
        check_case(f"random {k}", p, g, *gen.hd_case(p, g))


def test_cli_test_phase_writes_the_hausdorff_table_when_switched_on(tmp_path, monkeypatch):
    """``-p train``, then ``-p test`` with the switch off and on (unetTrainer): off writes no all_hd_matrix.csv; on writes the
    Hausdorff rows, an empty line and the HD95 rows ('%.4f', ',') of get_hd_matrix of validate_epoch's predictions, and
    all_trois_matrix.csv is the same bytes both times."""
    from smsut_amd import config as cfg
    from smsut_amd.misc import utils
    from smsut_amd.trainer import baseTrainer, unetTrainer as T
    seen, calls = [], []

    def spy_hd(prd, gt):
        seen.append(({k: v.copy() for k, v in prd.items()}, {k: v.copy() for k, v in gt.items()}))
        return utils.get_hd_matrix(prd, gt)

    def spy_all(prd, gt):
        calls.append(1)
        return utils.get_all_matrix(prd, gt)

    monkeypatch.setattr(baseTrainer, "get_hd_matrix", spy_hd)
    monkeypatch.setattr(baseTrainer, "get_all_matrix", spy_all)
    for name, val in (("input_size", 64), ("batch_size", 4), ("num_iter_per_epoch", 4), ("max_epoch", 2), ("expr_root", str(tmp_path))):
        monkeypatch.setattr(cfg, name, val)
    assert cfg.test_hausdorff is False
    T.main(["-p", "train", "-nm", "u"])
    root = os.path.join(str(tmp_path), "u", "000")
    T.main(["-p", "test", "-nm", "u", "-i", "000", "-wh", "best"])
    assert not os.path.exists(os.path.join(root, "all_hd_matrix.csv")) and not seen and len(calls) == 1
    trois = open(os.path.join(root, "all_trois_matrix.csv"), "rb").read()
    monkeypatch.setattr(cfg, "test_hausdorff", True)
    T.main(["-p", "test", "-nm", "u", "-i", "000", "-wh", "best"])
    assert open(os.path.join(root, "all_trois_matrix.csv"), "rb").read() == trois
    assert len(seen) == 1 and len(calls) == 2
    lines = open(os.path.join(root, "all_hd_matrix.csv")).read().split("\n")
    assert len(lines) == 12 and lines[5] == "" and lines[11] == ""
    rows = [ln.split(",") for ln in lines[:5] + lines[6:11]]
    assert all(len(r) == cfg.n_label + 1 and all(len(v.split(".")[1]) == 4 for v in r) for r in rows)
    hd, hd95 = utils.get_hd_matrix(*seen[0])
    assert utils.matrix_text(hd) == "\n".join(lines[:5]) + "\n"
    assert utils.matrix_text(hd95) == "\n".join(lines[6:11]) + "\n"
    assert (hd95 <= hd).all()
