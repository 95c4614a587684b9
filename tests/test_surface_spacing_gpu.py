"""Anisotropic voxel spacing of the surface metrics on the MI355X (smsut_surface_stats_sp / smsut_surface_hd_sp of
csrc/metrics.hip through ops.surface_stats / ops.surface_hd ``spacing=`` and misc.utils' ``voxelspacing=`` / ``spacings=``)
against tests/golden/spacing.npz.

Bars (derived, tests/golden/make_spacing_golden.py asserts their ground): scipy and the device reach a distance through at most
four fp64 roundings and a square root each, about 8 * 2^-53 = 9e-16 relative apart at worst, so single distances (hd, hd95, the
order statistics, the directed maxima) are held to rtol 1e-14; sums, ASD and ASSD to 1e-13 (the summation order adds a few
ulp * log n); counts are exact.  The squared distances themselves are also compared bit for bit with the generator's NumPy
restatement of the kernels' expression (``hd2r``): rounding is monotone, so the separable minimum is the minimum of that
expression over the other border, and the select must return exactly one of those values."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL_D = 1e-14
RTOL_SUM = 1e-13


@pytest.fixture(scope="module")
def fx(golden):
    return golden("spacing")


@pytest.fixture(scope="module")
def mx(golden):
    return golden("metrics")


@pytest.fixture(scope="module")
def hx(golden):
    return golden("hausdorff")


@pytest.fixture(scope="module")
def vols(fx, mx, hx):
    """name -> (p, g) of every case the fixture runs, and of hausdorff.npz's designed ones."""
    own, hown = {str(n) for n in fx["own"]}, {str(n) for n in hx["own"]}
    names = {str(r).split()[0] for r in fx["runs"]} | hown
    src = lambda n: fx if n in own else (hx if n in hown else mx)
    return {n: (src(n)[f"p_{n}"], src(n)[f"g_{n}"]) for n in names}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def runs_of(fx, names):
    out = []
    for r in fx["runs"]:
        c, s = str(r).split()
        if c in names:
            out.append((c, int(s)))
    return out


def spacing_of(fx, s, ndim):
    return tuple(float(v) for v in fx["spacings"][s][3 - ndim:])


def check_run(fx, vols, c, s):
    """ops.surface_stats / ops.surface_hd on the whole volume against the fixture's rows; then the four metric functions on every
    label both masks hold."""
    from smsut_amd import ops
    from smsut_amd.misc import utils
    p, g = vols[c]
    sp = spacing_of(fx, s, p.ndim)
    tag = f"{c} {sp}"
    st, six, r2 = fx[f"st_{c}_s{s}"], fx[f"hd6_{c}_s{s}"], fx[f"hd2r_{c}_s{s}"]
    got = ops.surface_stats(dev(p), dev(g), 4, spacing=sp)
    assert got.dtype == np.float64 and got.shape == (4, 7)
    np.testing.assert_array_equal(got[:, [0, 1, 2, 3, 5]], st[:, [0, 1, 2, 3, 5]], err_msg=tag)
    for col in (4, 6):
        ok = ~np.isnan(st[:, col])
        np.testing.assert_allclose(got[ok, col], st[ok, col], rtol=RTOL_SUM, atol=0, err_msg=tag)
    got = ops.surface_hd(dev(p), dev(g), 4, spacing=sp)
    assert got.dtype == np.float64 and got.shape == (4, 6)
    np.testing.assert_array_equal(got[:, :2], six[:, :2], err_msg=tag)
    has = six[:, 2] >= 0
    np.testing.assert_array_equal(got[~has, 2:], -1.0, err_msg=tag)
    np.testing.assert_allclose(np.sqrt(got[has, 2:]), six[has, 2:], rtol=RTOL_D, atol=0, err_msg=tag)
    np.testing.assert_array_equal(got[:, 2:], r2, err_msg=tag + " (exact select)")
    for lab in np.flatnonzero(has) + 1:
        P, G = p == lab, g == lab
        row = st[lab - 1]
        np.testing.assert_allclose(utils.hd(P, G, voxelspacing=sp), fx[f"hd_{c}_s{s}"][lab - 1], rtol=RTOL_D, atol=0, err_msg=tag)
        np.testing.assert_allclose(utils.hd95(P, G, voxelspacing=sp), fx[f"hd95_{c}_s{s}"][lab - 1], rtol=RTOL_D, atol=0, err_msg=tag)
        np.testing.assert_allclose(utils.asd(P, G, voxelspacing=sp), row[4] / row[3], rtol=RTOL_SUM, atol=0, err_msg=tag)
        np.testing.assert_allclose(utils.asd(G, P, voxelspacing=sp), row[6] / row[5], rtol=RTOL_SUM, atol=0, err_msg=tag)
        np.testing.assert_allclose(utils.assd(P, G, voxelspacing=sp), 0.5 * (row[4] / row[3] + row[6] / row[5]), rtol=RTOL_SUM,
                                   atol=0, err_msg=tag)


def test_axis_order(fx, vols):
    """P = {(0,0,0)}, G = {(2,0,0), (0,0,6)}: the nearer one is decided by the weights of z and x."""
    from smsut_amd import ops
    from smsut_amd.misc import utils
    p, g = vols["axis_order"]
    assert p.shape == (3, 2, 8) and np.argwhere(p).tolist() == [[0, 0, 0]] and np.argwhere(g).tolist() == [[0, 0, 6], [2, 0, 0]]
    for sp, want in (((1.0, 1.0, 1.0), 2.0), ((5.0, 1.25, 0.7), 4.2), ((0.7, 1.25, 5.0), 1.4)):
        six = ops.surface_hd(dev(p), dev(g), 1, spacing=sp)[0]
        np.testing.assert_allclose(np.sqrt(six[2]), want, rtol=RTOL_D, atol=0)
        np.testing.assert_allclose(utils.asd(p, g, voxelspacing=sp), want, rtol=RTOL_D, atol=0)
        st = ops.surface_stats(dev(p), dev(g), 1, spacing=sp)[0]
        np.testing.assert_allclose(st[4], want, rtol=RTOL_D, atol=0)
    assert ops.surface_hd(dev(p), dev(g), 1)[0][2] == 4.0                      # and without a spacing: voxels
    for c, s in runs_of(fx, {"axis_order"}):
        check_run(fx, vols, c, s)


def test_unit_spacing_is_the_integer_path_bit_for_bit(vols, hx):
    from smsut_amd import ops
    names = ["blobs_a", "odd_5x37x53"] + [str(n) for n in hx["own"] if str(n) != "long_line"]
    planar = 0
    for n in names:
        p, g = (dev(v) for v in vols[n])
        one = (1.0,) * p.dim()
        planar += p.dim() == 2
        assert np.array_equal(ops.surface_stats(p, g, 4, spacing=one), ops.surface_stats(p, g, 4)), n
        assert np.array_equal(ops.surface_hd(p, g, 4, spacing=one), ops.surface_hd(p, g, 4)), n
    assert planar >= 3
    p, g = (dev(v) for v in vols["blobs_a"])
    for q in (50.0, 100.0, 1.0):
        assert np.array_equal(ops.surface_hd(p, g, 4, q=q, spacing=(1.0, 1.0, 1.0)), ops.surface_hd(p, g, 4, q=q)), q


def test_power_of_two_scaling_is_exact(vols):
    from smsut_amd import ops
    for n in ("blobs_a", "nested", "slant"):
        p, g = (dev(v) for v in vols[n])
        n_cls = 4 if n == "blobs_a" else 1                                      # labels that both masks hold
        nd = p.dim()
        st1, hd1 = ops.surface_stats(p, g, n_cls, spacing=(1.0,) * nd), ops.surface_hd(p, g, n_cls, spacing=(1.0,) * nd)
        assert (hd1[:, 2:] >= 0).all()
        for f in (2.0, 0.25):
            st, hd = ops.surface_stats(p, g, n_cls, spacing=(f,) * nd), ops.surface_hd(p, g, n_cls, spacing=(f,) * nd)
            assert np.array_equal(st[:, [0, 1, 2, 3, 5]], st1[:, [0, 1, 2, 3, 5]]) and np.array_equal(hd[:, :2], hd1[:, :2])
            assert np.array_equal(st[:, [4, 6]], f * st1[:, [4, 6]]), (n, f)
            assert np.array_equal(np.sqrt(hd[:, 2:]), f * np.sqrt(hd1[:, 2:])), (n, f)
    # an anisotropic spacing scaled as a whole: every squared distance scales by exactly 16
    p, g = (dev(v) for v in vols["blobs_a"])
    a = ops.surface_hd(p, g, 4, spacing=(5.0, 1.25, 0.7))
    b = ops.surface_hd(p, g, 4, spacing=(20.0, 5.0, 2.8))
    assert np.array_equal(b[:, 2:], 16.0 * a[:, 2:])


@pytest.mark.parametrize("case", ["blobs_a", "blobs_b", "odd_5x37x53", "z_column", "empty", "one_sided"])
def test_parity_with_fixture(fx, vols, case):
    runs = runs_of(fx, {case})
    assert sorted(s for _, s in runs) == [1, 3, 4, 5]
    assert [tuple(fx["spacings"][s]) for s in (1, 3, 4, 5)] == [(5.0, 1.25, 0.7), (2.5, 0.78125, 0.78125), (1e-3, 3e-3, 7e-4),
                                                                (1234.5, 999.9, 1000.0)]
    for c, s in runs:
        check_run(fx, vols, c, s)


def test_cases_aimed_at_the_select(fx, vols):
    """sel_same: ranks lo and hi inside a run of 40 equal values; sel_next: lo is the last of its value and hi the next one up,
    apart in the last mantissa bits; straddle: 0 against a far voxel; far_pair: n = 1 per direction; sel_zero: every key 0."""
    from smsut_amd import ops
    runs = runs_of(fx, {"sel_same", "sel_next", "straddle", "far_pair", "sel_zero"})
    assert len(runs) == 5 and all(tuple(fx["spacings"][s]) == (3.0, 0.9, 1.1) for _, s in runs)
    for c, s in runs:
        check_run(fx, vols, c, s)
    p, g = (dev(v) for v in vols["sel_next"])
    six = ops.surface_hd(p, g, 1, spacing=(3.0, 0.9, 1.1))[0]
    assert six[4] < six[5] and six[5] - six[4] < 1e-14 * six[4]
    assert six[4] == np.float64(0.9) * np.float64(0.9) * 121.0 or six[4] == np.float64(1.1) * np.float64(1.1) * 81.0
    p, g = (dev(v) for v in vols["straddle"])
    six = ops.surface_hd(p, g, 1, q=50.0, spacing=(3.0, 0.9, 1.1))[0]        # pool {0, 0, far}: ranks 1 and 2
    assert six[4] == 0.0 and six[5] == six[3] > 1e4
    six = ops.surface_hd(p, g, 1, q=100.0, spacing=(3.0, 0.9, 1.1))[0]
    assert six[4] == six[5] == six[3]


def test_long_lines_and_many_blocks(fx, vols):
    runs = runs_of(fx, {"long_2x600", "long_5x37x300"})
    assert len(runs) == 2 and vols["long_2x600"][0].shape == (2, 600) and vols["long_5x37x300"][0].shape == (5, 37, 300)
    for c, s in runs:
        assert tuple(fx["spacings"][s]) == (2.0, 0.5, 1.5)
        check_run(fx, vols, c, s)


def test_bitwise_reproducible(vols):
    from smsut_amd import ops
    p, g = (dev(v) for v in vols["blobs_a"])
    sp = (5.0, 1.25, 0.7)
    a, b = ops.surface_stats(p, g, 4, spacing=sp), ops.surface_stats(p, g, 4, spacing=sp)
    assert a.tobytes() == b.tobytes()
    a, b = ops.surface_hd(p, g, 4, spacing=sp), ops.surface_hd(p, g, 4, spacing=sp)
    assert a.tobytes() == b.tobytes()


def test_matrices(fx, mx, hx):
    from smsut_amd.misc import utils
    keys = [str(k) for k in mx["gam_keys"]]
    prd = {k: mx[f"gam_p_{k}"].astype(np.int64) for k in keys}
    gt = {k: mx[f"gam_g_{k}"].astype(np.int64) for k in keys}
    spacings = {str(k): tuple(v) for k, v in zip(fx["spm_keys"], fx["spm_vals"])}
    assert "ct" in spacings and "ct_001" in spacings and spacings["ct"] != spacings["ct_001"]
    dc, hd_placeholder, assd = utils.get_all_matrix(prd, gt, spacings=spacings)
    np.testing.assert_array_equal(dc, mx["gam_dc"])
    np.testing.assert_array_equal(hd_placeholder, mx["gam_hd"])
    np.testing.assert_allclose(assd, fx["spm_assd"], rtol=RTOL_SUM, atol=0)
    hd, hd95 = utils.get_hd_matrix(prd, gt, spacings=spacings)
    np.testing.assert_allclose(hd, fx["spm_hd"], rtol=RTOL_D, atol=0)
    np.testing.assert_allclose(hd95, fx["spm_hd95"], rtol=RTOL_D, atol=0)
    # None: the matrices of today, as the existing fixtures hold them
    none = utils.get_all_matrix(prd, gt, spacings=None)
    plain = utils.get_all_matrix(prd, gt)
    assert all(np.array_equal(a, b) for a, b in zip(none, plain))
    np.testing.assert_allclose(none[2], mx["gam_assd"], rtol=1e-9, atol=0)
    none = utils.get_hd_matrix(prd, gt, spacings=None)
    assert all(np.array_equal(a, b) for a, b in zip(none, utils.get_hd_matrix(prd, gt)))
    np.testing.assert_allclose(none[0], hx["hdm_hd"], rtol=1e-9, atol=0)
    # one spacing for all volumes, and unit spacing by that route
    one = utils.get_all_matrix(prd, gt, spacings=(1.0, 1.0, 1.0))
    assert all(np.array_equal(a, b) for a, b in zip(one, plain))
    lacking = {k: v for k, v in spacings.items() if k != "t2"}
    for f in (utils.get_all_matrix, utils.get_hd_matrix):
        with pytest.raises(KeyError, match="t2_004"):
            f(prd, gt, spacings=lacking)


def test_test_phase_uses_config_spacing(tmp_path, monkeypatch, capsys):
    """``BaseTrainer.test`` on the synthetic loader with ``cfg.test_spacing = (2.0, 1.0, 1.0)``: other ASSD rows than with None,
    the same Dice rows, the log names the spacing, and both matrix functions receive it.  The predictions are the labels moved by
    one slice and two rows (``validate_epoch`` is replaced: what the network says is not the subject here), so every organ is
    there and the distances have a z part."""
    import argparse
    from smsut_amd import config as cfg
    from smsut_amd.misc import utils
    from smsut_amd.trainer import baseTrainer, unetTrainer as T
    seen = []

    def spy_all(prd, gt, **kw):
        seen.append(("all", kw))
        return utils.get_all_matrix(prd, gt, **kw)

    def spy_hd(prd, gt, **kw):
        seen.append(("hd", kw))
        return utils.get_hd_matrix(prd, gt, **kw)

    def moved_labels(self, loader, gt, meter=None):
        return sum(len(v) for v in gt.values()), {k: np.roll(v, (1, 2), axis=(0, 1)) for k, v in gt.items()}

    monkeypatch.setattr(baseTrainer, "get_all_matrix", spy_all)
    monkeypatch.setattr(baseTrainer, "get_hd_matrix", spy_hd)
    monkeypatch.setattr(baseTrainer.BaseTrainer, "validate_epoch", moved_labels)
    for name, val in (("input_size", 64), ("batch_size", 4), ("num_iter_per_epoch", 40), ("expr_root", str(tmp_path)),
                      ("test_hausdorff", True)):
        monkeypatch.setattr(cfg, name, val)
    assert cfg.test_spacing is None
    T.seed_all()
    t = T.UnetTrainer("test", argparse.Namespace(fold=0, expr_name="u"))
    root = str(tmp_path / "out")
    text = {}
    for sp in (None, (2.0, 1.0, 1.0), None):
        monkeypatch.setattr(cfg, "test_spacing", sp)
        capsys.readouterr()
        t.test("inTurn", root)
        said = "voxel spacing (2.0, 1.0, 1.0)" in capsys.readouterr().out
        assert said == (sp is not None)
        files = [open(os.path.join(root, f)).read() for f in ("all_trois_matrix.csv", "all_hd_matrix.csv", "dice_matrix.csv")]
        if sp is None and None in text:
            assert files == text[None]                                         # None again: the same bytes
        text[sp] = files
    kw = {"spacings": (2.0, 1.0, 1.0)}
    assert seen == [("all", {}), ("hd", {}), ("all", kw), ("hd", kw), ("all", {}), ("hd", {})]
    plain, spaced = (text[sp][0].split("\n") for sp in (None, (2.0, 1.0, 1.0)))
    assert len(plain) == len(spaced) == 12
    assert spaced[:6] == plain[:6] and text[None][2] == text[(2.0, 1.0, 1.0)][2]   # the Dice rows, the empty line; dice_matrix.csv
    assert spaced[6:11] != plain[6:11]                                         # the ASSD rows
    a, b = (np.array([[float(v) for v in ln.split(",")] for ln in x[6:11]]) for x in (plain, spaced))
    assert (a[:4, :4] > 0).any(axis=1).sum() >= 2                              # at least two modalities were scored
    assert (b >= a - 2e-4).all() and (b <= 2.0 * a + 2e-4).all()               # every axis weighs at least 1 and at most 2
    assert text[None][1] != text[(2.0, 1.0, 1.0)][1]                           # Hausdorff / HD95 rows as well


def test_errors_leave_the_device_usable(vols):
    from smsut_amd import _hip as H, ops
    from smsut_amd.misc import utils
    p3, g3 = vols["z_column"]
    p2, g2 = vols["nested"]
    for f in (utils.assd, utils.asd, utils.hd, utils.hd95):
        with pytest.raises(RuntimeError, match="length equal to input rank"):
            f(p3 == 3, g3 == 3, voxelspacing=(1.0, 2.0))
        with pytest.raises(RuntimeError, match="length equal to input rank"):
            f(p2, g2, voxelspacing=(1.0, 2.0, 3.0))
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError):
                f(p3 == 3, g3 == 3, voxelspacing=(1.0, bad, 1.0))
            with pytest.raises(ValueError):
                f(p2, g2, voxelspacing=bad)
    a = dev(p3)
    for f in (ops.surface_stats, ops.surface_hd):
        with pytest.raises(RuntimeError, match="length equal to input rank"):
            f(a, a, 4, spacing=(1.0, 1.0))
        for bad in (0.0, -2.0, float("inf"), float("nan"), 1e-101, 1e101):
            with pytest.raises(ValueError):
                f(a, a, 4, spacing=(bad, 1.0, 1.0))
    # the C ABI itself: a bad spacing is the invalid-argument status, nothing is launched
    lib = H.load()
    d, h, w = p3.shape
    b = dev(g3)
    ws = torch.empty(max(lib.smsut_surface_sp_ws(d, h, w, 4, 0), lib.smsut_surface_hd_sp_ws(d, h, w, 4, 0)), dtype=torch.uint8,
                     device="cuda")
    out7 = torch.full((4, 7), 123.0, dtype=torch.float64, device="cuda")
    out6 = torch.full((4, 6), 123.0, dtype=torch.float64, device="cuda")
    s = H.stream_ptr()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for args in ((1, 8, 4097, 4, 0), (2, 8, 8, 4, 1), (2, 8, 8, 256, 0), (0, 8, 8, 4, 0)):
        assert lib.smsut_surface_sp_ws(*args) == -1 and lib.smsut_surface_hd_sp_ws(*args) == -1, args
    assert lib.smsut_surface_sp_ws(d, h, w, 4, 0) == lib.smsut_surface_ws(d, h, w, 4, 0) + 4 * d * h * w      # fp64 for int32
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-101, 1e101):
        for k in range(3):
            sp = [1.0, 1.0, 1.0]
            sp[k] = bad
            assert lib.smsut_surface_stats_sp(ptr(a), ptr(b), ptr(out7), ptr(ws), d, h, w, 4, 0, *sp, s) == -1, sp
            assert lib.smsut_surface_hd_sp(ptr(a), ptr(b), ptr(out6), ptr(ws), d, h, w, 4, 0, 0.95, *sp, s) == -1, sp
    assert lib.smsut_surface_hd_sp(ptr(a), ptr(b), ptr(out6), ptr(ws), d, h, w, 4, 0, 0.0, 1.0, 1.0, 1.0, s) == -1
    assert lib.smsut_surface_stats_sp(ptr(a), ptr(b), ptr(out7), None, d, h, w, 4, 0, 1.0, 1.0, 1.0, s) == -1
    torch.cuda.synchronize()
    assert (out7 == 123.0).all() and (out6 == 123.0).all()                     # nothing ran
    # planar: sz is ignored, whatever it holds
    a2, b2 = dev(p2), dev(g2)
    hh, ww = p2.shape
    assert lib.smsut_surface_hd_sp(ptr(a2), ptr(b2), ptr(out6), ptr(ws), 1, hh, ww, 4, 1, 0.95, float("nan"), 0.9, 1.1, s) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out6.cpu().numpy(), ops.surface_hd(a2, b2, 4, spacing=(0.9, 1.1)))
    # and the ends of the documented range work
    for sp in (1e-100, 1e100):
        six = ops.surface_hd(a, b, 4, spacing=(sp, sp, sp))
        one = ops.surface_hd(a, b, 4)
        np.testing.assert_allclose(np.sqrt(six[2, 2:]), sp * np.sqrt(one[2, 2:]), rtol=RTOL_D, atol=0)
