"""Host side of the translation metrics: the aggregation of per-slice {sum SSIM, SE, AE} rows into the modality tables
(misc/utils.py ``translation_tables``), the CSV text, and the argument checks of ``ops.image_similarity`` -- which raise before
any device call, so they run on a machine without a GPU."""
import math

import numpy as np
import pytest
import torch

H, W = 16, 20                      # 6 x 10 = 60 window centres, 320 pixels per slice
CENTRES, PIXELS = 60, 320


@pytest.fixture()
def utils():
    import smsut_amd  # noqa: F401
    from smsut_amd.misc import utils
    return utils


def hand_made():
    """Two modalities (ct = 0, t2 = 3); ct has two volumes of 3 and 1 slices, t2 one volume of 2 slices; cells (0, 3), (0, 0) and
    (3, 3) of the cycle table have data, (3, 0) is missing; one paired cell."""
    rows, names, cells = [], [], []

    def add(name, cell, ssim_mean, se, ae):
        rows.append([ssim_mean * CENTRES, se, ae]); names.append(name); cells.append(cell)
    # cell (0, 3): ct_001 (3 slices) and ct_002 (1 slice)
    add("ct_001_0", (0, 3, "cycle"), 0.90, 3.2, 16.0)
    add("ct_001_1", (0, 3, "cycle"), 0.80, 0.032, 1.6)
    add("ct_001_2", (0, 3, "cycle"), 0.70, 0.32, 3.2)
    add("ct_002_0", (0, 3, "cycle"), 0.50, 32.0, 64.0)
    # cell (0, 0): identical images
    add("ct_001_0", (0, 0, "cycle"), 1.0, 0.0, 0.0)
    add("ct_001_1", (0, 0, "cycle"), 1.0, 0.0, 0.0)
    # cell (3, 3)
    add("t2_007_0", (3, 3, "cycle"), 0.25, 0.64, 6.4)
    add("t2_007_1", (3, 3, "cycle"), 0.75, 0.64, 9.6)
    # paired (0, 3)
    add("ct_002_0", (0, 3, "paired"), 0.6, 3.2, 32.0)
    return np.array(rows), names, cells, [(H, W)] * len(rows)


def test_volume_then_modality_means(utils):
    rows, names, cells, shapes = hand_made()
    t = utils.translation_tables(rows, names, cells, shapes, data_range=1.0)
    assert sorted(t) == ["cycle", "paired"] and all(len(v) == 3 and all(m.shape == (4, 4) for m in v) for v in t.values())
    ssim, psnr, mae = t["cycle"]
    # SSIM: volume = mean of slices, cell = mean of volumes (NOT the mean of all four slices, 0.725)
    assert ssim[0, 3] == pytest.approx(0.5 * ((0.9 + 0.8 + 0.7) / 3 + 0.5), abs=1e-14)
    assert ssim[3, 3] == pytest.approx(0.5, abs=1e-14)
    # PSNR from the volume's MSE: ct_001 has MSE (3.2 + 0.032 + 0.32) / 960, ct_002 32 / 320
    p1 = 10 * math.log10(1.0 / ((3.2 + 0.032 + 0.32) / (3 * PIXELS)))
    p2 = 10 * math.log10(1.0 / (32.0 / PIXELS))
    assert psnr[0, 3] == pytest.approx(0.5 * (p1 + p2), rel=1e-14)
    slice_psnrs = [10 * math.log10(1.0 / (se / PIXELS)) for se in (3.2, 0.032, 0.32)]
    assert abs(sum(slice_psnrs) / 3 - p1) > 5.0                      # the two rules differ on these numbers: 30 dB vs 24.3 dB
    # MAE
    assert mae[0, 3] == pytest.approx(0.5 * ((16.0 + 1.6 + 3.2) / (3 * PIXELS) + 64.0 / PIXELS), rel=1e-14)
    assert mae[3, 3] == pytest.approx(16.0 / (2 * PIXELS), rel=1e-14)
    # identical images: SE = 0 -> inf, SSIM 1, MAE 0
    assert psnr[0, 0] == math.inf and ssim[0, 0] == 1.0 and mae[0, 0] == 0.0
    # cells without data stay NaN, in every table
    empty = np.ones((4, 4), dtype=bool)
    for c in ((0, 3), (0, 0), (3, 3)):
        empty[c] = False
    for m in (ssim, psnr, mae):
        assert np.isnan(m[empty]).all() and not np.isnan(m[~empty]).any()
    ps, pp, pm = t["paired"]
    assert ps[0, 3] == pytest.approx(0.6, abs=1e-14) and pp[0, 3] == pytest.approx(10 * math.log10(PIXELS / 3.2), rel=1e-14)
    assert pm[0, 3] == pytest.approx(0.1, rel=1e-14) and np.isnan(ps).sum() == 15


def test_data_range_enters_psnr_only(utils):
    rows, names, cells, shapes = hand_made()
    t1 = utils.translation_tables(rows, names, cells, shapes, data_range=1.0)
    t255 = utils.translation_tables(rows, names, cells, shapes, data_range=255.0)
    assert t255["cycle"][1][0, 3] == pytest.approx(t1["cycle"][1][0, 3] + 20 * math.log10(255.0), rel=1e-14)
    assert np.array_equal(t255["cycle"][0], t1["cycle"][0], equal_nan=True)
    assert np.array_equal(t255["cycle"][2], t1["cycle"][2], equal_nan=True)


def test_bad_aggregation_arguments(utils):
    rows, names, cells, shapes = hand_made()
    with pytest.raises(ValueError):
        utils.translation_tables(rows[:-1], names, cells, shapes)
    with pytest.raises(ValueError):
        utils.translation_tables(rows, names, [(0, 4, "cycle")] * len(names), shapes)
    with pytest.raises(ValueError):
        utils.translation_tables(rows, names, [(0, 0, "triangle")] * len(names), shapes)
    empty = utils.translation_tables(np.zeros((0, 3)), [], [], [])
    assert all(np.isnan(m).all() for v in empty.values() for m in v)


def test_csv_text(utils):
    rows, names, cells, shapes = hand_made()
    text = utils.translation_text(utils.translation_tables(rows, names, cells, shapes))
    blocks = text.split("\n\n")
    assert len(blocks) == 6 and text.endswith("\n") and not text.endswith("\n\n")
    for blk in blocks:
        lines = blk.strip("\n").split("\n")
        assert len(lines) == 4 and all(len(ln.split(",")) == 4 for ln in lines)
    cyc_ssim, cyc_psnr, cyc_mae, par_ssim, _, par_mae = ([ln.split(",") for ln in b.strip("\n").split("\n")] for b in blocks)
    assert cyc_ssim[0][3] == "0.6500" and cyc_ssim[0][0] == "1.0000" and cyc_ssim[3][0] == "nan" and cyc_ssim[3][3] == "0.5000"
    assert cyc_psnr[0][0] == "inf" and cyc_psnr[1][1] == "nan"
    assert cyc_psnr[0][3] == "%.4f" % (0.5 * (10 * math.log10(960 / 3.552) + 10.0))
    assert cyc_mae[0][0] == "0.0000" and cyc_mae[3][3] == "0.0250"
    assert par_ssim[0][3] == "0.6000" and par_mae[0][3] == "0.1000" and par_ssim[0][0] == "nan"


def test_meter_refuses_bad_cells_and_names_before_the_device(utils):
    m = utils.TranslationMeter()
    a = torch.zeros(2, 16, 16)
    with pytest.raises(ValueError):
        m.update(a, a, ["ct_001_0", "ct_001_1"], 0, 4, "cycle")
    with pytest.raises(ValueError):
        m.update(a, a, ["ct_001_0", "ct_001_1"], 0, 0, "round")
    with pytest.raises(ValueError):
        m.update(a, a, ["ct_001_0"], 0, 0, "cycle")
    with pytest.raises(ValueError):
        m.update(a, a, ["ct_001_0", "ct001"], 0, 0, "cycle")
    assert m.rows().shape == (0, 3) and all(np.isnan(t).all() for v in m.result().values() for t in v)


def test_pairs_with_an_unknown_modality_are_skipped(monkeypatch):
    """The pair resolution of ``translation_report`` is host code over ``cfg.Modality``: an unknown name drops the pair."""
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    from smsut_amd.trainer.uganShp0Trainer import UGANShp0Trainer
    monkeypatch.setattr(cfg, "test_translation_pairs", (("t1in", "t1out"), ("ct", "pet"), ("mr", "t2")))
    assert UGANShp0Trainer.translation_partners() == {1: [2], 2: [1]}
    monkeypatch.setattr(cfg, "test_translation_pairs", ())
    assert UGANShp0Trainer.translation_partners() == {}


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf")])
def test_image_similarity_refuses_a_bad_data_range(bad):
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    a = torch.zeros(1, 16, 16)
    with pytest.raises(ValueError):
        ops.image_similarity(a, a, bad)


def test_image_similarity_refuses_shapes_and_dtypes():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    f = torch.zeros(2, 16, 16)
    for a, b in ((f, torch.zeros(2, 16, 17)), (f, torch.zeros(3, 16, 16)), (f, torch.zeros(2, 1, 16, 16)),       # mismatched
                 (f.double(), f.double()), (f, f.half()), (f.long(), f.long()),                                  # not fp32
                 (torch.zeros(2, 2, 16, 16), torch.zeros(2, 2, 16, 16)), (torch.zeros(16, 16), torch.zeros(16, 16)),   # not [N,(1,)H,W]
                 (torch.zeros(1, 10, 16), torch.zeros(1, 10, 16)), (torch.zeros(0, 16, 16), torch.zeros(0, 16, 16)),
                 (f.numpy(), f.numpy())):
        with pytest.raises(ValueError):
            ops.image_similarity(a, b, 1.0)


def test_image_similarity_has_no_cpu_fallback():
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip, ops
    if torch.cuda.is_available():
        pytest.skip("CPU-only check")
    with pytest.raises(_hip.SmsutHipError):
        ops.image_similarity(torch.zeros(1, 16, 16), torch.zeros(1, 16, 16), 1.0)


def test_workspace_query_and_limits_on_the_host():
    import ctypes
    import __graft_entry__ as ge
    import ssim_ref as R
    ge.build()
    lib = ctypes.CDLL(ge.LIB)
    ws = lib.smsut_image_similarity_ws
    ws.restype = ctypes.c_int64
    tiles = lambda h, w: -(-(h - 10) // R.TH) * -(-(w - 10) // R.TW)
    for n, h, w in ((1, 11, 11), (3, 43, 42), (8, 256, 256), (2, R.TH + 11, R.TW + 11), (65535, 4096, 4096)):
        assert ws(n, h, w) == n * tiles(h, w) * 24, (n, h, w)
    for n, h, w in ((0, 16, 16), (65536, 16, 16), (1, 10, 16), (1, 16, 10), (1, 4097, 16), (1, 16, 4097), (-1, 16, 16)):
        assert ws(n, h, w) == -1, (n, h, w)
    # invalid arguments return SMSUT_EINVAL (-1) before anything is launched: null pointers are never touched
    f = lib.smsut_image_similarity
    f.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_double, ctypes.c_void_p]
    for n, h, w, dr in ((1, 10, 16, 1.0), (1, 16, 4097, 1.0), (0, 16, 16, 1.0), (1, 16, 16, 0.0), (1, 16, 16, float("nan")),
                        (1, 16, 16, float("inf")), (1, 16, 16, -1.0)):
        assert f(None, None, None, None, n, h, w, dr, None) == -1, (n, h, w, dr)
