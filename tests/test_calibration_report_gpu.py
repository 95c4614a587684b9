"""The calibration report of the test phase (``cfg.test_calibration``; trainer/baseTrainer.py ``calibration_report``) on a tiny
``UnetTrainer`` and a hand-made test loader -- ``ct_000`` (4 slices of 32 x 32) and ``t1in_001`` (3 slices: a short batch) -- and the
``temperature`` argument of ``predict.Predictor``.  The file must hold what a ``CalibrationMeter`` fed by hand with the network's
outputs gives, the host and the ``validate_on_device`` loops must write the same bytes, and with the flag off ``test`` writes what it
always wrote."""
import os
import types

import numpy as np
import pytest
import torch

import calibration_ref as R
import tta_ref
from oracle import recipe

pytestmark = pytest.mark.gpu

NS = types.SimpleNamespace(fold=0, expr_name=None, write_env=False, model_id=None)
CFG_NAMES = ("input_size", "batch_size", "n_label", "base_width", "expr_root", "validate_on_device", "test_hausdorff",
             "test_spacing", "test_calibration", "test_calibration_bins")
SIZE, BS = 32, 4


def loader():
    img = recipe.synth_images((7, 1, SIZE, SIZE), 9100)
    msk = recipe.synth_labels(7, SIZE, SIZE, 5, 9110, block=8)
    mk = lambda lo, hi, m, mid, pid: (img[lo:hi], msk[lo:hi], torch.full((hi - lo,), mid, dtype=torch.int64),
                                      [f"{m}_{pid}_{z}" for z in range(hi - lo)])
    return [mk(0, 4, "ct", 0, "000"), mk(4, 7, "t1in", 1, "001")]


def new_trainer(cfg, batches):
    from smsut_amd.trainer.unetTrainer import UnetTrainer
    tr = UnetTrainer("train", NS)
    tr.net.load_state_dict(recipe.fill(recipe.unet_shapes(1, cfg.n_label + 1, cfg.base_width), 7))
    tr.get_loaders = lambda loader_type: (None, None, batches)
    return tr


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """``{(flag, on_device): {file: bytes}}`` of three ``test`` runs, the trainer, the config and the batches."""
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    old = [getattr(cfg, k) for k in CFG_NAMES]
    root = tmp_path_factory.mktemp("calibration")
    cfg.expr_root = str(root)
    cfg.input_size, cfg.batch_size, cfg.test_hausdorff, cfg.test_spacing, cfg.test_calibration_bins = SIZE, BS, False, None, 15
    batches = loader()
    out = {}
    for flag, on_device in ((True, False), (True, True), (False, False)):
        cfg.test_calibration, cfg.validate_on_device = flag, on_device
        tr = new_trainer(cfg, batches)                             # a fresh trainer each time, the same weights
        where = str(root / f"{flag}_{on_device}")
        mo = tr.test("synthetic", where)
        out[flag, on_device] = (mo, {f: open(os.path.join(where, f), "rb").read() for f in sorted(os.listdir(where))})
    cfg.test_calibration, cfg.validate_on_device = False, False
    yield out, tr, cfg, batches
    for k, v in zip(CFG_NAMES, old):
        setattr(cfg, k, v)


def outputs(tr, cfg, batches):
    """The logits the validation loops see: a short batch padded with zero images to the batch size and cropped back."""
    res = []
    tr.net.eval()
    with torch.no_grad():
        for img, msk, mdl, _ in batches:
            b = img.shape[0]
            x = img.cuda()
            if b != cfg.batch_size:
                x = torch.cat([x, torch.zeros(cfg.batch_size - b, *x.shape[1:], device=x.device)], 0)
            res.append((tr._forward_eval(x)[:b], msk.cuda(), int(mdl[0])))
    return res


def parse(text):
    return [np.array([[float(v) for v in ln.split(",")] for ln in b.strip("\n").split("\n")]) for b in text.split("\n\n")]


def test_file_holds_what_a_meter_fed_by_hand_gives(runs):
    from smsut_amd.misc import utils
    out, tr, cfg, batches = runs
    name = f"{tr.modality}_calibration.csv"
    files = out[True, False][1]
    assert sorted(files) == sorted(("dice_matrix.csv", f"{tr.modality}_trois_matrix.csv", name, "temperature.txt"))
    fed = outputs(tr, cfg, batches)
    k = cfg.n_label + 1
    raw = utils.CalibrationMeter(k, 15, rows=cfg.n_modal)
    for o, m, row in fed:
        raw.update(o, m, row)
    t, its = utils.fit_temperature([(o, m) for o, m, _ in fed], k)
    fit = utils.CalibrationMeter(k, 15, temperature=t, rows=cfg.n_modal)
    for o, m, row in fed:
        fit.update(o, m, row)
    text = files[name].decode()
    assert text == utils.calibration_text(raw.reliability(), utils.calibration_rows(raw), utils.calibration_rows(fit))
    assert float(files["temperature.txt"].decode()) == t and 0 < its <= 30
    rel, rows_raw, rows_fit = parse(text)
    assert rel.shape == (15, 5) and rows_raw.shape == rows_fit.shape == (cfg.n_modal + 1, 5)
    assert rel[:, 2].sum() == 7 * SIZE * SIZE and np.allclose(rel[:, 1] - rel[:, 0], 1 / 15, atol=1e-6)
    assert np.isnan(rows_raw[2:cfg.n_modal]).all() and not np.isnan(rows_raw[[0, 1, cfg.n_modal]]).any()      # ct, t1in, overall
    # the written numbers are the fp64 reference's of the same logits
    z = np.concatenate([o.permute(0, 2, 3, 1).cpu().numpy() for o, _, _ in fed])
    y = np.concatenate([m.cpu().numpy() for _, m, _ in fed])
    for beta, rows in ((1.0, rows_raw), (R.beta_of(t), rows_fit)):
        want = utils.CalibrationTotals(R.stats(z, y, k, 15, beta)[0], k, 15)
        print("T", 1 / beta, "written", rows[-1], "fp64", want.summary())
        assert np.allclose(rows[-1, 2:4], want.summary()[2:4], rtol=1e-4, atol=2e-6)        # NLL, Brier (six decimals written)
    assert rows_fit[-1, 2] <= rows_raw[-1, 2] + 1e-6             # the fitted T minimises the NLL of these batches


def test_host_and_device_loops_write_the_same_bytes(runs):
    out = runs[0]
    assert sorted(out[True, True][1]) == sorted(out[True, False][1])
    for f, data in out[True, False][1].items():
        assert out[True, True][1][f] == data and len(data) > 0, f
    assert np.array_equal(out[True, True][0], out[True, False][0])


def test_flag_off_writes_what_it_always_wrote(runs):
    out, tr = runs[0], runs[1]
    same = ("dice_matrix.csv", f"{tr.modality}_trois_matrix.csv")
    assert sorted(out[False, False][1]) == sorted(same)           # the directory listing is what it was
    for f in same:
        assert out[False, False][1][f] == out[True, False][1][f] and len(out[False, False][1][f]) > 0, f
    assert np.array_equal(out[False, False][0], out[True, False][0])
    assert tr._calibration is None


def recording(f, seen):
    def g(x):
        o = f(x)
        seen.append(o)
        return o
    return g


def test_predictor_temperature(runs):
    from smsut_amd import ops
    from smsut_amd.predict import Predictor
    _, tr, cfg, _ = runs
    k, t = cfg.n_label + 1, 1.7
    beta = R.beta_of(t)
    f = tr._forward_eval
    img = torch.from_numpy(np.random.default_rng(12).integers(0, 256, (BS, SIZE, SIZE), dtype=np.uint8)).cuda()
    copies = ops.layout_copies()
    # one member: the argmax does not move with T, wherever the reference's two largest probabilities are further apart than the budget
    seen = []
    p1, c1 = Predictor(recording(f, seen), batch_size=BS, tta="none").predict_slices(img, confidence=True)
    pt, ct = Predictor(f, batch_size=BS, tta="none", temperature=t).predict_slices(img, confidence=True)
    z = seen[0].permute(0, 2, 3, 1).cpu().double()
    bp = R.b_p(k, beta)
    for scale in (1.0, beta):
        _, rconf, _, rgap = tta_ref.merge_ref([z * scale], [0])
        print("scale", scale, "smallest top-two gap of the reference", float(rgap.min()), "budget", bp)
        assert float(rgap.min()) > 4 * bp                         # no exception on the chosen input
        got = c1 if scale == 1.0 else ct
        assert float((got.cpu().double() - rconf).abs().max()) <= bp
    assert torch.equal(pt, p1) and not torch.equal(ct, c1)
    # several members: the confidence is tta_merge's on the pre-scaled logits, to the bit
    seen = []
    pf, cf = Predictor(recording(f, seen), batch_size=BS, tta="flips", temperature=t).predict_slices(img, confidence=True)
    tf = ops.tta_transforms("flips")
    assert len(seen) == len(tf)
    mp, mc, _ = ops.tta_merge([o * beta for o in seen], tf, classes=k, want_conf=True)
    assert torch.equal(pf, mp) and torch.equal(cf.view(torch.int32), mc.view(torch.int32))
    # None and 1 leave the path untouched
    p0, c0 = Predictor(f, batch_size=BS, tta="flips").predict_slices(img, confidence=True)
    for same in (None, 1, 1.0, [None]):
        pn, cn = Predictor(f, batch_size=BS, tta="flips", temperature=same).predict_slices(img, confidence=True)
        assert torch.equal(pn, p0) and torch.equal(cn.view(torch.int32), c0.view(torch.int32)), same
    assert not torch.equal(cf, c0)
    # one value per forward of an ensemble
    seen = []
    pe, ce = Predictor([recording(f, seen), f], batch_size=BS, tta="none", temperature=[None, t]).predict_slices(img, confidence=True)
    mp, mc, _ = ops.tta_merge([seen[0], seen[0] * beta], [0, 0], classes=k, want_conf=True)
    assert torch.equal(pe, mp) and torch.equal(ce.view(torch.int32), mc.view(torch.int32))
    assert ops.layout_copies() == copies
    for bad in ([1.0, 2.0], 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            Predictor(f, temperature=bad)
    for bad in (True, [True], "2", ["2"], object()):
        with pytest.raises(TypeError):
            Predictor(f, temperature=bad)
    assert Predictor(f, temperature=np.float32(t)).scales == Predictor(f, temperature=float(np.float32(t))).scales   # a NumPy scalar
