"""The translation report of the ugan test phase (``cfg.test_translation``; trainer/uganShp0Trainer.py ``translation_report``) on a
tiny ``UGANConsisTrainer`` and a hand-made test loader: registered volumes ``t1in_001`` / ``t1out_001`` (4 slices of 32 x 32 each)
and a ``ct_002`` volume without a partner.  The six tables must be the ones this file computes itself with tests/ssim_ref.py from
tensors it obtains by calling the trainer's network with the same vectors; with the flag off ``test`` writes what it always wrote."""
import os
import types

import numpy as np
import pytest
import torch

import ssim_ref as R
from oracle import recipe

pytestmark = pytest.mark.gpu

NS = types.SimpleNamespace(fold=0, expr_name=None, write_env=False, model_id=None)
CFG_NAMES = ("input_size", "batch_size", "n_label", "base_width", "expr_root", "validate_on_device", "test_hausdorff",
             "test_spacing", "test_translation", "test_translation_pairs")
SIZE, BS = 32, 4


@pytest.fixture()
def cfg_fix(tmp_path):
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    old = [getattr(cfg, k) for k in CFG_NAMES]
    cfg.expr_root = str(tmp_path)
    cfg.input_size, cfg.batch_size = SIZE, BS
    yield cfg
    for k, v in zip(CFG_NAMES, old):
        setattr(cfg, k, v)


def loader():
    img = recipe.synth_images((11, 1, SIZE, SIZE), 8100)
    t1in = img[0:4]
    t1out = (0.8 * t1in + 0.2 * img[4:8]).clamp(-1, 1)                        # the same anatomy, another contrast
    ct = img[8:11]                                                            # 3 slices: a short batch
    msk = recipe.synth_labels(4, SIZE, SIZE, 5, 8110, block=8)
    mk = lambda x, m, mid, pid: (x, msk[:x.shape[0]], torch.full((x.shape[0],), mid, dtype=torch.int64),
                                 [f"{m}_{pid}_{z}" for z in range(x.shape[0])])
    return [mk(t1in, "t1in", 1, "001"), mk(t1out, "t1out", 2, "001"), mk(ct, "ct", 0, "002")]


def new_trainer(cfg, batches):
    from smsut_amd.trainer.uganConsisTrainer import UGANConsisTrainer
    tr = UGANConsisTrainer("test", NS)
    tr.net.load_state_dict(recipe.fill(recipe.ugan_shapes(1, cfg.n_label + 1, cfg.n_modal, cfg.base_width), 31))
    tr.get_loaders = lambda loader_type: (None, None, batches)
    return tr


def own_tables(tr, cfg, batches):
    """{table: (ssim, psnr, mae)} and the SSIM bars, from the network's tensors through tests/ssim_ref.py."""
    nm = cfg.n_modal
    t = {k: [np.full((nm, nm), np.nan) for _ in range(3)] for k in ("cycle", "paired")}
    bars = {k: np.zeros((nm, nm)) for k in t}

    def cell(table, i, j, a, b):
        a, b = a.cpu().numpy()[:, 0], b.cpu().numpy()[:, 0]
        s64 = [R.ssim_mean(x, y) for x, y in zip(a, b)]
        s32 = [R.ssim_mean(x, y, np.float32) for x, y in zip(a, b)]
        se, ae = zip(*(R.se_ae(x, y) for x, y in zip(a, b)))
        t[table][0][i, j] = np.mean(s64)                                      # one volume per cell: the mean of its slices
        t[table][1][i, j] = R.psnr_of(sum(se), a.size)
        t[table][2][i, j] = sum(ae) / a.size
        bars[table][i, j] = np.mean([R.ssim_bar(x, y) for x, y in zip(s32, s64)])

    real, fwd_of = {}, {}
    tr.net.eval()
    with torch.no_grad():
        for img, _, mdl, names in batches:
            i = int(mdl[0])
            x = img.cuda()
            vec_org = tr.label2onehot(mdl, nm).to(tr.device)
            real[i] = tr.denorm(x)
            for j, vec in enumerate(tr.create_vectors(vec_org, nm)):
                _, fwd = tr.net(x, vec - vec_org, val_phase=True)
                _, back = tr.net(fwd, vec_org - vec, val_phase=True)
                cell("cycle", i, j, tr.denorm(x), tr.denorm(back))
                fwd_of[i, j] = tr.denorm(fwd)
    for i, j in ((1, 2), (2, 1)):
        cell("paired", i, j, fwd_of[i, j], real[j])
    return t, bars


def parse(text):
    blocks = [b for b in text.split("\n\n")]
    return [np.array([[float(v) for v in ln.split(",")] for ln in b.strip("\n").split("\n")]) for b in blocks]


def test_tables_and_file(cfg_fix, tmp_path):
    from smsut_amd.misc import utils
    cfg = cfg_fix
    cfg.test_translation = True
    batches = loader()
    tr = new_trainer(cfg, batches)
    got = {}
    report = tr.translation_report
    tr.translation_report = lambda ld, root: got.setdefault("tables", report(ld, root))
    root = str(tmp_path / "on")
    tr.test("inTurn", root)
    files = ("dice_matrix.csv", f"{tr.modality}_trois_matrix.csv", f"{tr.modality}_translation_matrix.csv")
    assert sorted(os.listdir(root)) == sorted(files)
    text = open(os.path.join(root, files[2])).read()
    tables = got["tables"]
    assert text == utils.translation_text(tables)
    want, bars = own_tables(tr, cfg, batches)
    written = parse(text)
    assert len(written) == 6 and all(m.shape == (cfg.n_modal, cfg.n_modal) for m in written)
    k = 0
    for table in ("cycle", "paired"):
        has = ~np.isnan(want[table][0])
        assert has.sum() == (3 * cfg.n_modal if table == "cycle" else 2)       # rows ct, t1in, t1out | (t1in, t1out) both ways
        for q, (g, w) in enumerate(zip(tables[table], want[table])):
            assert np.array_equal(np.isnan(g), ~has), (table, q)
            print(table, q, "max |got - want|", np.abs(g[has] - w[has]).max())
            if q == 0:
                assert (np.abs(g[has] - w[has]) <= bars[table][has]).all(), (table, g, w)
            elif q == 1:
                assert np.isfinite(w[has]).all() and (np.abs(g[has] - w[has]) <= 1e-9 * np.abs(w[has])).all(), (table, g, w)
            else:
                assert (np.abs(g[has] - w[has]) <= 1e-12 * np.abs(w[has])).all(), (table, g, w)
            # the file holds the same numbers at four decimals
            assert np.array_equal(np.isnan(written[k]), ~has)
            assert (np.abs(written[k][has] - g[has]) <= 0.5e-4 + 1e-12).all()
            k += 1
    # a translation is not the identity, and the cycle brings the image closer than the paired translation of a random net
    assert (tables["cycle"][2][has_rows(cfg)] > 0).all()


def has_rows(cfg):
    m = np.zeros((cfg.n_modal, cfg.n_modal), dtype=bool)
    m[:3] = True
    return m


def test_flag_off_writes_what_it_always_wrote(cfg_fix, tmp_path):
    cfg = cfg_fix
    batches = loader()
    out = {}
    for flag in (True, False):
        cfg.test_translation = flag
        tr = new_trainer(cfg, batches)                                         # a fresh trainer each time, the same weights
        root = str(tmp_path / ("on" if flag else "off"))
        mo = tr.test("inTurn", root)
        out[flag] = (mo, {f: open(os.path.join(root, f), "rb").read() for f in sorted(os.listdir(root))})
    same = ("dice_matrix.csv", f"{tr.modality}_trois_matrix.csv")
    assert sorted(out[False][1]) == sorted(same)                               # no translation file
    assert sorted(out[True][1]) == sorted(same + (f"{tr.modality}_translation_matrix.csv",))
    for f in same:
        assert out[True][1][f] == out[False][1][f] and len(out[False][1][f]) > 0, f
    assert np.array_equal(out[True][0], out[False][0])


def test_nothing_is_read_back_before_the_loader_is_exhausted(cfg_fix, tmp_path):
    """The meter keeps device rows only: while the loader runs no row leaves the device (``TranslationMeter.rows`` is the one
    copy, made by ``result``)."""
    from smsut_amd.misc import utils
    cfg = cfg_fix
    batches = loader()
    tr = new_trainer(cfg, batches)
    calls, seen = [], []

    class Spy(utils.TranslationMeter):
        def update(self, *a, **k):
            seen.append(len(calls))
            return super().update(*a, **k)

        def rows(self):
            calls.append(1)
            return super().rows()
    orig = utils.TranslationMeter
    utils.TranslationMeter = Spy
    try:
        tables = tr.translation_report(batches, str(tmp_path / "spy"))
    finally:
        utils.TranslationMeter = orig
    assert len(calls) == 1 and seen and set(seen) == {0}
    assert len(seen) == 3 * cfg.n_modal + 2                                    # one launch per (batch, j) and per paired direction
    assert not np.isnan(tables["paired"][0][1, 2]) and not np.isnan(tables["paired"][0][2, 1])
