"""Validation on the device (``cfg.validate_on_device``; trainer/baseTrainer.py ``validate_epoch_device``, misc/utils.py
``DiceCounter``) against the host path it stands in for (``_collect_labels`` + ``validate_epoch`` + ``validate_dice``), trainer by
trainer.  Both paths run the same deterministic forward kernels on the same inputs (no float atomics in the forward), the
prediction is the same comparison chain, and the Dice matrix is the same fp64 arithmetic on equal integers: the bar is equality
-- of the Dice dict, of the meter's sums and counts, and of the bytes of the files ``test()`` writes -- not a tolerance."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import recipe

pytestmark = pytest.mark.gpu

NS = types.SimpleNamespace(fold=0, expr_name=None, write_env=False, model_id=None)
CFG_NAMES = ("input_size", "batch_size", "n_label", "base_width", "num_iter_per_epoch", "expr_root", "validate_on_device",
             "test_hausdorff", "test_spacing")


@pytest.fixture()
def cfg_fix(tmp_path):
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    old = [getattr(cfg, k) for k in CFG_NAMES]
    cfg.expr_root = str(tmp_path)
    yield cfg
    for k, v in zip(CFG_NAMES, old):
        setattr(cfg, k, v)


def new_meter(cfg):
    from smsut_amd.misc.utils import Meter
    return Meter([f"loss_{i}" for i in range(cfg.n_modal)] + ["loss"], [], alpha=1.0)


def both_paths(tr, cfg, batches, rewind=None):
    """(host, device) results of one validation over ``batches``: each ``(n_prd, Dice dict, meter, volume keys)``."""
    meter_h = new_meter(cfg)
    gt = tr._collect_labels(batches)
    n_h, prd = tr.validate_epoch(batches, gt, meter_h)
    host = (n_h, tr.validate_dice(prd, gt), meter_h, list(gt.keys()))
    if rewind is not None:
        rewind()
    meter_d = new_meter(cfg)
    n_d, counter = tr.validate_epoch_device(batches, meter_d)
    return host, (n_d, tr.validate_dice_device(counter), meter_d, counter.keys), (prd, gt, counter)


def assert_same(host, device):
    (n_h, dice_h, meter_h, keys_h), (n_d, dice_d, meter_d, keys_d) = host, device
    assert n_d == n_h and keys_d == keys_h
    assert list(dice_d) == list(dice_h) and all(dice_d[k] == dice_h[k] for k in dice_h), (dice_d, dice_h)
    assert meter_d.cur_values == meter_h.cur_values and meter_d.n == meter_h.n, (meter_d.cur_values, meter_h.cur_values)
    assert meter_h.n["loss"] > 0 and meter_h.cur_values["loss"] > 0.0


def assert_counts_are_the_volumes(prd, gt, counter, n_cls):
    """The device counts are the host volumes' overlap counts, and the prediction is not one class everywhere."""
    got = counter.counts[:len(counter.keys)].cpu().numpy()
    for s, k in enumerate(counter.keys):
        for c in range(n_cls):
            want = (np.count_nonzero((prd[k] == c) & (gt[k] == c)), np.count_nonzero(prd[k] == c), np.count_nonzero(gt[k] == c))
            assert tuple(got[s, c]) == want, (k, c, got[s, c], want)
    assert np.count_nonzero(got[:, :, 1].sum(0)) >= 2


def test_unet_trainer_ragged_synthetic_loader(cfg_fix):
    from smsut_amd.trainer.unetTrainer import UnetTrainer
    from smsut_amd.misc.synthetic import SyntheticSliceLoader
    cfg = cfg_fix
    cfg.input_size, cfg.batch_size = 64, 4
    tr = UnetTrainer("train", NS)
    tr.net.load_state_dict(recipe.fill(recipe.unet_shapes(1, cfg.n_label + 1, cfg.base_width), 7))
    test = SyntheticSliceLoader(3, size=64, n_batches=2, device="cuda")        # ragged: 3 < batch_size 4 -> padded
    state = test.state_dict()
    host, device, (prd, gt, counter) = both_paths(tr, cfg, test, rewind=lambda: test.load_state_dict(state))
    assert host[0] == 6 and host[2].n["loss"] == 8                             # the PADDED batch size is what the meter counts
    assert_same(host, device)
    assert_counts_are_the_volumes(prd, gt, counter, cfg.n_label + 1)


@pytest.mark.parametrize("name", ("dtc", "meanTeacher", "crossPse"))
def test_sibling_trainers_ragged_synthetic_loader(cfg_fix, name):
    """The labelled / unlabelled siblings through the shared evaluation loop; dtc's ``_forward_eval`` hands it one element of the
    network's tuple."""
    import importlib
    import dtc_ref
    from smsut_amd.misc.synthetic import SyntheticSliceLoader
    cfg = cfg_fix
    cfg.input_size, cfg.batch_size = 64, 4
    tr = getattr(importlib.import_module(f"smsut_amd.trainer.{name}Trainer"), f"{name}Trainer")("train", NS)
    shapes = (dtc_ref.shapes if name == "dtc" else recipe.unet_shapes)(1, cfg.n_label + 1, cfg.base_width)
    tr.net.load_state_dict(recipe.fill(shapes, 7))
    test = SyntheticSliceLoader(3, size=64, n_batches=2, device="cuda")        # ragged: 3 < batch_size 4 -> padded
    state = test.state_dict()
    host, device, (prd, gt, counter) = both_paths(tr, cfg, test, rewind=lambda: test.load_state_dict(state))
    assert host[0] == 6 and host[2].n["loss"] == 8                             # the PADDED batch size is what the meter counts
    assert_same(host, device)
    assert_counts_are_the_volumes(prd, gt, counter, cfg.n_label + 1)


def test_ugan_trainer_on_the_recipe_validation_batches(cfg_fix, golden):
    from smsut_amd.trainer.uganConsisTrainer import UGANConsisTrainer
    g = golden("validate")
    cfg = cfg_fix
    bs, size = int(g["bs"]), int(g["H"])
    cfg.input_size, cfg.batch_size = size, bs
    tr = UGANConsisTrainer("test", NS)
    tr.net.load_state_dict(recipe.fill(recipe.ugan_shapes(1, 5, 4, 16), int(g["g_seed"])))
    batches = recipe.validation_batches(bs, size)                              # ct_001: 5 slices, t2_007: 6; short last batches
    host, device, (prd, gt, counter) = both_paths(tr, cfg, batches)
    assert host[0] == 11 and counter.keys == ["ct_001", "t2_007"]              # order of first appearance
    assert_same(host, device)
    assert_counts_are_the_volumes(prd, gt, counter, 5)


def test_coranet_trainer_counts_head_zero(cfg_fix):
    import coranet_ref as R
    from smsut_amd.trainer.coraNetTrainer import coraNetTrainer
    cfg = cfg_fix
    cfg.input_size, cfg.batch_size, cfg.n_label, cfg.base_width = R.SIZE, R.BS, R.L, R.WIDTH
    tr = coraNetTrainer("train", NS)
    tr.net.load_state_dict(recipe.fill(R.shapes(), R.SEED_STUDENT))
    img, msk = R.val_inputs()
    modal = lambda m, n: torch.full((n,), m, dtype=torch.int64)
    batches = [(img, msk, modal(0, R.BS), [f"ct_002_{z}" for z in range(R.BS)]),
               (img[:1].flip(-1), msk[:1].flip(-1), modal(3, 1), ["t2_005_0"])]        # a short batch: padded to BS, cropped back
    host, device, (prd, gt, counter) = both_paths(tr, cfg, batches)
    assert host[0] == R.BS + 1 and counter.classes == R.L + 1 and tuple(counter.counts.shape[1:]) == (R.L + 1, 3)
    assert_same(host, device)
    assert_counts_are_the_volumes(prd, gt, counter, R.L + 1)


def test_test_phase_files_are_byte_identical(cfg_fix, tmp_path):
    from smsut_amd.trainer.unetTrainer import UnetTrainer
    cfg = cfg_fix
    cfg.input_size, cfg.batch_size, cfg.test_hausdorff, cfg.test_spacing = 64, 4, True, None
    tr = UnetTrainer("train", types.SimpleNamespace(fold=0, expr_name=None, write_env=False, model_id=None, iters_per_epoch=20))
    tr.net.load_state_dict(recipe.fill(recipe.unet_shapes(1, cfg.n_label + 1, cfg.base_width), 7))
    files = ("dice_matrix.csv", f"{tr.modality}_trois_matrix.csv", f"{tr.modality}_hd_matrix.csv")
    out = {}
    for flag in (False, True):
        cfg.validate_on_device = flag
        root = str(tmp_path / ("device" if flag else "host"))
        mo = tr.test("synthetic", root)                                        # two batches of 4 slices: volumes ct_000, t1in_001
        assert sorted(os.listdir(root)) == sorted(files)
        out[flag] = (mo, {f: open(os.path.join(root, f), "rb").read() for f in files})
    assert (out[True][0] == out[False][0]).all() and out[False][0].max() > 0.0
    for f in files:
        assert out[True][1][f] == out[False][1][f] and len(out[False][1][f]) > 0, f


def test_matrix_functions_take_device_volumes(cfg_fix):
    from smsut_amd.misc import utils
    rs = np.random.RandomState(4)
    blocky = lambda: np.repeat(np.repeat(rs.randint(0, 5, (6, 4, 4)), 8, 1), 8, 2).astype(np.int64)
    prd = {k: blocky() for k in ("ct_001", "t1out_002", "ct_003")}
    gt = {k: blocky() for k in prd}
    dev = lambda d: {k: torch.from_numpy(v.astype(np.uint8)).cuda() for k, v in d.items()}
    for fn in (utils.get_all_matrix, utils.get_hd_matrix):
        want, got = fn(prd, gt), fn(dev(prd), dev(gt))
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
        assert want[-1].max() > 0.0
        assert all(np.array_equal(a, b) for a, b in zip(fn(dev(prd), gt), want))       # mixed: device prediction, NumPy truth
        for bad in (lambda v: torch.from_numpy(v).float().cuda(), lambda v: torch.from_numpy(v.astype(np.uint8)),
                    lambda v: torch.from_numpy(v).cuda()):                             # float | CPU | int64 on the device
            with pytest.raises(TypeError):
                fn({k: bad(v) for k, v in prd.items()}, gt)


def test_dice_counter_refuses_a_repeated_name_and_grows_on_the_device(cfg_fix):
    from smsut_amd.misc.utils import DiceCounter, dice_matrix_from_counts
    rs = np.random.RandomState(9)
    z = torch.from_numpy(rs.standard_normal((2, 5, 8, 8)).astype(np.float32)).cuda().contiguous(memory_format=torch.channels_last)
    lab = torch.from_numpy(rs.randint(0, 5, (2, 8, 8))).cuda()
    counter = DiceCounter(slots=1)
    assert counter.update(z, lab, ["ct_001_0", "ct_001_1"]) is None
    first = counter.counts.clone()
    for names in (["ct_001_1", "ct_001_2"], ["t2_004_0", "t2_004_0"]):          # seen before | twice in one batch
        with pytest.raises(ValueError):
            counter.update(z, lab, names)
    assert counter.keys == ["ct_001"] and torch.equal(counter.counts, first)     # a refused batch leaves no trace
    pred = counter.update(z, lab, ["t2_004_0", "t1in_002_0"], want_pred=True)    # two new volumes: 1 slot -> 4, on the device
    counter.update(z, lab, ["ct_001_2", "t1out_009_5"])
    assert counter.keys == ["ct_001", "t2_004", "t1in_002", "t1out_009"] and counter.counts.shape[0] >= 4
    assert pred.dtype == torch.uint8 and torch.equal(pred.long(), z.argmax(1))
    got = counter.counts[:4].cpu().numpy()
    assert (got[0] == first[0].cpu().numpy() + got[1]).all()                     # ct_001: both slices, then slice 0 again
    assert got[:, :, 1].sum() == 6 * 64
    assert (counter.matrix() == dice_matrix_from_counts(counter.keys, got)).all()
    with pytest.raises(ValueError):
        counter.update(z, lab, ["ct_011_0", "ct_011_1"], classes=3)              # another class count than before
