"""CoraNet without a GPU: the new entry points exist at every layer (header, library, ctypes table, trainer module, config), and
the fp64 restatement the GPU tests use as their reference (tests/coranet_ref.py) reproduces every scalar of tests/golden/coranet.npz,
which the reference's own modules produced (tests/golden/make_coranet_golden.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import coranet_ref as R
from oracle import recipe, smsut_oracle as O

ENTRY_POINTS = ("smsut_cora_ws", "smsut_cora_sup_stats", "smsut_cora_sup_final", "smsut_cora_sup_bwd", "smsut_cora_semi_stats",
                "smsut_cora_semi_final", "smsut_cora_semi_bwd", "smsut_cora_pseudo", "smsut_ema_multi", "smsut_ema_chunk")


def test_entry_points_trainer_module_and_class_weights():
    ge.build()
    header = open(os.path.join(ge.ROOT, "include", "smsut_hip.h")).read()
    lib = ctypes.CDLL(ge.LIB)
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip, config as cfg
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} not declared in include/smsut_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _hip.SIGNATURES
    assert "smsut_cora_ws" in _hip._RET_I64
    lib.smsut_cora_ws.restype = ctypes.c_int64
    lib.smsut_cora_ws.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int]
    for (n, hw, L) in ((8, 65536, 4), (1, 64, 10), (3, 1600, 1)):
        ws = lib.smsut_cora_ws(n, hw, L)
        per = 3 * (L + 1) + 4
        assert ws % (n * per) == 0 and 1 <= ws // (n * per) <= 128        # blocks per sample x the wider of the two statistics rows
    assert lib.smsut_ema_chunk() == lib.smsut_sgd_chunk()

    from smsut_amd.trainer import coraNetTrainer as mod
    assert issubclass(mod.coraNetTrainer, smsut_amd.trainer.baseTrainer.BaseTrainer)
    parser = mod.make_parser()
    for phase in ("pretrain", "train", "test", "pseudo"):
        assert parser.parse_args(["-p", phase, "-f", "1", "-nm", "x", "-i", "000", "-wh", "best"]).phase == phase
    with pytest.raises(SystemExit):
        parser.parse_args(["-p", "nonsense"])

    assert (cfg.thres, cfg.pre_epoch, cfg.cora_epoch, cfg.pred_step) == (0.5, 100, 200, 10)
    old = cfg.n_label
    try:
        cfg.n_label = 4
        assert cfg.class_weights(cfg.w_con) == [1, 5, 5, 5, 5] and cfg.class_weights(cfg.w_rad) == [5, 1, 1, 1, 1]
        assert cfg.class_weights(cfg.default_w) == [1, 1, 1, 1, 1]
        cfg.n_label = 1
        assert cfg.class_weights(cfg.w_con) == [1, 5] and cfg.class_weights(cfg.w_rad) == [5, 1]
    finally:
        cfg.n_label = old


def close(got, ref, tol=1e-6):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(got - ref) <= tol * np.abs(ref))), (got, ref)


def test_restatement_reproduces_the_logits_only_case(golden):
    """the reference's loss modules in fp64 on stored logits, against the restatement in fp64: 1e-6 relative"""
    g = golden("coranet")
    z, e, y, q, m = R.loss_case()
    wc, wr = torch.tensor(R.W_CON), torch.tensor(R.W_RAD)
    assert all(close(R.sup_loss(z.double(), y, wc, wr).tolist(), g["case_sup"]))
    cw = float(g["case_cw"])
    for tag, mm in (("", m), ("_m1", torch.ones_like(m)), ("_m0", torch.zeros_like(m))):
        ok, rep = close(R.semi_loss(z.double(), e.double(), q, mm, cw).tolist(), g["case_semi" + tag])
        assert ok, (tag, rep)
    assert float(g["case_semi_m1"][1]) == 0.0                             # nothing uncertain: the consistency term vanishes
    qp, mp = R.pseudo(z)
    assert np.array_equal(qp.numpy(), g["case_plab"]) and np.array_equal(mp.numpy(), g["case_mask"])


def test_restatement_reproduces_every_trainer_scalar(golden):
    """The fixture's steps replayed with the in-tree U-Net oracle (fp32, as the reference ran) and the restatement in fp64 on its
    logits: every recorded scalar to 1e-6 relative, the weights after the last step, pred_unlabel and the validation batch."""
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    g = golden("coranet")
    assert (int(g["L"]), int(g["width"]), int(g["H"]), int(g["bs"]), int(g["epoch"])) == (R.L, R.WIDTH, R.SIZE, R.BS, R.EPOCH)
    wc, wr = torch.tensor(R.W_CON), torch.tensor(R.W_RAD)
    cw = R.rampup(R.EPOCH, 30)
    for name, (it0, seeds) in R.SCENARIOS.items():
        sd = {k: v.clone().requires_grad_(True) for k, v in recipe.fill(R.shapes(), R.SEED_STUDENT).items()}
        ema = {k: v.clone() for k, v in recipe.fill(R.shapes(), R.SEED_TEACHER).items()}
        opt = torch.optim.SGD(list(sd.values()), lr=R.LR, momentum=R.MOMENTUM, weight_decay=R.WD)
        assert g[name + "_scalars"].shape == (len(seeds), 6)
        for k, seed in enumerate(seeds):
            it = it0 + k
            img1, msk, img2 = R.step_inputs(seed)
            sup = R.sup_loss(O.unet_forward(sd, img1).double(), msk, wc, wr)
            semi, total = torch.zeros(2, dtype=torch.float64), sup[0]
            if name != "pre" and it >= 1000:
                q = torch.from_numpy(g[name + "_plab"][k].astype(np.int64))
                m = torch.from_numpy(g[name + "_mask"][k].astype(np.float32))
                with torch.no_grad():
                    e = O.unet_forward(ema, img2)
                semi = R.semi_loss(O.unet_forward(sd, img2).double(), e.double(), q, m, cw)
                total = total + semi[0] + 0.1 * semi[1]
            opt.zero_grad(); total.backward(); opt.step()
            with torch.no_grad():
                new = R.ema(list(ema.values()), [v.detach() for v in sd.values()], R.ema_alpha(it))
                for t, v in zip(ema.values(), new):
                    t.copy_(v)
            if name != "pre":
                for grp in opt.param_groups:
                    grp["lr"] = R.LR * (1.0 - it / R.MAX_IT) ** 0.9
            ok, rep = close(sup.tolist() + semi.tolist(), g[name + "_scalars"][k])
            assert ok, (name, k, rep)
        if name == "t500":
            assert g["t500_scalars"][0, 4] == 0.0 and g["t500_scalars"][0, 5] == 0.0
        if name == "pre":
            assert np.array_equal(g["pre_post_fc"], g["pre_post_ema_fc"])             # alpha = 0: the teacher is the student
    from conftest import rel_err
    assert rel_err(sd["decoder.fc.weight"].detach().numpy(), g["post_fc"]) < 1e-5
    assert rel_err(sd["encoder.pre_conv.weight"].detach().numpy(), g["post_pre"]) < 1e-5
    assert rel_err(ema["decoder.fc.weight"].numpy(), g["post_ema_fc"]) < 1e-5
    assert rel_err(ema["encoder.pre_conv.weight"].numpy(), g["post_ema_pre"]) < 1e-5

    sd = recipe.fill(R.shapes(), R.SEED_STUDENT)
    with torch.no_grad():
        img, lab = R.pred_inputs()
        q, m = R.pseudo(O.unet_forward(sd, img))
        assert (q.numpy() != g["pred_plab"]).mean() <= 0.01 and (m.numpy() != g["pred_mask"]).mean() <= 0.01
        dice = np.mean([R.binary_dc(g["pred_plab"][i], lab[i].numpy()) for i in range(R.PRED_SLICES)])
        assert abs(dice - float(g["pred_dice"])) < 1e-12
        img, msk = R.val_inputs()
        ok, rep = close(R.sup_loss(O.unet_forward(sd, img).double(), msk, wc, wr).tolist(), g["val_loss"])
        assert ok, rep
