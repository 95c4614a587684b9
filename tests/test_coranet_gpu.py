"""CoraNet on the GPU: the fused three-head kernels (csrc/coranet.hip) against the fp64 restatement of tests/coranet_ref.py (pinned to
the reference's modules by tests/test_coranet_cpu.py), and ``coraNetTrainer`` against tests/golden/coranet.npz.

Bars of the kernel tests: scalars 1e-6 + 2e-5 |ref|, gradients rel_err < 2e-5 -- what ``test_softmax_mse_and_argmax_kernels`` sets for
this kernel family (torch's own fp32 evaluation is within 5e-7 of fp64 on these shapes; the rest is for __expf / __logf and the order
of summation).  Bars of the trainer tests: those of ``test_mean_teacher_iterations_match_golden``."""
import os
import types

import numpy as np
import pytest
import torch

import coranet_ref as R
from conftest import rel_err
from oracle import recipe

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 24, 40), (8, 4, 64, 64), (3, 1, 40, 40), (1, 10, 8, 8), (2, 4, 256, 256)]       # (N, L, H, W)


def weights(L):
    return torch.tensor([1.0] + [5.0] * L), torch.tensor([5.0] + [1.0] * L)


def make_case(n, L, h, w, seed):
    rs = np.random.RandomState(seed)
    z = torch.from_numpy(2 * rs.standard_normal((n, 3 * L + 1, h, w))).float()
    e = torch.from_numpy(2 * rs.standard_normal((n, 3 * L + 1, h, w))).float()
    y = torch.from_numpy(rs.randint(0, L + 1, (n, h, w)).astype(np.int64))
    q = torch.from_numpy(rs.randint(0, L + 1, (n, h, w)).astype(np.int64))
    m = torch.from_numpy((rs.uniform(size=(n, h, w)) < 0.6).astype(np.float32))
    return z, e, y, q, m


def dev_logits(z):
    return z.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)


def scalars_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    print(what, "got", got, "ref", ref, "err", np.abs(got - ref))
    assert np.all(np.isfinite(got)), (what, got)
    assert np.all(np.abs(got - ref) <= 1e-6 + 2e-5 * np.abs(ref)), (what, got, ref)


def grad_close(got, ref, what):
    got, ref = got.cpu().numpy(), ref.numpy()
    assert np.all(np.isfinite(got)), what
    if np.abs(ref).max() == 0.0:
        assert np.abs(got).max() == 0.0, what
        return
    err = rel_err(got, ref)
    print(what, "gradient rel_err", err)
    assert err < 2e-5, (what, err)


def check_sup(ops, z, y, what):
    L = R.n_labels(z)
    wc, wr = weights(L)
    zd = z.double().requires_grad_(True)
    ref = R.sup_loss(zd, y, wc, wr, 0.5, 0.5)
    ref[0].backward()
    zg = dev_logits(z)
    got = ops.cora_sup_loss(zg, y.cuda(), wc.cuda(), wr.cuda(), 0.5, 0.5)
    got[0].backward()
    scalars_close(got.tolist(), ref.tolist(), what + " sup")
    grad_close(zg.grad, zd.grad, what + " sup")


def check_semi(ops, z, e, q, m, cw, what):
    for co in ((1.0, 0.1), (0.0, 1.0)):                      # the trainer's combination, and the consistency term alone
        zd = z.double().requires_grad_(True)
        ref = R.semi_loss(zd, e.double(), q, m, cw)
        (co[0] * ref[0] + co[1] * ref[1]).backward()
        zg = dev_logits(z)
        got = ops.cora_semi_loss(zg, e.cuda().contiguous(memory_format=torch.channels_last), q.cuda(), m.cuda(), cw)
        (co[0] * got[0] + co[1] * got[1]).backward()
        scalars_close(got.tolist(), ref.tolist(), what + " semi")
        grad_close(zg.grad, zd.grad, what + f" semi {co}")
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d_L%d_%dx%d" % s)
def test_head_kernels_match_fp64_restatement(shape):
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    n, L, h, w = shape
    z, e, y, q, m = make_case(n, L, h, w, 11 + L)
    check_sup(ops, z, y, str(shape))
    check_semi(ops, z, e, q, m, 0.7, str(shape))


def test_head_kernels_edge_cases():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    n, L, h, w = 3, 4, 17, 19                               # HW = 323: not a multiple of 256
    z, e, y, q, m = make_case(n, L, h, w, 21)
    check_sup(ops, z, y, "odd HW")
    check_semi(ops, z, e, q, m, 0.7, "odd HW")
    got = check_semi(ops, z, e, q, torch.ones_like(m), 0.7, "mask all ones")
    assert got[1].item() == 0.0                              # (and its gradient is exactly zero: grad_close on the (0, 1) combination)
    got = check_semi(ops, z, e, q, torch.zeros_like(m), 0.7, "mask all zeros")
    ref_dice_only = R.soft_dice(R.heads(z.double())[0], q, False) / 2
    assert abs(got[0].item() - ref_dice_only.item()) <= 1e-6 + 2e-5 * ref_dice_only.item()       # masked CE = 0
    y2, q2 = y.clone(), q.clone()
    y2[y2 == 2] = 0; q2[q2 == 2] = 3                         # class 2 absent from labels and pseudo labels
    check_sup(ops, z, y2, "class absent")
    check_semi(ops, z, e, q2, m, 0.7, "class absent")


def test_cora_pseudo_equals_torch_argmax_exactly():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    for shape in SHAPES:
        n, L, h, w = shape
        z = make_case(n, L, h, w, 31)[0]
        q, m = ops.cora_pseudo(z.cuda().contiguous(memory_format=torch.channels_last))
        rq, rm = R.pseudo(z)
        assert q.dtype == torch.int64 and m.dtype == torch.float32
        assert torch.equal(q.cpu(), rq) and torch.equal(m.cpu(), rm), shape
    for L in (1, 2, 4, 10):
        tie = torch.zeros(1, 3 * L + 1, 4, 4)
        tie[:, 0] = 1.0                                      # background ties with a foreground class in every head ...
        for k in range(3):
            tie[:, 1 + k * L + (L - 1)] = 1.0                # ... the head's last class: the first maximum (background) wins
        tie[:, :, 0, 0] = 0.0
        tie[:, 1 + L, 0, 0] = 2.0                            # one pixel where heads 1 and 2 disagree
        if L > 1:
            tie[:, 1, 1, 1] = 3.0; tie[:, 2, 1, 1] = 3.0     # two foreground classes tie in head 0: the lower index wins
        q, m = ops.cora_pseudo(tie.cuda().contiguous(memory_format=torch.channels_last))
        rq, rm = R.pseudo(tie)
        assert torch.equal(q.cpu(), rq) and torch.equal(m.cpu(), rm), L
        assert rq[0, 2, 2] == 0 and rm[0, 2, 2] == 1.0 and rm[0, 0, 0] == 0.0


def test_ema_update_one_launch():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    torch.manual_seed(5)
    shapes = [(1,), (7,), (8192 * 3 + 5,), (8192,)]
    params = [torch.randn(s, device="cuda") for s in shapes]
    ema = [torch.randn(s, device="cuda") for s in shapes]
    w = ops.new_weight(16, 8, 3, 3, device="cuda"); w.copy_(torch.randn(16, 8, 3, 3))           # HWIO strides, as the conv weights
    we = ops.new_weight(16, 8, 3, 3, device="cuda"); we.copy_(torch.randn(16, 8, 3, 3))
    params.append(w); ema.append(we)
    ref = [e.clone() for e in ema]
    alpha = 0.99
    ops.ema_update(ema, params, alpha)
    for r, p in zip(ref, params):
        r.mul_(alpha).add_(p, alpha=1 - alpha)
    for e, r in zip(ema, ref):
        assert rel_err(e.cpu().numpy(), r.cpu().numpy()) < 1e-6
    ops.ema_update(ema, params, 0)
    for e, p in zip(ema, params):
        assert torch.equal(e, p)
    with pytest.raises(ValueError):
        ops.ema_update(ema, [p.contiguous() for p in params], 0.5)                             # another layout: refused, not converted


# ------------------------------------------------------------------------------------------- trainer vs the fixture
@pytest.fixture()
def cfg_fix(tmp_path):
    """3 classes (7 channels), base width 8, 64x64, bs 2 -- the fixture's configuration; runs write below tmp_path."""
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    names = ("input_size", "batch_size", "n_label", "base_width", "num_iter_per_epoch", "expr_root")
    old = [getattr(cfg, k) for k in names]
    cfg.input_size, cfg.batch_size, cfg.n_label, cfg.base_width = R.SIZE, R.BS, R.L, R.WIDTH
    cfg.expr_root = str(tmp_path)
    yield cfg
    for k, v in zip(names, old):
        setattr(cfg, k, v)


NS = types.SimpleNamespace(fold=0, expr_name=None, write_env=False, model_id=None)


def make_trainer(it, args=NS):
    from smsut_amd.trainer.coraNetTrainer import coraNetTrainer
    tr = coraNetTrainer("train", args)
    tr.net.load_state_dict(recipe.fill(R.shapes(), R.SEED_STUDENT))
    tr.ema.load_state_dict(recipe.fill(R.shapes(), R.SEED_TEACHER))
    tr.net.train(); tr.ema.train()
    tr.epoch, tr.iter = R.EPOCH, it
    return tr


def test_trainer_steps_match_golden(cfg_fix, golden):
    g = golden("coranet")
    cfg = cfg_fix
    # pretrain step at iteration 0
    tr = make_trainer(0)
    img1, msk, _ = R.step_inputs(R.SCENARIOS["pre"][1][0])
    got = tr.pretrain_iteration(img1.cuda(), msk.cuda()).tolist()
    ref = g["pre_scalars"][0]
    print("pre", got, ref)
    assert len(got) == 4 and np.all(np.abs(np.array(got) - ref[:4]) <= 1e-3 * np.abs(ref[:4]) + 1e-5), (got, ref)
    assert tr.iter == 1 and all(grp["lr"] == cfg.lr for grp in tr.optimizer.param_groups)       # no learning-rate change
    for pe, ps in zip(tr.ema.parameters(), tr.net.parameters()):
        assert torch.equal(pe, ps)                                                              # alpha = 0
    assert rel_err(tr.net.state_dict()["decoder.fc.weight"].cpu().numpy(), g["pre_post_fc"]) < 2e-3

    # train step at iteration 500: semi terms off
    tr = make_trainer(500)
    img1, msk, img2 = R.step_inputs(R.SCENARIOS["t500"][1][0])
    q = torch.from_numpy(g["t500_plab"][0].astype(np.int64)).cuda()
    m = torch.from_numpy(g["t500_mask"][0].astype(np.float32)).cuda()
    got = tr.train_iteration(img1.cuda(), msk.cuda(), img2.cuda(), q, m).tolist()
    ref = g["t500_scalars"][0]
    print("t500", got, ref)
    assert np.all(np.abs(np.array(got[:4]) - ref[:4]) <= 1e-3 * np.abs(ref[:4]) + 1e-5), (got, ref)
    assert got[4] == 0.0 and got[5] == 0.0
    assert abs(tr.optimizer.param_groups[0]["lr"] - R.LR * (1.0 - 500 / R.MAX_IT) ** 0.9) < 1e-12

    # two consecutive train steps at iterations 1200, 1201
    tr = make_trainer(1200)
    for k, seed in enumerate(R.SCENARIOS["t1200"][1]):
        img1, msk, img2 = R.step_inputs(seed)
        q = torch.from_numpy(g["t1200_plab"][k].astype(np.int64)).cuda()
        m = torch.from_numpy(g["t1200_mask"][k].astype(np.float32)).cuda()
        got = np.array(tr.train_iteration(img1.cuda(), msk.cuda(), img2.cuda(), q, m).tolist())
        ref = g["t1200_scalars"][k]
        print("t1200", k, got, ref)
        assert np.all(np.abs(got[:4] - ref[:4]) <= 1e-3 * np.abs(ref[:4]) + 1e-5), (k, got, ref)
        tol = 1e-3 if k == 0 else 2e-2                       # the second step passes through the updated weights
        assert np.all(np.abs(got[4:] - ref[4:]) <= tol * np.abs(ref[4:]) + 1e-7), (k, got, ref)
    assert tr.iter == 1202 and tr.alpha == 0.99
    sd, esd = tr.net.state_dict(), tr.ema.state_dict()
    assert rel_err(sd["decoder.fc.weight"].cpu().numpy(), g["post_fc"]) < 2e-3
    assert rel_err(sd["encoder.pre_conv.weight"].cpu().numpy(), g["post_pre"]) < 2e-3
    assert rel_err(esd["decoder.fc.weight"].cpu().numpy(), g["post_ema_fc"]) < 1e-4
    assert rel_err(esd["encoder.pre_conv.weight"].cpu().numpy(), g["post_ema_pre"]) < 1e-4


def test_pred_unlabel_and_validation_match_golden(cfg_fix, golden):
    g = golden("coranet")
    tr = make_trainer(0)
    assert list(tr.net.state_dict().keys()) == list(R.shapes().keys())
    assert all(tuple(v.shape) == tuple(R.shapes()[k]) for k, v in tr.net.state_dict().items())
    img, lab = R.pred_inputs()
    loader = [(img, lab, torch.zeros(R.PRED_SLICES, dtype=torch.int64), [f"ct_001_{z}" for z in range(R.PRED_SLICES)])]
    src, dice = tr.pred_unlabel(loader)
    plab, mask = src.plab.cpu().numpy(), src.mask.cpu().numpy()
    dq, dm = float((plab != g["pred_plab"]).mean()), float((mask != g["pred_mask"]).mean())
    print("pred_unlabel: differing pixels labels %.4f %%, mask %.4f %%" % (100 * dq, 100 * dm))
    assert dq <= 0.01 and dm <= 0.01
    assert src.plab.is_cuda and src.mask.is_cuda and src.img.is_cuda and src.mask.dtype == torch.float32
    assert abs(dice - np.mean([R.binary_dc(plab[i], lab[i].numpy()) for i in range(R.PRED_SLICES)])) < 1e-12
    seen = []
    assert len(src) == R.PRED_SLICES // R.BS
    for bi, bq, bm, bl, bmd in src:                          # shuffled, drop-last batches over the device tensors
        assert bi.shape == (R.BS, 1, R.SIZE, R.SIZE) and bq.shape == bm.shape == bl.shape == (R.BS, R.SIZE, R.SIZE)
        for i in range(R.BS):
            j = [k for k in range(R.PRED_SLICES) if torch.equal(bi[i].cpu(), img[k])]
            assert len(j) == 1 and torch.equal(bq[i], src.plab[j[0]]) and torch.equal(bl[i].cpu(), lab[j[0]])
            seen += j
    assert sorted(seen) == list(range(R.PRED_SLICES))

    # one validation batch: three-head supervised loss, prediction = argmax of head 0
    class Catch:
        def __init__(self):
            self.losses = []

        def collect_loss_by(self, loss, m, n):
            self.losses.append(loss)
            return {}, {}

        def accumulate(self, v, n):
            pass
    img, msk = R.val_inputs()
    names = [f"ct_002_{z}" for z in range(R.BS)]
    meter = Catch()
    n_prd, prd = tr.validate_epoch([(img, msk, torch.zeros(R.BS, dtype=torch.int64), names)], {"ct_002": msk.numpy()}, meter)
    ref = float(g["val_loss"][0])
    assert n_prd == R.BS and abs(meter.losses[0] - ref) <= 1e-3 * abs(ref), (meter.losses, ref)
    with torch.no_grad():
        want = R.pseudo(tr.net(img.cuda()).float().cpu())[0].numpy()
    assert (prd["ct_002"] != want).mean() <= 0.01


def test_checkpoints_prefit_and_fit_run_to_the_end(cfg_fix):
    cfg = cfg_fix
    cfg.num_iter_per_epoch = 3
    from smsut_amd.trainer.coraNetTrainer import coraNetTrainer
    args = types.SimpleNamespace(fold=0, expr_name="cora", write_env=True, model_id=None, iters_per_epoch=3)
    torch.manual_seed(3)
    tr = coraNetTrainer("train", args)
    ckpt = os.path.join(tr.expr_root, tr.model_idx, "ckpt")
    before = {k: v.clone() for k, v in tr.ema.state_dict().items()}
    tr.save_ema_model("probe")
    for p in tr.ema.parameters():
        p.zero_()
    tr.load_ema_model(tr.model_idx, "probe")
    for k, v in tr.ema.state_dict().items():
        assert torch.equal(v, before[k]), k                  # bit-exact round trip

    tr.prefit("synthetic", max_epoch=2)
    assert tr.iter == 6 and tr.epoch == 2
    for f in ("pre_best.ckpt", "pre_ema_best.ckpt", "pre_last.ckpt", "pre_ema_last.ckpt"):
        assert os.path.exists(os.path.join(ckpt, f)), f
    tr.semi_start_iter = 0                                   # exercise the pseudo-labelled terms in this short run
    tr.fit("synthetic", max_epoch=2)
    assert tr.iter == 12 and os.path.exists(os.path.join(ckpt, "last.ckpt"))
    img1, msk, img2 = R.step_inputs(77)
    q, m = __import__("smsut_amd").ops.cora_pseudo(tr.net(img2.cuda()))
    scal = tr.train_iteration(img1.cuda(), msk.cuda(), img2.cuda(), q, m).tolist()
    print("after prefit + fit:", scal)
    assert len(scal) == 6 and all(np.isfinite(scal)) and scal[4] > 0.0 and scal[5] >= 0.0      # (teacher ~ student this early: alpha = 0)
    assert all(torch.isfinite(p).all() for p in tr.net.parameters()) and all(torch.isfinite(p).all() for p in tr.ema.parameters())
