"""Dual-task consistency on the GPU (csrc/dtc.hip, network/dtc.py, trainer/dtcTrainer.py) against tests/dtc_ref.py (pinned to brute
force, scipy and the reference's modules by tests/test_dtc_cpu.py and tests/golden/dtc.npz).

Bars.  ``edt_sq``: integer equality.  ``signed_distance_map``: |got - fp64| <= 1e-6 (two correctly rounded square roots and one division
of exact integers are at most 3 * 2^-24 = 1.8e-7 from fp64; 1e-6 is still below the effect of any wrong neighbour at these sizes), the
boundary / empty / full values exact.  ``dtc_loss``: the bars of this kernel family in tests/test_coranet_gpu.py, scalars
1e-6 + 2e-5 |ref|, gradients rel_err < 2e-5.  Trainer: first step as ``test_mean_teacher_iterations_match_golden``; the second step and
the weights after it pass through sigmoid(-1500 t), so their bar is four times the distance between the fixture's fp32 and fp64 CPU
replays of the same arithmetic and never less than 2e-2 (both printed); those bars exceed the whole update of two steps, so the weight
UPDATE (after - initial) is also held to rel_err < 0.1 against the fixture's, which a trainer that drops a term or a step misses."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import dtc_ref as R
from conftest import rel_err
from oracle import recipe

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def edt_case(name, b, c, h, w):
    """(labels int64 [b, h, w], d2 int32, sdf fp64): computed once, shared by the tests, never modified"""
    lab = R.label_pattern(name, b, c, h, w)
    d2, sdf = R.sdf(lab, c)
    for a in (lab, d2, sdf):
        a.setflags(write=False)
    return lab, d2, sdf


# ------------------------------------------------------------------------------------------- distance transform
@pytest.mark.parametrize("shape", R.EDT_SHAPES, ids=lambda s: "B%d_C%d_%dx%d" % s)
def test_edt_sq_is_exact(shape):
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    b, c, h, w = shape
    for name in R.PATTERNS:
        lab, d2, _ = edt_case(name, b, c, h, w)
        got = ops.edt_sq(torch.from_numpy(lab.copy()).cuda(), c)
        assert got.dtype == torch.int32 and tuple(got.shape) == (b, c, h, w)
        got = got.cpu().numpy()
        bad = int((got != d2).sum())
        assert bad == 0, (name, shape, bad, np.argwhere(got != d2)[:5])
        if name == "checker":
            assert h * w == 1 or np.all(got[:, :2] == 1)
        if name == "corner":
            assert got[0, c - 1, 0, 0] == (h - 1) ** 2 + (w - 1) ** 2             # the column search spans the whole column
        if name == "absent" and c > 1 and h * w > 1:
            assert np.all(got[:, 1] == 0) and np.all(got[-1] == 0)                 # the empty and the full image in one call


@pytest.mark.parametrize("shape", R.EDT_SHAPES, ids=lambda s: "B%d_C%d_%dx%d" % s)
def test_signed_distance_map(shape):
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    b, c, h, w = shape
    worst = 0.0
    for name in R.PATTERNS:
        lab, d2, sdf = edt_case(name, b, c, h, w)
        got = ops.signed_distance_map(torch.from_numpy(lab.copy()).cuda(), c)
        assert got.dtype == torch.float32 and tuple(got.shape) == (b, c, h, w) and not got.requires_grad
        assert got.stride() == (h * w * c, 1, w * c, c)                            # channels-last memory
        got = got.cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(got))
        worst = max(worst, float(np.abs(got - sdf).max()))
        p = R.class_masks(lab, c)
        assert np.all(got[p & (d2 == 1)] == 0.0), name                             # the inner boundary, exactly
        flat = d2.max(axis=(2, 3), keepdims=True) == 0
        assert np.all(got[np.broadcast_to(flat, p.shape) & ~p] == 1.0) and np.all(got[np.broadcast_to(flat, p.shape) & p] == -1.0), name
    print(shape, "max |sdf - fp64| =", worst)
    assert worst <= 1e-6, (shape, worst)


def test_sdf_arguments_are_checked():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    lab = torch.from_numpy(R.label_pattern("blobs", 2, 3, 20, 24)).cuda()
    try:
        ops.sdf_check()                                                            # (start from a clear flag)
    except ValueError:
        pass
    for bad_value in (3, -1):
        bad = lab.clone()
        bad[1, 7, 5] = bad_value
        with pytest.raises(ValueError):
            ops.signed_distance_map(bad, 3, validate=True)                         # a label outside [0, C)
    ops.signed_distance_map(lab, 3, validate=True)                                 # the flag was cleared by the raise
    ops.signed_distance_map(lab.clone().fill_(2), 3, validate=True)
    with pytest.raises(ValueError):
        ops.edt_sq(lab, 17)
    with pytest.raises(ValueError):
        ops.edt_sq(lab, 0)
    with pytest.raises(ValueError):
        ops.signed_distance_map(torch.zeros(1, 513, 8, dtype=torch.int64, device="cuda"), 2)
    with pytest.raises(ValueError):
        ops.signed_distance_map(torch.zeros(1, 8, 513, dtype=torch.int64, device="cuda"), 2)
    with pytest.raises(TypeError):
        ops.signed_distance_map(lab.int(), 3)
    with pytest.raises(TypeError):
        ops.signed_distance_map(lab[0], 3)


# ------------------------------------------------------------------------------------------- loss
def dev(x):
    return x.cuda().contiguous(memory_format=torch.channels_last)


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


def check_loss(ops, t, z, s, what, need_live=False, k=R.K):
    for co in ((1.0, 0.0), (0.0, 1.0), (0.3, 0.7)):
        td, zd = t.double().requires_grad_(True), z.double().requires_grad_(True)
        ref = R.dtc_loss(td, zd, s.double(), k)
        (co[0] * ref[0] + co[1] * ref[1]).backward()
        tg, zg = dev(t).requires_grad_(True), dev(z).requires_grad_(True)
        got = ops.dtc_loss(tg, zg, dev(s), k)
        assert tuple(got.shape) == (2,) and got.dtype == torch.float32
        (co[0] * got[0] + co[1] * got[1]).backward()
        scalars_close(got.tolist(), ref.tolist(), what)
        grad_close(tg.grad, td.grad, what + f" d/dt {co}")
        grad_close(zg.grad, zd.grad, what + f" d/dz {co}")
        if need_live and co == (0.0, 1.0):                     # the unsaturated sigmoid is exercised, or the test shows nothing
            live = float((td.grad != 0).double().mean())
            print(what, "share of pixels with a non-zero fp64 d L_cons / dt:", live)
            assert live >= 0.25, (what, live)
    return got, tg.grad, zg.grad


@pytest.mark.parametrize("shape", R.LOSS_SHAPES, ids=lambda s: "N%d_B%d_C%d_%dx%d" % s)
def test_dtc_loss_matches_fp64_restatement(shape):
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    n, b, c, h, w = shape
    t, z, s = R.loss_case(n, b, c, h, w, 11 + c)
    check_loss(ops, t, z, s, str(shape), need_live=True)


def test_dtc_loss_edge_cases():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    n, b, c, h, w = 4, 2, 5, 17, 19                          # HW = 323: not a multiple of 256
    t, z, s = R.loss_case(n, b, c, h, w, 21)
    sign = torch.where(torch.from_numpy(np.random.RandomState(1).uniform(size=tuple(t.shape)) < 0.5), 1.0, -1.0).float()
    check_loss(ops, sign, z, s, "t = +-1")                   # k t = +-1500: exp overflows onto 0 or 1, never NaN
    got, gt, gz = check_loss(ops, torch.zeros_like(t), z, s, "t = 0")           # sigma = 0.5 everywhere
    want = ((0.5 - torch.softmax(z.double(), 1)) ** 2).mean().item()
    assert abs(got[1].item() - want) <= 1e-6 + 2e-5 * want
    # sdf = t[:B]: L_sdf is exactly 0 and contributes an exactly zero gradient
    tg, zg = dev(t).requires_grad_(True), dev(z).requires_grad_(True)
    got = ops.dtc_loss(tg, zg, dev(t[:b].clone()), R.K)
    got[0].backward()
    assert got[0].item() == 0.0 and tg.grad.abs().max().item() == 0.0 and zg.grad.abs().max().item() == 0.0
    check_loss(ops, t, z, t[:b].clone(), "sdf = t[:B]")
    for cc in (3, 16):                                       # the runtime-C form of the kernels (C not one of 1, 2, 5)
        check_loss(ops, *R.loss_case(3, 2, cc, 9, 31, 25 + cc), f"C = {cc}", need_live=True)
    # two runs: bit-identical scalars and gradients
    t, z, s = R.loss_case(16, 8, 5, 64, 64, 23)
    runs = []
    for _ in range(2):
        tg, zg = dev(t).requires_grad_(True), dev(z).requires_grad_(True)
        out = ops.dtc_loss(tg, zg, dev(s), R.K)
        (0.3 * out[0] + 0.7 * out[1]).backward()
        runs.append((out.detach().clone(), tg.grad.clone(), zg.grad.clone()))
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_)
    with pytest.raises(ValueError):
        ops.dtc_loss(dev(t), dev(z), dev(torch.cat([s, s, s])), R.K)              # B > N
    with pytest.raises(ValueError):
        ops.dtc_loss(dev(t), dev(z[:, :4]), dev(s), R.K)


def test_sdf_and_loss_forward_capture_into_one_graph():
    """Nothing in ``signed_distance_map`` or the forward of ``dtc_loss`` synchronises with the host: after one eager call both are
    captured in one graph on one stream (no parallel branches) and the replay reproduces the eager results bit for bit."""
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    n, b, c, h, w = 4, 2, 5, 64, 96
    t, z, _ = R.loss_case(n, b, c, h, w, 31)
    lab = torch.from_numpy(R.label_pattern("blobs", b, c, h, w)).cuda()
    t, z = dev(t), dev(z)
    with torch.no_grad():
        sdf_e = ops.signed_distance_map(lab, c)
        out_e = ops.dtc_loss(t, z, sdf_e, R.K)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        sdf_g = ops.signed_distance_map(lab, c)
        out_g = ops.dtc_loss(t, z, sdf_g, R.K)
    sdf_g.zero_(); out_g.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sdf_g, sdf_e) and torch.equal(out_g, out_e)
    lab2 = torch.from_numpy(R.label_pattern("half", b, c, h, w)).cuda()        # new labels in the captured buffer, replayed
    with torch.no_grad():
        sdf_e2 = ops.signed_distance_map(lab2, c)
        out_e2 = ops.dtc_loss(t, z, sdf_e2, R.K)
    lab.copy_(lab2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sdf_g, sdf_e2) and torch.equal(out_g, out_e2)
    del graph


# ------------------------------------------------------------------------------------------- network
def test_network_matches_reference_fixture(golden):
    import smsut_amd  # noqa: F401
    from smsut_amd.network.dtc import UNet
    g = golden("dtc")
    net = UNet(1, R.C, R.WIDTH, norm_type="instance", act_type="lrelu")
    sd = net.state_dict()
    assert list(sd.keys()) == list(g["keys"])
    for v, row in zip(sd.values(), g["shapes"]):
        assert tuple(v.shape) == tuple(int(x) for x in row[:v.dim()])
    assert "decoder.fc1.0.weight" in sd and "decoder.fc2.weight" in sd
    net.load_state_dict(recipe.fill(R.shapes(), R.SEED_NET))
    net.cuda().train()
    x = R.fwd_input().cuda()
    t, z = net(x)
    assert t.shape == z.shape == (2, R.C, R.SIZE, R.SIZE)
    et, ez = rel_err(t.detach().cpu().numpy(), g["fwd_tanh"]), rel_err(z.detach().cpu().numpy(), g["fwd_logits"])
    print("tanh head rel_err", et, "logits rel_err", ez)
    assert et < 1e-3 and ez < 1e-3
    assert t.abs().max().item() <= 1.0
    (t.sum() + z.sum()).backward()
    for p in (net.decoder.fc1[0].weight, net.decoder.fc2.weight, net.encoder.pre_conv.weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0.0


# ------------------------------------------------------------------------------------------- trainer
@pytest.fixture()
def cfg_fix(tmp_path):
    """5 classes, base width 8, 32 x 32, bs 2 -- the fixture's configuration; runs write below tmp_path."""
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    names = ("input_size", "batch_size", "n_label", "base_width", "num_iter_per_epoch", "max_epoch", "expr_root")
    old = [getattr(cfg, k) for k in names]
    cfg.input_size, cfg.batch_size, cfg.n_label, cfg.base_width = R.SIZE, R.BS, R.C - 1, R.WIDTH
    cfg.expr_root = str(tmp_path)
    yield cfg
    for k, v in zip(names, old):
        setattr(cfg, k, v)


NS = types.SimpleNamespace(fold=0, expr_name=None, write_env=False, model_id=None)


def test_trainer_steps_match_golden(cfg_fix, golden):
    from smsut_amd.trainer.dtcTrainer import dtcTrainer
    g = golden("dtc")
    s32, s64 = g["scalars32"], g["scalars64"]
    d_scal = float((np.abs(s32[1] - s64[1]) / np.abs(s64[1])).max())
    d_w = max(rel_err(g["post32_" + k], g["post64_" + k]) for k in ("fc1", "fc2", "pre"))
    bar_scal, bar_w = max(4 * d_scal, 2e-2), max(4 * d_w, 2e-2)
    print("fp32 vs fp64 CPU replay: second-step scalars %.2e, weights %.2e -> bars %.2e, %.2e" % (d_scal, d_w, bar_scal, bar_w))
    tr = dtcTrainer("train", NS)
    assert (tr.beta, tr.k, tr.consistency, tr.epoch_rampup) == (R.BETA, R.K, R.CONSISTENCY, R.RAMPUP)
    tr.net.load_state_dict(recipe.fill(R.shapes(), R.SEED_NET))
    tr.net.train()
    tr.epoch, tr.iter = R.EPOCH, R.IT0
    for k, seed in enumerate(R.STEP_SEEDS):
        img, msk = R.step_inputs(seed)
        got = tr.train_iteration(img.cuda(), msk.cuda())
        assert got.is_cuda and tuple(got.shape) == (3,)
        got, ref = np.array(got.tolist()), s32[k]
        print("step", k, "got", got, "ref", ref, "rel", np.abs(got - ref) / np.abs(ref))
        if k == 0:
            assert abs(got[0] - ref[0]) <= 1e-3 * abs(ref[0]) + 1e-5, (got, ref)
            assert np.all(np.abs(got[1:] - ref[1:]) <= 1e-3 * np.abs(ref[1:]) + 1e-7), (got, ref)
        else:
            assert np.all(np.abs(got - ref) <= bar_scal * np.abs(ref) + 1e-7), (got, ref)
    assert tr.iter == R.IT0 + 2
    assert abs(tr.optimizer.param_groups[0]["lr"] - R.LR * (1.0 - (R.IT0 + 1) / R.MAX_IT) ** 0.9) < 1e-12
    sd, init = tr.net.state_dict(), recipe.fill(R.shapes(), R.SEED_NET)
    for k, name in (("fc1", "decoder.fc1.0.weight"), ("fc2", "decoder.fc2.weight"), ("pre", "encoder.pre_conv.weight")):
        got_w, w0, ref_w = sd[name].cpu().numpy().astype(np.float64), init[name].numpy().astype(np.float64), g["post32_" + k].astype(np.float64)
        err = rel_err(got_w, ref_w)
        # bar_w is wider than the two steps' whole update (6.5e-3 at most), so the UPDATE is compared too: a trainer that does not
        # backpropagate or step gives 1.0 here, one that drops beta * L_sdf 0.78 / 0.27 (fc1 / pre_conv), one that drops the
        # consistency term 0.31 - 0.43; the fp64 CPU replay is within 1.5e-2 (figures: docstring of tests/golden/make_dtc_golden.py)
        upd = rel_err(got_w - w0, ref_w - w0)
        print(name, "rel_err after two steps", err, "rel_err of the update", upd)
        assert err < bar_w, (name, err)
        assert upd < 0.1, (name, upd)


def test_fit_then_test_phase_run_to_the_end(cfg_fix):
    """``-p train`` for two short epochs on the synthetic slices writes best / last; ``-p test`` on the result scores the logits head."""
    cfg = cfg_fix
    cfg.num_iter_per_epoch, cfg.max_epoch = 3, 2
    from smsut_amd.trainer import dtcTrainer as T
    T.main(["-p", "train", "-nm", "dtc"])
    root = os.path.join(cfg.expr_root, "dtc", "000")
    for f in ("best.ckpt", "last.ckpt"):
        assert os.path.exists(os.path.join(root, "ckpt", f)), f
    sd = torch.load(os.path.join(root, "ckpt", "last.ckpt"), map_location="cpu")
    assert list(sd.keys()) == list(R.shapes().keys()) and all(torch.isfinite(v).all() for v in sd.values())
    T.main(["-p", "test", "-nm", "dtc", "-i", "000", "-wh", "last"])
    mo = np.loadtxt(os.path.join(root, "dice_matrix.csv"), delimiter=",")
    assert mo.shape == (cfg.n_modal + 1, cfg.n_label + 1) and np.all(np.isfinite(mo)) and np.all((mo >= 0) & (mo <= 1))
