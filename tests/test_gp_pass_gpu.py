"""The discriminator's gradient-penalty pass -- the backward of the backward that ``d_loss.backward()`` runs after
``autograd.grad(out_src, x_hat, create_graph=True)`` (trainer/uganShp0Trainer.gradient_penalty) -- against fp64.

Part A: every conv family of the discriminator differentiated twice, against the closed forms in fp64 (gx = dgrad(gy, w),
dL/dgy = conv(v, w), dL/dw = wgrad(v, gy) for L = sum(gx * v)), inside and outside ``ops.input_grads_only()``, at the bars the same
kernels meet once-differentiated in ``test_conv2d_fwd_dgrad_wgrad`` (1e-5 data gradient / forward, 5e-5 weight gradient), with the
entry points and integer arguments of every launch asserted from a reading of ``ops._conv_*_launch``.
Part B: one stride-2 ``BottleBlock`` in its downsample and identity forms, with the penalty's cotangent of ones and with a differentiated
random one (the only consumer of the final activation's second-order result); part C: a whole ``Discriminator`` with the capped identity block
and the full-window ``conv_cls``, in the D step the trainers compose.  Reference: tests/gp_ref.py in fp64 with the activation masks of the
GPU run.  Bar of a tensor: max(4 * d32, single-op bar), d32 = rel_err(fp32 CPU replay with the same masks, fp64) -- four times the same
arithmetic's own fp32 noise, as tests/test_dtc_gpu.py allows a different summation order; single-op bars 1e-5 (outputs, dydx), 5e-5
(second-order tensors: the InstanceNorm double-backward bar; weight gradients).  Scalars: |got - ref| <= 1e-6 + 2e-5 |ref|.

Measured on an MI355X: GPU error / d32, worst tensor of each group (every tensor is printed by the tests).  4 * d32 stayed below the
single-op bar everywhere, so every bar below IS the single-op bar: 1e-5 for out and dydx, 5e-5 for the rest.

    case                  out              dydx             d_x_hat          parameter gradients (worst)     d_cot (cotangent run)
    block  2 16->32 @16   5.7e-7 / 4.4e-7  6.7e-7 / 5.3e-7  5.9e-7 / 5.2e-7  1.3e-6 / 6.3e-7  bn1.weight     4.8e-7 / 3.6e-7
    block  3  8->16 @32   6.1e-7 / 4.6e-7  4.5e-7 / 5.2e-7  5.0e-7 / 4.3e-7  6.6e-7 / 7.4e-7  bn1.weight     4.5e-7 / 2.6e-7
    block  2 32->32 @8    6.5e-7 / 4.3e-7  5.8e-7 / 4.7e-7  8.9e-7 / 8.4e-7  1.7e-6 / 8.5e-7  conv2.weight   1.1e-6 / 4.9e-7
    block  2 256->256 @8  2.3e-6 / 1.1e-6  2.2e-6 / 2.0e-6  3.3e-6 / 2.8e-6  2.8e-6 / 2.4e-6  conv2.weight   2.7e-6 / 2.0e-6
    discriminator         5.4e-7 / 5.7e-7  4.0e-7 / 3.6e-7  8.8e-7 / 6.8e-7  2.0e-6 / 1.2e-6  main.2.conv1.weight
      out_cls 8.6e-7 / 7.9e-7; real|fake pass: out_src 7.4e-7 / 6.6e-7, out_cls 8.5e-7 / 1.2e-6
      scalars |got - fp64| (bar): d_real 6.3e-8 (1.8e-6), d_fake 1.2e-8 (1.1e-6), d_cls 6.3e-7 (5.4e-5), gp 9.4e-6 (8.4e-4)
    block gp |got - fp64| (bar): 4.8e-5 (1.3e-2), 4.3e-5 (3.0e-2), 1.5e-5 (2.1e-3), 3.5e-5 (2.0e-2)
    part A, worst of all cases: gx 2.3e-6, dL/dgy 1.7e-6 (bar 1e-5), dL/dw 2.6e-7 (bar 5e-5); Conv2dWgradFn.backward 8.0e-7, 5.3e-7
"""
import functools

import numpy as np
import pytest
import torch

import gp_ref as R
from conftest import rel_err
from conv_edge_helpers import conv_ref
from oracle import recipe

pytestmark = pytest.mark.gpu

A_SRC, B_GP = 1.0, 10.0          # block cases: loss = A_SRC * mean(out) + B_GP * gp (the affine shifts get a gradient from the first term only)


@pytest.fixture(scope="module")
def pkg():
    import smsut_amd
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from smsut_amd import ops
    assert ops.IN_EPS == R.IN_EPS
    return smsut_amd


def rnd(*shape, seed):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape)).float()


def act_dev(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def w_dev(ops, w):
    out = ops.new_weight(*w.shape, device="cuda")
    out.copy_(w)
    return out


def ints_of(name, args):
    from smsut_amd import _hip as H
    return [a for c, a in zip(H.SIGNATURES[name].replace(" ", ""), args) if c in "il"]


def calls(rec):
    return [(name, ints_of(name, args)) for name, args in rec]


def show(tag, rec):
    print(f"{tag}: " + " ".join(f"{n.replace('smsut_', '')}{tuple(i)}" for n, i in calls(rec)))


# ------------------------------------------------------------------------------------------- part A: conv families, twice
# (family, (N, H, W, Cin, Cout, k, stride, pad, bias))
CONV_CASES = [
    ("stem", (3, 32, 32, 1, 16, 4, 2, 1, True)),
    ("stem", (2, 30, 34, 1, 8, 4, 2, 1, True)),                # output 15 x 17
    ("c3", (2, 16, 16, 16, 32, 3, 1, 1, False)),
    ("c3", (2, 16, 16, 32, 32, 3, 1, 1, False)),
    ("c3", (2, 32, 32, 8, 16, 3, 1, 1, False)),                # 8-channel form
    ("c3", (1, 20, 12, 16, 32, 3, 1, 1, False)),               # ragged tiles
    ("c3_plane", (3, 8, 8, 64, 64, 3, 1, 1, False)),
    ("c3_plane", (2, 8, 8, 128, 256, 3, 1, 1, False)),
    ("c3_plane", (16, 4, 4, 256, 256, 3, 1, 1, False)),
    ("c3_persistent", (4, 128, 128, 16, 32, 3, 1, 1, False)),  # production level
    ("c1", (2, 16, 16, 8, 16, 1, 1, 0, False)),
    ("c1", (2, 8, 8, 16, 32, 1, 1, 0, False)),
    ("c1", (4, 4, 4, 128, 256, 1, 1, 0, False)),
    ("src", (2, 4, 4, 32, 1, 3, 1, 1, False)),
    ("src", (3, 4, 4, 256, 1, 3, 1, 1, False)),
    ("k4s1", (2, 9, 20, 20, 12, 4, 1, 1, False)),
]


def case_id(c):
    return c[0] + "_" + "x".join(str(int(v)) for v in c[1])


def family_calls(family, case):
    """(data gradient, forward, weight gradient): entry point and integer arguments of the launches ``ops._conv_dgrad_launch``,
    ``_conv_fwd_launch`` and ``_conv_wgrad_launch`` make for this layer, read from their dispatch ladders and the ``*_supported``
    queries (csrc):
      stem  4x4 s2 p1, Cin 1: not MFMA (k 4), not the k4 kernel (stride 2); ``small`` (Cin <= 8, Cout in 4..16), weight gradient ``flat``
      c3    3x3 s1 p1, Cin % 4 == 0: the MFMA conv (transposed = 1 for the data gradient) and ``wgrad_mfma``
      c1    1x1, Cin and Cout % 4 == 0: the streaming 1x1 kernel (transposed = 1 for the data gradient) and ``conv1x1_wgrad``
      src   3x3, Cout 1: forward MFMA (Ndim 1); data gradient generic (reduction width 1), weight gradient generic (Cout % 4 != 0, 9 Cin > 128)
      k4s1  4x4 s1 p1, channels % 4 == 0: the k4 MFMA kernels."""
    n, h, w, ci, co, k, s, p, _ = case
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    geom = [n, h, w, ci, ho, wo, co, k, s, p]
    if family == "stem":
        return (("smsut_conv2d_small_dgrad", geom), ("smsut_conv2d_small_fwd", geom), ("smsut_conv2d_flat_wgrad", geom))
    if family.startswith("c3"):
        return (("smsut_conv2d_fwd_mfma", [n, h, w, co, ci, 3, 1]), ("smsut_conv2d_fwd_mfma", [n, h, w, ci, co, 3, 0]),
                ("smsut_conv2d_wgrad_mfma", [n, h, w, ci, co, 3]))
    if family == "c1":
        return (("smsut_conv1x1_fwd", [n, h * w, co, ci, 1]), ("smsut_conv1x1_fwd", [n, h * w, ci, co, 0]),
                ("smsut_conv1x1_wgrad", [n, h * w, ci, co]))
    if family == "src":
        g11 = [n, h, w, ci, ho, wo, co, k, k, s, p]
        return (("smsut_conv2d_dgrad_generic", g11), ("smsut_conv2d_fwd_mfma", [n, h, w, ci, co, 3, 0]), ("smsut_conv2d_wgrad_generic", g11))
    assert family == "k4s1"
    return (("smsut_conv2d_k4_fwd", [n, h, w, ci, co, 1]), ("smsut_conv2d_k4_fwd", [n, h, w, ci, co, 0]),
            ("smsut_conv2d_k4_wgrad", [n, h, w, ci, co]))


def plane_wgrad_applies(n, h, w, ci, co):
    """csrc/conv_mfma.hip: the whole-batch weight gradient takes planes of at most 64 pixels; the register-row kernel, which is asked
    first, needs W % 16 == 0"""
    return h * w <= 64 and w % 4 == 0 and ci % 32 == 0 and co % 32 == 0 and n * h * w <= 4096 and w % 16 != 0


@functools.lru_cache(maxsize=None)
def conv_case(case):
    """inputs and fp64 closed forms of one case, computed once and shared: logical NCHW / OIHW CPU tensors"""
    n, h, w, ci, co, k, s, p, has_b = case
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    t = dict(x=rnd(n, ci, h, w, seed=1), w=rnd(co, ci, k, k, seed=2) / np.sqrt(ci * k * k), b=rnd(co, seed=3) if has_b else None,
             gy=rnd(n, co, ho, wo, seed=4), v=rnd(n, ci, h, w, seed=5), u=rnd(co, seed=6), U=rnd(co, ci, k, k, seed=7) / np.sqrt(ci * k * k))
    nhwc, hwio = (lambda a: a.permute(0, 2, 3, 1)), (lambda a: a.permute(2, 3, 1, 0))
    back, wback = (lambda a: a.permute(0, 3, 1, 2)), (lambda a: a.permute(3, 2, 0, 1))
    _, gx, _, _ = conv_ref(nhwc(t["x"]), hwio(t["w"]), None, s, p, nhwc(t["gy"]))
    _, _, gw_v, _ = conv_ref(nhwc(t["v"]), hwio(t["w"]), None, s, p, nhwc(t["gy"]))
    _, gx_U, _, _ = conv_ref(nhwc(t["x"]), hwio(t["U"]), None, s, p, nhwc(t["gy"]))
    t.update(gx=back(gx), d_gy=back(conv_ref(nhwc(t["v"]), hwio(t["w"]), None, s, p)), d_w=wback(gw_v),
             dx_U=back(gx_U), dgy_U=back(conv_ref(nhwc(t["x"]), hwio(t["U"]), None, s, p)))
    return t


def close(tag, got, ref, bar, fails):
    e = rel_err(got.detach().cpu().numpy(), ref.numpy())
    print(f"{tag}: rel_err {e:.3g} bar {bar:.3g}")
    assert tuple(got.shape) == tuple(ref.shape), tag
    if not e < bar:
        fails.append((tag, e, bar))


@pytest.mark.parametrize("fc", CONV_CASES, ids=case_id)
def test_conv_family_double_backward(pkg, fc):
    from smsut_amd import _hip as H, ops, profiling
    family, case = fc
    n, h, w, ci, co, k, s, p, has_b = case
    if family == "c3_persistent" and not H.call("smsut_conv2d_mfma_persistent", n, h, w, ci, co, 3, 0):
        pytest.skip("the persistent 3x3 kernel declines this shape")
    if family == "c3_plane":
        assert plane_wgrad_applies(n, h, w, ci, co)
    t = conv_case(case)
    xd = act_dev(t["x"]).requires_grad_(True)
    wd = w_dev(ops, t["w"]).requires_grad_(True)
    bd = t["b"].cuda().requires_grad_(True) if has_b else None
    gyd = act_dev(t["gy"]).requires_grad_(True)
    vd, ud = act_dev(t["v"]), t["u"].cuda()
    want_dgrad, want_fwd, want_wgrad = family_calls(family, case)
    fails = []
    copies = ops.layout_copies()
    for scope in ("input_grads_only", "default"):
        res = {}

        def first():
            y = ops.conv2d(xd, wd, bd, s, p)
            if scope == "input_grads_only":
                with ops.input_grads_only():
                    (res["gx"],) = torch.autograd.grad(y, xd, gyd, create_graph=True)
            elif has_b:
                res["gx"], res["gb"] = torch.autograd.grad(y, (xd, bd), gyd, create_graph=True)
            else:
                (res["gx"],) = torch.autograd.grad(y, xd, gyd, create_graph=True)

        def second():
            L = (res["gx"] * vd).sum()
            if "gb" in res:
                (res["d_gy_bias"],) = torch.autograd.grad((res["gb"] * ud).sum(), gyd, retain_graph=True)
                L = L + (res["gb"] * ud).sum()
            res["d_gy"], res["d_w"], res["d_x"] = torch.autograd.grad(L, (gyd, wd, xd), allow_unused=True)

        rec1 = profiling.record_step(first)
        rec2 = profiling.record_step(second)
        show(f"{scope} first grad", rec1)
        show(f"{scope} second-order pass", rec2)
        c1, c2 = calls(rec1), calls(rec2)
        assert (want_dgrad[0], want_dgrad[1]) in c1, (scope, want_dgrad)
        assert (want_fwd[0], want_fwd[1]) in c2, (scope, want_fwd)
        assert (want_wgrad[0], want_wgrad[1]) in c2, (scope, want_wgrad)
        if scope == "input_grads_only":
            assert not [nm for nm, _ in c1 if nm == "smsut_colsum" or "wgrad" in nm], c1
        close(f"{scope} gx", res["gx"], t["gx"], 1e-5, fails)
        ref_dgy = t["d_gy"] + (t["u"].double().view(1, -1, 1, 1) if "gb" in res else 0.0)
        close(f"{scope} dL/dgy", res["d_gy"], ref_dgy, 1e-5, fails)
        close(f"{scope} dL/dw", res["d_w"], t["d_w"], 5e-5, fails)
        assert res["d_w"].stride() == wd.stride()
        assert res["d_x"] is None or not bool(res["d_x"].any())
        if "gb" in res:
            # fill(0) + bias_add(u): exact values, exactly
            assert torch.equal(res["d_gy_bias"], ud.view(1, -1, 1, 1).expand_as(gyd)), "d/dgy of the bias term is u broadcast, bit for bit"
    assert ops.layout_copies() == copies
    assert not fails, fails


WGRAD_BWD_CASES = [CONV_CASES[0], CONV_CASES[2]]


@pytest.mark.parametrize("fc", WGRAD_BWD_CASES, ids=case_id)
def test_conv_wgrad_backward(pkg, fc):
    """Conv2dWgradFn.backward: with L = sum(gw * U), dL/dx = dgrad(gy, U) and dL/dgy = conv(x, U)"""
    from smsut_amd import ops, profiling
    family, case = fc
    n, h, w, ci, co, k, s, p, has_b = case
    t = conv_case(case)
    xd = act_dev(t["x"]).requires_grad_(True)
    wd = w_dev(ops, t["w"]).requires_grad_(True)
    bd = t["b"].cuda().requires_grad_(True) if has_b else None
    gyd = act_dev(t["gy"]).requires_grad_(True)
    Ud = w_dev(ops, t["U"])
    res = {}
    copies = ops.layout_copies()
    y = ops.conv2d(xd, wd, bd, s, p)
    (gw,) = torch.autograd.grad(y, wd, gyd, create_graph=True)
    assert gw.stride() == wd.stride()

    def second():
        res["d_x"], res["d_gy"] = torch.autograd.grad((gw * Ud).sum(), (xd, gyd))

    rec = profiling.record_step(second)
    show("second-order pass", rec)
    want_dgrad, want_fwd, _ = family_calls(family, case)
    assert want_dgrad in calls(rec) and want_fwd in calls(rec), calls(rec)
    assert ops.layout_copies() == copies
    fails = []
    close("dL/dx", res["d_x"], t["dx_U"], 1e-5, fails)
    close("dL/dgy", res["d_gy"], t["dgy_U"], 1e-5, fails)
    assert not fails, fails


# ------------------------------------------------------------------------------------------- parts B and C: shared comparison
def compare(tag, rows, scalars):
    """rows: (name, GPU tensor, fp64, fp32 replay, kind of single-op bar); scalars: (name, GPU, fp64).  Everything is printed, then asserted."""
    fails = []
    for name, got, r64, r32, kind in rows:
        d32 = rel_err(r32.numpy(), r64.numpy())
        bar = max(4.0 * d32, R.SINGLE_OP_BARS[kind])
        assert tuple(got.shape) == tuple(r64.shape), (tag, name)
        e = rel_err(got.detach().cpu().numpy(), r64.numpy())
        print(f"{tag} {name}: err {e:.3g}  d32 {d32:.3g}  bar {bar:.3g}")
        if not e < bar:
            fails.append((name, e, bar))
    for name, got, ref in scalars:
        got, ref = float(got), float(ref)
        print(f"{tag} {name}: got {got:.8g} fp64 {ref:.8g} |diff| {abs(got - ref):.3g} bar {1e-6 + 2e-5 * abs(ref):.3g}")
        if not abs(got - ref) <= 1e-6 + 2e-5 * abs(ref):
            fails.append((name, got, ref))
    assert not fails, (tag, fails)


def step_rows(got, r64, r32):
    rows = [("out", got["src"], r64["src"], r32["src"], "out"), ("dydx", got["dydx"], r64["dydx"], r32["dydx"], "dydx"),
            ("d_x_hat", got["d_x_hat"], r64["d_x_hat"], r32["d_x_hat"], "second")]
    assert set(got["grads"]) == set(r64["grads"])
    for k, g in got["grads"].items():
        assert g is not None and r64["grads"][k] is not None, k
        rows.append((k, g, r64["grads"][k], r32["grads"][k], "wgrad"))
    return rows


FIRST_ORDER_ONLY = ("smsut_restail_", "smsut_instnorm_pool_")


def assert_twice_differentiable_forms(rec):
    bad = [n for n, _ in rec if n.startswith(FIRST_ORDER_ONLY) or n.endswith("_fin")]
    assert not bad, bad


# ------------------------------------------------------------------------------------------- part B: one stride-2 BottleBlock
def make_block(ci, co, seed):
    from smsut_amd.network.blocks import BottleBlock
    torch.manual_seed(seed)
    blk = BottleBlock(ci, co, norm_type="instance", act_type="lrelu", stride=2).cuda().train()
    for p in blk.parameters():
        p.data.add_(0.1 * torch.randn_like(p))
    return blk


def gpu_block_step(blk, x, cot=None):
    """the gradient-penalty step on blk(x_hat) as the trainers run it (``cot``: a differentiated cotangent in the place of the ones);
    returns (results, masks of the run, launch record)"""
    from smsut_amd import ops, profiling
    masks, got = {}, {}
    hooks = [blk.bn1.register_forward_hook(lambda m, i, o: masks.__setitem__("bn1", (o.detach() > 0).cpu())),
             blk.register_forward_hook(lambda m, i, o: masks.__setitem__("out", (o.detach() > 0).cpu()))]
    blk.zero_grad(set_to_none=True)
    xh = x.clone().requires_grad_(True)
    c = None if cot is None else cot.clone().requires_grad_(True)

    def step():
        out = blk(xh)
        with ops.input_grads_only():
            (dydx,) = torch.autograd.grad(out, xh, torch.ones_like(out) if c is None else c, retain_graph=True, create_graph=True)
        gp = ops.grad_penalty(dydx)
        (ops.mean_all(out, A_SRC) + B_GP * gp).backward()
        got.update(src=out.detach(), dydx=dydx.detach(), gp=gp.detach())

    try:
        rec = profiling.record_step(step)
    finally:
        for hk in hooks:
            hk.remove()
    got.update(d_x_hat=xh.grad, d_cot=None if c is None else c.grad, grads={k: p.grad for k, p in blk.named_parameters()})
    return got, masks, rec


@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=lambda c: "n%d_%dto%d_%d" % c)
def test_bottleblock_gradient_penalty_pass(pkg, case):
    n, ci, co, h = case
    blk = make_block(ci, co, 100 * n + ci)
    assert (blk.downsample is None) == (ci == co)
    x = act_dev(rnd(n, ci, h, h, seed=21))
    got, masks, rec = gpu_block_step(blk, x)
    show("x_hat pass", rec)
    assert_twice_differentiable_forms(rec)
    pools = [i for nm, i in calls(rec) if nm == "smsut_avgpool2_fwd"]
    assert [n, h, h, ci] in pools, "the shortcut pools x"
    if ci == co:
        assert not [nm for nm, _ in rec if nm.startswith("smsut_conv1x1")], "the identity form has no shortcut conv"
    assert tuple(got["src"].shape) == (n, co, h // 2, h // 2)
    params = {k: p.detach().cpu() for k, p in blk.named_parameters()}
    r64 = R.block_step(x.cpu(), params, masks, A_SRC, B_GP)
    r32 = R.block_step(x.cpu(), params, masks, A_SRC, B_GP, dtype=torch.float32)
    compare("block n%d %d->%d @%d" % case, step_rows(got, r64, r32), [("gp", got["gp"], r64["gp"])])


@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=lambda c: "n%d_%dto%d_%d" % c)
def test_bottleblock_gradient_penalty_pass_with_a_cotangent(pkg, case):
    """Inside the discriminator a block's cotangent is the next layer's data gradient, and the second-order pass hands d loss / d cotangent
    on to that layer.  With the ones of the penalty itself that result is dropped -- and with it everything ``ActBwdFn.backward`` of the
    block's final activation computes -- so this run differentiates a random cotangent too and compares its gradient."""
    n, ci, co, h = case
    blk = make_block(ci, co, 100 * n + ci)
    x = act_dev(rnd(n, ci, h, h, seed=21))
    cot = act_dev(1.0 + 0.5 * rnd(n, co, h // 2, h // 2, seed=22))
    got, masks, rec = gpu_block_step(blk, x, cot)
    assert_twice_differentiable_forms(rec)
    params = {k: p.detach().cpu() for k, p in blk.named_parameters()}
    r64 = R.block_step(x.cpu(), params, masks, A_SRC, B_GP, cot=cot.cpu())
    r32 = R.block_step(x.cpu(), params, masks, A_SRC, B_GP, cot=cot.cpu(), dtype=torch.float32)
    rows = step_rows(got, r64, r32) + [("d_cot", got["d_cot"], r64["d_cot"], r32["d_cot"], "second")]
    compare("block+cot n%d %d->%d @%d" % case, rows, [("gp", got["gp"], r64["gp"])])


@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=lambda c: "n%d_%dto%d_%d" % c)
def test_bottleblock_first_order_pass_refuses_a_double_backward(pkg, case):
    """both forms: a pass through the first-order-only kernels must raise, not return wrong numbers, when it is differentiated twice"""
    from smsut_amd import ops, profiling
    if not ops.IN_ACT_POOL:
        pytest.skip("SMSUT_IN_ACT_POOL switched off in the environment")
    n, ci, co, h = case
    blk = make_block(ci, co, 100 * n + ci)
    xh = act_dev(rnd(n, ci, h, h, seed=21)).requires_grad_(True)
    res = {}

    def fwd():
        with ops.first_order_pass():
            res["out"] = blk(xh)

    rec = profiling.record_step(fwd)
    assert [nm for nm, _ in rec if nm.startswith("smsut_instnorm_pool_")], "the pass took the fused IN + act + pool"
    with pytest.raises(RuntimeError):
        (dydx,) = torch.autograd.grad(res["out"], xh, torch.ones_like(res["out"]), create_graph=True)
        dydx.square().sum().backward()


def test_bottleblock_gradient_penalty_pass_keeps_fp32_operands(pkg):
    """tests/test_f16_gpu.py's header: the twice-differentiated pass keeps fp32 operands under set_conv_dtype("f16")"""
    from smsut_amd import ops
    n, ci, co, h = R.BLOCK_CASES[0]
    blk = make_block(ci, co, 100 * n + ci)
    x = act_dev(rnd(n, ci, h, h, seed=21))
    prev = ops.conv_dtype()
    runs = {}
    try:
        for name in ("f32", "f16"):
            ops.set_conv_dtype(name)
            runs[name] = gpu_block_step(blk, x)
    finally:
        ops.set_conv_dtype(prev)
    names = [nm for nm, _ in runs["f16"][2]]
    assert not [nm for nm in names if "_f16" in nm or "_hs" in nm], names
    assert names == [nm for nm, _ in runs["f32"][2]]
    a, b = runs["f32"][0], runs["f16"][0]
    for k in ("src", "dydx", "gp", "d_x_hat"):
        assert torch.equal(a[k], b[k]), k
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


# ------------------------------------------------------------------------------------------- part C: the discriminator's D step
def test_discriminator_d_step_with_the_capped_block(pkg):
    from smsut_amd import ops, profiling
    from smsut_amd.network.blocks import BottleBlock
    from smsut_amd.network.ugan import Discriminator
    d = R.DISC
    D = Discriminator(d["size"], d["n_modal"], d["width"], max_width=d["max_width"])
    D.load_state_dict(recipe.fill(recipe.disc_shapes(d["size"], d["n_modal"], d["width"], d["max_width"]), 5))
    D.cuda().train()
    blocks = [m for m in D.main if isinstance(m, BottleBlock)]
    assert len(blocks) == 2 and blocks[0].downsample is not None and blocks[1].downsample is None      # 8->16, then the capped 16->16
    assert D.conv_cls.kernel_size == 4 and D.conv_cls.padding == 0
    x, xf, alpha, tgt = (t.cuda() for t in R.disc_inputs(6))
    b = x.shape[0]
    masks_rf, masks_hat = {}, {}
    cur = [masks_rf]
    hooks = [m.register_forward_hook(lambda m_, i, o, name=name: cur[0].__setitem__(name, (o.detach() > 0).cpu()))
             for name, m in D.named_modules() if name == "main.1" or name.endswith(".bn1") or isinstance(m, BottleBlock)]
    assert len(hooks) == 5
    got = {}

    def step():
        src, cls = D(torch.cat([x, xf], 0))
        d_real = ops.mean_all(src[:b], -1.0)
        d_cls = ops.cross_entropy_rows(cls[:b], tgt)
        d_fake = ops.mean_all(src[b:], 1.0)
        x_hat = ops.row_lerp(x, xf, alpha).requires_grad_(True)
        cur[0] = masks_hat
        out_src, out_cls = D(x_hat)
        with ops.input_grads_only():
            (dydx,) = torch.autograd.grad(out_src, x_hat, torch.ones_like(out_src), retain_graph=True, create_graph=True)
        d_gp = ops.grad_penalty(dydx)
        d_loss = d_real + d_fake + 1.0 * d_cls + 10.0 * d_gp
        D.zero_grad(set_to_none=True)
        d_loss.backward()
        got.update(src=out_src.detach(), more=out_cls.detach(), dydx=dydx.detach(), gp=d_gp.detach(), loss=d_loss.detach(),
                   src_rf=src.detach(), cls_rf=cls.detach(), d_real=d_real.detach(), d_fake=d_fake.detach(), d_cls=d_cls.detach(),
                   x_hat=x_hat.detach(), d_x_hat=x_hat.grad)

    try:
        rec = profiling.record_step(step)
    finally:
        for hk in hooks:
            hk.remove()
    got["grads"] = {k: p.grad for k, p in D.named_parameters()}
    show("D step", rec)
    assert_twice_differentiable_forms(rec)
    assert set(masks_rf) == set(masks_hat) == {"main.1", "main.2.bn1", "main.2", "main.3.bn1", "main.3"}
    assert tuple(masks_hat["main.3"].shape) == (b, 16, 4, 4) and tuple(masks_rf["main.3"].shape) == (2 * b, 16, 4, 4)
    # conv_cls: the full-window kernel (generic entry point, K == H == W, pad 0, Cout <= 16), forward, data and weight gradient
    full = [4, 4, 16, 1, 1, 4, 4, 4, 1, 0]
    for nm in ("smsut_conv2d_fwd_generic", "smsut_conv2d_dgrad_generic", "smsut_conv2d_wgrad_generic"):
        assert (nm, [2 * b] + full) in calls(rec), nm
    assert ("smsut_conv2d_fwd_generic", [b] + full) in calls(rec)
    # the capped block's shortcut pools its 16-channel 8x8 input in both passes
    assert ("smsut_avgpool2_fwd", [b, 8, 8, 16]) in calls(rec) and ("smsut_avgpool2_fwd", [2 * b, 8, 8, 16]) in calls(rec)
    params = {k: p.detach().cpu() for k, p in D.named_parameters()}
    args = (x.cpu(), xf.cpu(), got["x_hat"].cpu(), tgt.cpu(), params, masks_rf, masks_hat)
    r64 = R.disc_step(*args)
    r32 = R.disc_step(*args, dtype=torch.float32)
    rows = step_rows(got, r64, r32)
    rows[0] = ("out_src", got["src"], r64["src"], r32["src"], "out")
    rows += [("out_cls", got["more"], r64["more"], r32["more"], "out"),
             ("out_src real|fake", got["src_rf"], r64["src_rf"], r32["src_rf"], "out"),
             ("out_cls real|fake", got["cls_rf"], r64["cls_rf"], r32["cls_rf"], "out")]
    compare("disc", rows, [(k, got[k], r64[k]) for k in ("d_real", "d_fake", "d_cls", "gp", "loss")])
