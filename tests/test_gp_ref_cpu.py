"""Pins tests/gp_ref.py, the fp64 reference of tests/test_gp_pass_gpu.py, without a device:

* with the masks taken from its own pre-activations it IS torch autograd of the ordinary composition (``F.leaky_relu``), to 1e-12, for both
  forms of the stride-2 BottleBlock and the small discriminator: outputs, dydx, the penalty and every second-order gradient;
* the identity form pools its shortcut;
* its fp32 and fp64 replays (same masks) stay within the single-op bars times the number of kernels in the chain, so the measured bars
  of the GPU test, max(4 * that distance, single-op bar), are a few single-op bars and not vacuous.  The distances are printed."""
import pytest
import torch
import torch.nn.functional as F

import gp_ref as R
from conftest import rel_err

A, B = 1.0, 10.0             # loss = A * mean(out) + B * gp, the weights the GPU test uses for the block cases


def plain_block(x, p, pre=""):
    """the block as the reference network writes it: nn-style ops, ordinary LeakyReLU"""
    out = F.conv2d(x, p[pre + "conv1.weight"], None, 1, 1)
    out = F.leaky_relu(F.instance_norm(out, None, None, p[pre + "bn1.weight"], p[pre + "bn1.bias"], True, 0.1, 1e-5), 0.01)
    out = F.avg_pool2d(out, 2)
    out = F.conv2d(out, p[pre + "conv2.weight"], None, 1, 1)
    out = F.instance_norm(out, None, None, p[pre + "bn2.weight"], p[pre + "bn2.bias"], True, 0.1, 1e-5)
    identity = F.avg_pool2d(x, 2)
    if pre + "downsample.0.weight" in p:
        identity = F.conv2d(identity, p[pre + "downsample.0.weight"])
        identity = F.instance_norm(identity, None, None, p[pre + "downsample.1.weight"], p[pre + "downsample.1.bias"], True, 0.1, 1e-5)
    return F.leaky_relu(out + identity, 0.01)


def plain_disc(x, p):
    h = F.leaky_relu(F.conv2d(x, p["main.0.weight"], p["main.0.bias"], 2, 1))
    for i in (2, 3):
        h = plain_block(h, p, f"main.{i}.")
    return F.conv2d(h, p["conv_src.weight"], None, 1, 1), F.conv2d(h, p["conv_cls.weight"]).flatten(1)


def plain_gp(fwd, x_hat, params, a, b, weight=None):
    x = x_hat.double().requires_grad_(True)
    p = {k: v.double().requires_grad_(True) for k, v in params.items()}
    src = fwd(x, p)
    src = src[0] if isinstance(src, tuple) else src
    if weight is None:
        weight = torch.ones(src.size(), dtype=src.dtype)
    dydx = torch.autograd.grad(outputs=src, inputs=x, grad_outputs=weight, retain_graph=True, create_graph=True, only_inputs=True)[0]
    norm = torch.sqrt(torch.sum(dydx.view(dydx.size(0), -1) ** 2, dim=1))
    gp = torch.mean((norm - 1) ** 2)
    (a * src.mean() + b * gp).backward()
    return src.detach(), dydx.detach(), gp.detach(), x.grad, {k: v.grad for k, v in p.items()}


def disc_params(seed):
    from oracle import recipe
    d = R.DISC
    return recipe.fill(recipe.disc_shapes(d["size"], d["n_modal"], d["width"], d["max_width"]), seed)


def assert_same(tag, got, ref, bar=1e-12):
    e = rel_err(got.numpy(), ref.numpy())
    assert got.shape == ref.shape and e < bar, (tag, e)


@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=lambda c: "n%d_%dto%d_%d" % c)
def test_block_reference_is_autograd_of_the_plain_composition(case):
    n, ci, co, h = case
    x, p = R.block_input(n, ci, h, 11), R.block_params(ci, co, 12)
    assert ("downsample.0.weight" in p) == (ci != co)
    got = R.block_step(x, p, {}, A, B)
    src, dydx, gp, gx, grads = plain_gp(plain_block, x, p, A, B)
    assert got["src"].shape == (n, co, h // 2, h // 2)             # the identity form too: its shortcut is pooled
    assert_same("out", got["src"], src)
    assert_same("dydx", got["dydx"], dydx)
    assert_same("gp", got["gp"], gp)
    assert_same("d_x_hat", got["d_x_hat"], gx)
    assert set(got["grads"]) == set(grads)
    for k in grads:
        assert float(grads[k].abs().max()) > 0, k
        assert_same(k, got["grads"][k], grads[k])


@pytest.mark.parametrize("case", R.BLOCK_CASES[1:3], ids=lambda c: "n%d_%dto%d_%d" % c)
def test_block_reference_differentiates_a_cotangent(case):
    """gp_step(cot=...): the cotangent's own gradient, which the final activation's second-order result reaches nothing else but"""
    n, ci, co, h = case
    x, p = R.block_input(n, ci, h, 11), R.block_params(ci, co, 12)
    cot = (1 + 0.5 * R.block_input(n, co, h // 2, 13)).requires_grad_(True)
    got = R.block_step(x, p, {}, A, B, cot=cot)
    src, dydx, gp, gx, grads = plain_gp(plain_block, x, p, A, B, weight=cot)
    assert_same("dydx", got["dydx"], dydx)
    assert_same("d_x_hat", got["d_x_hat"], gx)
    assert float(cot.grad.abs().max()) > 0
    assert_same("d_cot", got["d_cot"], cot.grad)
    for k in grads:
        assert_same(k, got["grads"][k], grads[k])
    assert R.block_step(x, p, {}, A, B)["d_cot"] is None


def test_discriminator_reference_is_autograd_of_the_plain_composition():
    p = disc_params(5)
    assert "main.2.downsample.0.weight" in p and "main.3.downsample.0.weight" not in p and "main.4.conv1.weight" not in p
    assert p["conv_cls.weight"].shape == (4, 16, 4, 4)
    x, xf, alpha, _ = R.disc_inputs(6)
    x_hat = alpha * x + (1 - alpha) * xf
    masks = {}
    got = R.gp_step(lambda xh, q: R.discriminator(xh, q, masks), x_hat, p, A, B)
    assert set(masks) == {"main.1", "main.2.bn1", "main.2", "main.3.bn1", "main.3"}
    src, dydx, gp, gx, grads = plain_gp(plain_disc, x_hat, p, A, B)
    assert got["src"].shape == (3, 1, 4, 4) and got["more"].shape == (3, 4)
    assert_same("out_src", got["src"], src)
    assert_same("out_cls", got["more"], plain_disc(x_hat.double(), {k: v.double() for k, v in p.items()})[1])
    assert_same("dydx", got["dydx"], dydx)
    assert_same("gp", got["gp"], gp)
    assert_same("d_x_hat", got["d_x_hat"], gx)
    for k in grads:
        if k == "conv_cls.weight":
            assert got["grads"][k] is None and grads[k] is None          # the x_hat pass uses out_src only
        else:
            assert_same(k, got["grads"][k], grads[k])


def test_d_step_composes_the_trainers_loss():
    """disc_step against the loss written out with F.leaky_relu: d_real + d_fake + d_cls + 10 gp and its parameter gradients"""
    p = disc_params(5)
    x, xf, alpha, tgt = R.disc_inputs(6)
    x_hat = alpha * x + (1 - alpha) * xf
    got = R.disc_step(x, xf, x_hat, tgt, p, {}, {})
    q = {k: v.double().requires_grad_(True) for k, v in p.items()}
    src, cls = plain_disc(torch.cat([x, xf], 0).double(), q)
    xh = x_hat.double().requires_grad_(True)
    (dydx,) = torch.autograd.grad(plain_disc(xh, q)[0].sum(), xh, create_graph=True)
    gp = ((dydx.flatten(1).norm(dim=1) - 1) ** 2).mean()
    loss = -src[:3].mean() + src[3:].mean() + F.cross_entropy(cls[:3], tgt) + 10 * gp
    loss.backward()
    assert_same("loss", got["loss"], loss.detach())
    assert_same("d_cls", got["d_cls"], F.cross_entropy(cls[:3], tgt).detach())
    assert_same("src_rf", got["src_rf"], src.detach())
    for k in q:
        assert_same(k, got["grads"][k], q[k].grad)


def _distances(tag, r32, r64, n_ops):
    """rel_err(fp32 replay, fp64) of every compared tensor against n_ops single-op bars"""
    rows = [("out", r32["src"], r64["src"], "out"), ("dydx", r32["dydx"], r64["dydx"], "dydx"),
            ("d_x_hat", r32["d_x_hat"], r64["d_x_hat"], "second")]
    rows += [(k, r32["grads"][k], r64["grads"][k], "wgrad") for k in r64["grads"] if r64["grads"][k] is not None]
    worst = 0.0
    for name, a, b, kind in rows:
        d = rel_err(a.numpy(), b.numpy())
        bar = n_ops * R.SINGLE_OP_BARS[kind]
        print(f"{tag} {name}: d32 {d:.3g}  {n_ops} x single-op bar {bar:.3g}")
        assert d < bar, (tag, name, d, bar)
        worst = max(worst, d / R.SINGLE_OP_BARS[kind])
    d = abs(float(r32["gp"]) - float(r64["gp"]))
    print(f"{tag} gp: fp32 {float(r32['gp']):.8g} fp64 {float(r64['gp']):.8g} |diff| {d:.3g}")
    assert d <= n_ops * (1e-6 + 2e-5 * abs(float(r64["gp"])))
    return worst


@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=lambda c: "n%d_%dto%d_%d" % c)
def test_block_fp32_replay_is_within_the_scaled_single_op_bars(case):
    n, ci, co, h = case
    x, p = R.block_input(n, ci, h, 11).float(), {k: v.float() for k, v in R.block_params(ci, co, 12).items()}
    masks = {}
    r64 = R.block_step(x, p, masks, A, B)                          # fills the masks from the fp64 pre-activations
    r32 = R.replay(torch.float32, lambda xx, q: (R.bottle_block(xx, q, R.SLOPE, 2, masks), None), x, p, A, B)
    assert r32["src"].dtype == torch.float32 and r64["src"].dtype == torch.float64
    _distances("block n%d %d->%d @%d" % case, r32, r64, R.BLOCK_OPS[ci != co])


def test_discriminator_fp32_replay_is_within_the_scaled_single_op_bars():
    p = disc_params(5)
    x, xf, alpha, tgt = R.disc_inputs(6)
    x_hat = alpha * x + (1 - alpha) * xf
    m_rf, m_hat = {}, {}
    r64 = R.disc_step(x, xf, x_hat, tgt, p, m_rf, m_hat)
    r32 = R.disc_step(x, xf, x_hat, tgt, p, m_rf, m_hat, dtype=torch.float32)
    _distances("disc", r32, r64, R.disc_ops(p))
