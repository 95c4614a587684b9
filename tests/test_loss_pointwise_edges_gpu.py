"""The loss kernels (``csrc/loss.hip``) and the elementwise / resampling kernels (``csrc/pointwise.hip``) against fp64 on the
CPU, at the shapes where they take another path: a partial block, several blocks with a ragged last one, the capped grid
with its grid-stride loop, both vector widths, the smallest planes, ties, NaN, exact zeros and non-uniform upstream
gradients.  Every reference is computed here in fp64 (plain torch, and ``oracle.smsut_oracle`` where it has the formula).

Bars (the project's own, ``test_coranet_gpu.py`` / ``test_softmax_mse_and_argmax_kernels``):
  * scalars              |got - ref| <= 1e-6 + 2e-5 |ref|
  * float tensors        rel_err < 2e-5
  * pure data movement   torch.equal to the fp32 torch result
Where fp32 itself cannot hold a bar the bound is 4 x the error of the same formula evaluated in fp32 on the CPU; the measured
value stands beside the case (``L2_C1_UNIT``)."""

import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

TENSOR_BAR = 2e-5
SENT = 12345.0
GUARD = 256
EW_CAP_ITEMS = 2048 * 256          # work items of one trip of a capped elementwise grid (ew_grid)


def sized(items):
    """a case is either far below one capped trip or past it by a non-multiple of the block"""
    return items < EW_CAP_ITEMS // 2 or (items > EW_CAP_ITEMS and items % 256 != 0)


@pytest.fixture(scope="module")
def ops():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops as o
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return o


@pytest.fixture(scope="module")
def H():
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    return _hip


def rnd(*shape, seed=0, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape) * scale).float()


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def leaf(t):
    """a device leaf with NHWC memory (4-D) that wants a gradient"""
    t = t.cuda()
    return (cl(t) if t.dim() == 4 else t.contiguous()).requires_grad_(True)


def nchw(rows, n, h, w):
    """rows [n*h*w][C] (the kernels' pixel-major view) as a logical NCHW tensor over that same NHWC memory"""
    return rows.view(n, h, w, -1).permute(0, 3, 1, 2)


def check_scalar(tag, got, ref):
    got, ref = float(got), float(ref)
    bar = 1e-6 + 2e-5 * abs(ref)
    print(f"{tag}: got {got:.9g} ref {ref:.9g} |diff| {abs(got - ref):.3g} bar {bar:.3g}")
    assert abs(got - ref) <= bar, tag


def check_tensor(tag, got, ref, bar=TENSOR_BAR):
    e = rel_err(got.detach().cpu().numpy(), ref.detach().numpy())
    print(f"{tag}: rel_err {e:.3g} bar {bar:.3g}")
    assert e < bar, tag


def poisoned(n_floats):
    """n_floats of NaN (a partial that is read but never written shows) followed by a sentinel guard in the same allocation"""
    buf = torch.full((int(n_floats) + GUARD,), float("nan"), device="cuda")
    buf[int(n_floats):] = SENT
    return buf, buf[int(n_floats):]


def guarded_out(n):
    buf = torch.full((n + GUARD,), SENT, device="cuda")
    return buf, buf[n:]


def untouched(*guards):
    return all(bool((g == SENT).all()) for g in guards)


# ------------------------------------------------------------------------------------------------ 1. reductions
# sum_blocks(n) = min(ceil(n / 2048), 512): one partial block | four blocks, the last ragged | the 512-block cap, where a thread
# makes 8-9 trips of stride 131072
SUM_SIZES = [pytest.param(100, id="sum-partial-block"), pytest.param(3 * 2048 + 77, id="sum-4blocks-ragged"),
             pytest.param(1_100_003, id="sum-cap")]


@pytest.mark.parametrize("wrt", ["only-a", "only-b"])
@pytest.mark.parametrize("n", SUM_SIZES)
def test_l1_mean(ops, n, wrt):
    a, b = rnd(1, 1, 1, n, seed=1), rnd(1, 1, 1, n, seed=2)
    ties = torch.tensor([0, n // 3, n - 1])               # a == b exactly: the gradient is 0 there
    b[..., ties] = a[..., ties]
    a64, b64 = a.double(), b.double()
    r_leaf = (a64 if wrt == "only-a" else b64).requires_grad_(True)
    ref = (a64 - b64).abs().mean()
    (ref * 1.7).backward()
    ad, bd = a.cuda(), b.cuda()
    d_leaf = (ad if wrt == "only-a" else bd).requires_grad_(True)
    out = ops.l1_mean(ad, bd)
    (out * 1.7).backward()
    check_scalar("l1", out.item(), ref.item())
    check_tensor("l1 grad", d_leaf.grad, r_leaf.grad)
    assert bool((d_leaf.grad.cpu().flatten()[ties] == 0).all()), "a tie must get a zero gradient"
    assert (bd if wrt == "only-a" else ad).grad is None


@pytest.mark.parametrize("n", SUM_SIZES)
def test_mean_all(ops, n):
    x = rnd(1, 1, 1, n, seed=3) + 0.5                     # (+0.5: a mean that is not a cancellation to ~0)
    x64 = x.double().requires_grad_(True)
    ref = -x64.mean()
    (ref * 3.0).backward()
    xd = leaf(x)
    out = ops.mean_all(xd, -1.0)
    (out * 3.0).backward()
    check_scalar("mean_all", out.item(), ref.item())
    check_tensor("mean_all grad", xd.grad, x64.grad)


GP_SCALES = (0.1, 1.0, 10.0)                              # three rows of very different norms: a row mix-up shows


def gp_input(n):
    return rnd(3, n, seed=5) * torch.tensor(GP_SCALES).view(3, 1) / float(np.sqrt(n))


def gp_ref(d64):
    return torch.mean((torch.sqrt(torch.sum(d64 ** 2, 1)) - 1) ** 2)


@pytest.mark.parametrize("n", SUM_SIZES)
def test_grad_penalty(ops, n):
    d = gp_input(n)
    d64 = d.double().requires_grad_(True)
    ref = gp_ref(d64)
    (ref * 1.7).backward()
    dd = leaf(d)
    out = ops.grad_penalty(dd)
    (out * 1.7).backward()
    check_scalar("gp", out.item(), ref.item())
    check_tensor("gp grad", dd.grad, d64.grad)


# P = 71 * 15493 = 1100003 pixels: the forward's 512-block cap and the backward's capped grid (3 trips), P % 256 != 0
@pytest.mark.parametrize("n,c,h,w", [pytest.param(1, 2, 71, 15493, id="smse-cap-P1100003-C2"), pytest.param(3, 32, 10, 10, id="smse-P300-C32"),
                                     pytest.param(3, 1, 10, 10, id="smse-P300-C1")])
def test_softmax_mse(ops, n, c, h, w):
    a, b = nchw(rnd(n * h * w, c, seed=6, scale=2.0), n, h, w), nchw(rnd(n * h * w, c, seed=7, scale=2.0), n, h, w)
    a64 = a.double().requires_grad_(True)
    ref = torch.mean((torch.softmax(a64, 1) - torch.softmax(b.double(), 1)) ** 2)
    (ref * 1.7).backward()
    ad = a.cuda().requires_grad_(True)
    out = ops.softmax_mse(ad, b.cuda())
    (out * 1.7).backward()
    check_scalar("softmax_mse", out.item(), ref.item())   # (C = 1: both softmaxes are 1, loss and gradient exactly 0)
    check_tensor("softmax_mse grad", ad.grad, a64.grad)


@pytest.mark.parametrize("n", SUM_SIZES)
def test_sum_workspace_guards(ops, H, n):
    """smsut_sum / smsut_l1_fwd / smsut_gp_fwd with a workspace of exactly smsut_sum_ws floats: every partial that is read was
    written (the workspace starts as NaN), nothing lands behind it, and the value is the one the op returns."""
    s = H.stream_ptr()
    x = (rnd(n, seed=3) + 0.5).cuda()
    ws, g = poisoned(H.call("smsut_sum_ws", n, 1))
    out, og = guarded_out(1)
    H.call("smsut_sum", x, out, ws, n, 1.0 / n, s)
    check_scalar("sum", out[0].item(), x.cpu().double().mean().item())
    assert untouched(g, og) and out[0].item() == ops.mean_all(x, 1.0).item()

    a, b = rnd(1, 1, 1, n, seed=1).cuda(), rnd(1, 1, 1, n, seed=2).cuda()
    ws, g = poisoned(H.call("smsut_sum_ws", n, 1))
    out, og = guarded_out(1)
    H.call("smsut_l1_fwd", a, b, out, ws, n, s)
    check_scalar("l1", out[0].item(), (a.cpu().double() - b.cpu().double()).abs().mean().item())
    assert untouched(g, og) and out[0].item() == ops.l1_mean(a, b).item()

    d = gp_input(n).cuda()
    ws, g = poisoned(H.call("smsut_sum_ws", n, 3))        # rows x blocks partials
    out, og = guarded_out(1)
    norms, ng = guarded_out(3)
    H.call("smsut_gp_fwd", d, out, norms, ws, 3, n, s)
    check_scalar("gp", out[0].item(), gp_ref(d.cpu().double()).item())
    check_tensor("gp norms", norms[:3], d.cpu().double().norm(dim=1))
    assert untouched(g, og, ng) and out[0].item() == ops.grad_penalty(d).item()


# ------------------------------------------------------------------------------------------------ 2. Dice + CE
# pix_blocks(HW) = min(ceil(HW / 1024), 64): 10x10 one partial block | 56x56 = 3*1024 + 64: four blocks per image, the last with
# 64 live lanes | 300x300: the 64-block cap, 6 forward and 2 backward trips.  C 2-5 compile-time, 6 / 17 / 32 (= MAXC) runtime.
DICE_HW = {"dice-1block-partial": (10, 10), "dice-4blocks-ragged": (56, 56), "dice-64block-cap": (300, 300)}
DICE_CASES = [pytest.param(k, c, id=f"{k}-C{c}") for k in DICE_HW for c in (2, 3, 4, 5, 6, 17, 32)
              if k != "dice-64block-cap" or c in (2, 5, 32)]


@functools.lru_cache(maxsize=None)
def dice_inputs(h, w, c, scale):
    """N = 3; image 0 is all background and (C >= 3) class C-1 occurs nowhere: count = 0 terms in both Dice groupings.  With two
    classes the single foreground class stays in images 1 and 2."""
    lg = nchw(rnd(3 * h * w, c, seed=11 + c, scale=float(scale)), 3, h, w)
    lb = torch.from_numpy(np.random.RandomState(12 + c).randint(0, c - 1 if c >= 3 else c, size=(3, h, w)).astype(np.int64))
    lb[0] = 0
    return lg, lb


@pytest.mark.parametrize("scale", [2, 15], ids=["logits2", "logits15-saturated"])
@pytest.mark.parametrize("batch_dice", [True, False], ids=["batch-dice", "sample-dice"])
@pytest.mark.parametrize("hw,c", DICE_CASES)
def test_dice_ce(ops, hw, c, batch_dice, scale):
    from oracle import smsut_oracle as O
    h, w = DICE_HW[hw]
    lg, lb = dice_inputs(h, w, c, scale)
    lg64 = lg.double().requires_grad_(True)
    ref = O.dice_ce(lg64, lb, 0.3, 0.7, batch_dice)       # (CE weight, Dice weight): unequal, a swap shows
    (ref * 1.7).backward()
    ld = lg.cuda().requires_grad_(True)
    out = ops.dice_ce(ld, lb.cuda(), 0.3, 0.7, batch_dice)
    (out * 1.7).backward()
    check_scalar("dice_ce", out.item(), ref.item())
    check_tensor("dice_ce grad", ld.grad, lg64.grad)


@pytest.mark.parametrize("batch_dice", [True, False], ids=["G1", "GN"])
@pytest.mark.parametrize("hw,c", [pytest.param("dice-1block-partial", 17, id="dice-1block-partial-C17"),
                                  pytest.param("dice-4blocks-ragged", 3, id="dice-4blocks-ragged-C3"),
                                  pytest.param("dice-64block-cap", 5, id="dice-64block-cap-C5")])
def test_dice_stats_workspace_guards(ops, H, hw, c, batch_dice):
    """smsut_dicece_stats with exactly smsut_dicece_ws floats of NaN: the N * pix_blocks partial slabs the reduce reads are all
    written, nothing lands behind them, and {tp, sum_p, count} / the CE sum agree with fp64."""
    h, w = DICE_HW[hw]
    lg, lb = dice_inputs(h, w, c, 2)
    n, g = 3, (1 if batch_dice else 3)
    ld, lbd = lg.cuda(), lb.cuda()
    ws, wg = poisoned(H.call("smsut_dicece_ws", n, h * w, c, g))
    stats, sg = guarded_out(g * c * 3)
    ce, cg = guarded_out(1)
    H.call("smsut_dicece_stats", ld, lbd, stats, ce, ws, n, h * w, c, g, H.stream_ptr())
    p = torch.softmax(lg.double(), 1)
    oh = torch.zeros_like(p).scatter_(1, lb.unsqueeze(1), 1.0)
    dims = (0, 2, 3) if batch_dice else (2, 3)
    ref = torch.stack([(p * oh).sum(dims), p.sum(dims), oh.sum(dims)], -1).reshape(g, c, 3)
    for k, what in enumerate(("tp", "sum_p", "count")):
        check_tensor(f"dice stats {what}", stats[:g * c * 3].view(g, c, 3)[..., k], ref[..., k])
    check_scalar("ce sum", ce[0].item(), F.cross_entropy(lg.double(), lb, reduction="sum").item())
    assert untouched(wg, sg, cg)
    st2, ce2 = ops.dice_ce_stats(ld, lbd, batch_dice)
    assert torch.equal(st2.flatten(), stats[:g * c * 3]) and torch.equal(ce2, ce[:1])


# ------------------------------------------------------------------------------------------------ 3. rows, patches, argmax
# 300 rows: the single forward block loops (256 + 44), the backward takes two blocks
@pytest.mark.parametrize("b,c", [pytest.param(16, 4, id="ce-rows16"), pytest.param(300, 7, id="ce-rows300-fwd-loop-2bwd-blocks"),
                                 pytest.param(1, 1, id="ce-rows1-C1")])
def test_cross_entropy_rows(ops, b, c):
    z = rnd(b, c, seed=21, scale=2.0)
    t = torch.from_numpy(np.random.RandomState(22).permutation(b) % c).long()     # every class occurs as a target
    z64 = z.double().requires_grad_(True)
    ref = F.cross_entropy(z64, t)
    (ref * 1.7).backward()
    zd = leaf(z)
    out = ops.cross_entropy_rows(zd, t.cuda())
    (out * 1.7).backward()
    check_scalar("ce_rows", out.item(), ref.item())
    check_tensor("ce_rows grad", zd.grad, z64.grad)


# C = 1 at unit scale: gx = gy/e - x (gy x)/(n e^2) with e = n + 1e-7 is gy * 1e-7 / e^2, the difference of two terms that agree
# to seven digits, so fp32 keeps none (torch's own fp32 gradient does no better).  Measured: the kernel's formula evaluated in
# fp32 on the CPU, both with the last multiply-subtract as two roundings and as one fma (the compiler may contract it), against
# the fp64 gradient, larger of the two per row count; the bound is 4 x that.   rows: (measured, bound)
L2_C1_UNIT = {1: (1.97e-1, 7.88e-1), 5: (6.78e-3, 2.72e-2), 64: (1.06e-2, 4.24e-2)}


@pytest.mark.parametrize("c", [1, 32, 64, 65, 256, 300])   # one lane | half a wave | a full wave | a second trip | the trainers' 256 | ragged
@pytest.mark.parametrize("rows", [1, 5, 64])               # four rows per block: a partial block | two blocks, one row in the last | full
def test_l2_normalize(ops, rows, c):
    from oracle import smsut_oracle as O
    gy = rnd(rows, c, seed=24)
    for what, scale in (("unit", 1.0),) + ((("eps-scale", 1e-7),) if c == 1 else ()):
        # (C = 1 also at |x| ~ 1e-7, where the 1e-7 of the denominator matters and the gradient is well conditioned)
        x = rnd(rows, c, seed=23, scale=scale)
        x64 = x.double().requires_grad_(True)
        ref = O.l2_normalize(x64)
        ref.backward(gy.double())
        xd = leaf(x)
        out = ops.l2_normalize(xd)
        out.backward(gy.cuda())
        check_tensor(f"l2 fwd {what}", out, ref.detach())
        check_tensor(f"l2 bwd {what}", xd.grad, x64.grad, L2_C1_UNIT[rows][1] if c == 1 and what == "unit" else TENSOR_BAR)


def test_l2_normalize_zero_row(ops):
    """The kernel's stated behaviour for a zero row (torch's gradient is NaN there): y = 0, gx = gy / 1e-7."""
    x = rnd(5, 65, seed=23)
    x[1] = 0.0
    gy = rnd(5, 65, seed=24)
    xd = leaf(x)
    out = ops.l2_normalize(xd)
    out.backward(gy.cuda())
    assert bool((out[1] == 0).all()) and bool(torch.isfinite(xd.grad).all())
    check_tensor("l2 zero row", xd.grad[1], gy[1].double() / 1e-7)
    x64 = x.double()[[0, 2, 3, 4]].requires_grad_(True)
    (x64 / (x64.norm(dim=1, keepdim=True) + 1e-7)).backward(gy.double()[[0, 2, 3, 4]])
    check_tensor("l2 other rows", xd.grad[[0, 2, 3, 4]], x64.grad)


# np + 1 logits and dim both walk a 256-thread block: 65 / 256 (the trainers' shape), 301 / 70 (a second trip over j), 2 / 8, 33 / 32
@pytest.mark.parametrize("rows,npatch,dim", [pytest.param(128, 64, 256, id="nce-np65-dim256"), pytest.param(600, 300, 70, id="nce-np301-dim70"),
                                             pytest.param(3, 1, 8, id="nce-np2-dim8"), pytest.param(64, 32, 32, id="nce-np33-dim32")])
def test_patch_nce_weighted_rows(ops, H, rows, npatch, dim):
    from oracle import smsut_oracle as O
    q, k = rnd(rows, dim, seed=31), rnd(rows, dim, seed=32)
    wt = torch.from_numpy(np.random.RandomState(33).uniform(0.5, 2.0, rows)).float()      # one upstream gradient per row
    q64 = q.double().requires_grad_(True)
    ref = O.patch_nce(O.l2_normalize(q64), O.l2_normalize(k.double()), rows // npatch)
    (ref * wt.double()).sum().backward()
    qd = leaf(q)
    qn, kn = ops.l2_normalize(qd), ops.l2_normalize(k.cuda())
    out = ops.patch_nce(qn, kn, npatch)
    (out * wt.cuda()).sum().backward()
    check_tensor("nce loss", out, ref.detach())
    check_tensor("nce grad", qd.grad, q64.grad)
    loss = torch.empty(rows, device="cuda")
    probs = torch.empty(rows, npatch + 1, device="cuda")
    H.call("smsut_patchnce_fwd", qn.detach(), kn, loss, probs, rows, npatch, dim, 0.07, H.stream_ptr())
    assert torch.equal(loss, out.detach())
    assert float((probs.double().sum(1) - 1).abs().max()) < 1e-6, "the saved softmax rows must sum to 1"


@pytest.mark.parametrize("p", [1, 17, 63], ids=["P1", "P17", "P63-all"])
@pytest.mark.parametrize("c", [5, 8])
def test_gather_patches_on_dirty_memory(ops, c, p):
    b, h, w = 3, 7, 9
    feat = rnd(b, c, h, w, seed=41)
    ids = torch.from_numpy(np.random.RandomState(42).permutation(h * w)[:p].copy()).long()      # unsorted, unique
    gg = rnd(b * p, c, seed=43)
    ref = feat.permute(0, 2, 3, 1).flatten(1, 2)[:, ids, :].flatten(0, 1)
    fd = leaf(feat)
    out = ops.gather_patches(fd, ids.cuda())
    assert torch.equal(out.detach().cpu(), ref)
    ggd = gg.cuda()
    dirty = [torch.full((b * c * h * w,), 1e10, device="cuda") for _ in range(64)]    # the gradient's next home: a missing zero-fill shows
    torch.cuda.synchronize()
    del dirty
    out.backward(ggd)
    want = torch.zeros(b, h * w, c)
    want[:, ids, :] = gg.view(b, p, c)
    got = fd.grad.cpu().permute(0, 2, 3, 1).flatten(1, 2)
    assert torch.equal(got, want), "un-sampled rows exactly 0, sampled rows the upstream rows bit for bit"


@pytest.mark.parametrize("c", [1, 2, 5, 32])
def test_argmax_channels_gridstride(ops, c):
    p = 600_000                                            # > 2048 * 256 pixels: the second grid-stride trip
    z = nchw(torch.from_numpy(np.random.RandomState(51).randint(-3, 4, size=(p, c))).float(), 1, 600, 1000)    # many equal maxima
    assert torch.equal(ops.argmax_channels(z.cuda()).cpu(), torch.argmax(z, 1))


def test_argmax_channels_nan(ops):
    nan = float("nan")
    rows = torch.tensor([[nan, 1., 2., 3., 4.], [0., 1., nan, 3., 4.], [0., 1., 2., 3., nan], [0., nan, 5., nan, 4.],
                         [nan, nan, nan, nan, nan], [4., 4., 1., 4., 0.], [0., 7., 7., nan, 7.], [-1., -2., -3., -4., -5.]])
    z = nchw(rows, 1, 2, 4)
    assert torch.equal(ops.argmax_channels(z.cuda()).cpu(), torch.argmax(z, 1))      # the first NaN, else the first maximum


# ------------------------------------------------------------------------------------------------ 4. elementwise / resampling
# "gridstride" cases: more than 2048 * 256 work items (float4s where the kernel vectorises) by a non-multiple of 256
EW_SHAPES = [pytest.param((1, 1, 5, 7), id="35-elements"), pytest.param((1, 1, 1451, 1451), id="1451x1451-gridstride-scalar-tail")]


def with_zeros(t):
    t = t.clone()
    t.view(-1)[::5] = 0.0                                  # exact zeros: the mask at y == 0 is `slope`
    return t


@pytest.mark.parametrize("slope", [0.0, 0.01])
@pytest.mark.parametrize("with_b", [True, False], ids=["add_act", "leaky_relu"])
@pytest.mark.parametrize("shape", EW_SHAPES)
def test_add_act(ops, shape, with_b, slope):
    assert sized(int(np.prod(shape)) // 4) and np.prod(shape) % 4          # (float4 work items, and a scalar tail)
    a, gy = rnd(*shape, seed=61), rnd(*shape, seed=63)
    if with_b:
        b = rnd(*shape, seed=62)
        b.view(-1)[::5] = -a.view(-1)[::5]                 # a + b == 0 exactly
        b64 = b.double().requires_grad_(True)
        bd = leaf(b)
    else:
        a = with_zeros(a)
    a64 = a.double().requires_grad_(True)
    ref = F.leaky_relu(a64 + b64 if with_b else a64, slope)
    ref.backward(gy.double())
    ad = leaf(a)
    out = ops.add_act(ad, bd, slope) if with_b else ops.leaky_relu(ad, slope)
    out.backward(gy.cuda())
    check_tensor("add_act fwd", out, ref.detach())
    check_tensor("add_act grad a", ad.grad, a64.grad)
    zero = (out.detach().cpu().flatten()[::5] == 0)
    assert bool(zero.all()) and torch.equal(ad.grad.cpu().flatten()[::5], gy.flatten()[::5] * slope)
    if with_b:
        check_tensor("add_act grad b", bd.grad, b64.grad)


@pytest.mark.parametrize("shape", EW_SHAPES)
def test_tanh(ops, shape):
    x, gy = rnd(*shape, seed=64, scale=2.0), rnd(*shape, seed=65)
    x64 = x.double().requires_grad_(True)
    ref = torch.tanh(x64)
    ref.backward(gy.double())
    xd = leaf(x)
    out = ops.tanh(xd)
    out.backward(gy.cuda())
    check_tensor("tanh fwd", out, ref.detach())
    check_tensor("tanh grad", xd.grad, x64.grad)


@pytest.mark.parametrize("shape", [pytest.param((3, 1, 4, 5), id="60-elements"), pytest.param((3, 1, 419, 419), id="3x419x419-gridstride")])
def test_row_lerp(ops, shape):
    assert sized(int(np.prod(shape)))
    a, b = rnd(*shape, seed=66), rnd(*shape, seed=67)
    al = torch.tensor([0.25, 0.9, 0.0]).view(3, 1, 1, 1)
    out = ops.row_lerp(a.cuda(), b.cuda(), al.cuda())
    check_tensor("row_lerp", out, al.double() * a.double() + (1 - al.double()) * b.double())


@pytest.mark.parametrize("n,h,w", [pytest.param(2, 4, 5, id="200-elements"), pytest.param(3, 191, 193, id="3x191x193x5-gridstride")])
def test_modal_planes(ops, n, h, w):
    assert sized(n * h * w * 5)
    x, m = rnd(n, 1, h, w, seed=68), rnd(n, 4, seed=69)
    gy = cl(rnd(n, 5, h, w, seed=70))
    xd = leaf(x)
    out = ops.modal_planes(xd, m.cuda())
    out.backward(gy.cuda())
    assert torch.equal(out.detach().cpu(), torch.cat([x, m.view(n, 4, 1, 1).repeat(1, 1, h, w)], 1))
    assert torch.equal(xd.grad.cpu(), gy[:, :1])


# pools: work items = N * (H/2) * (W/2) * C / VEC (VEC = 4 when C % 4 == 0)
POOL_SHAPES = [pytest.param(3, c, 2, 2, id=f"C{c}-2x2-smallest") for c in (1, 6, 8)] + \
              [pytest.param(3, c, 6, 10, id=f"C{c}-6x10") for c in (1, 6, 8)] + \
              [pytest.param(3, 1, 838, 842, id="C1-838x842-gridstride-vec1"), pytest.param(3, 8, 594, 598, id="C8-594x598-gridstride-vec4")]


def _pool_items(n, c, h, w):
    return n * (h // 2) * (w // 2) * c // (4 if c % 4 == 0 else 1)


@pytest.mark.parametrize("n,c,h,w", POOL_SHAPES)
def test_avg_pool2(ops, n, c, h, w):
    assert sized(_pool_items(n, c, h, w))
    x, gy = rnd(n, c, h, w, seed=71), rnd(n, c, h // 2, w // 2, seed=72)
    x64 = x.double().requires_grad_(True)
    ref = F.avg_pool2d(x64, 2)
    ref.backward(gy.double())
    xd = leaf(x)
    out = ops.avg_pool2(xd)
    out.backward(cl(gy.cuda()))
    check_tensor("avg fwd", out, ref.detach())
    check_tensor("avg grad", xd.grad, x64.grad)


@pytest.mark.parametrize("skip", [False, True], ids=["max_pool2", "max_pool2_skip"])
@pytest.mark.parametrize("n,c,h,w", POOL_SHAPES)
def test_max_pool2(ops, n, c, h, w, skip):
    x, gy, gs = rnd(n, c, h, w, seed=73), rnd(n, c, h // 2, w // 2, seed=74), rnd(n, c, h, w, seed=75)
    x64 = x.double().requires_grad_(True)
    F.max_pool2d(x64, 2, 2).backward(gy.double())
    want = x64.grad + gs.double() if skip else x64.grad
    xd = leaf(x)
    if skip:
        out, sk = ops.max_pool2_skip(xd)
        torch.autograd.backward([out, sk], [cl(gy.cuda()), cl(gs.cuda())])
        assert torch.equal(sk.detach().cpu(), x)
    else:
        out = ops.max_pool2(xd)
        out.backward(cl(gy.cuda()))
    assert torch.equal(out.detach().cpu(), F.max_pool2d(x, 2, 2))
    check_tensor("max grad", xd.grad, want)


def _windows(c, wins):
    """one 2x2 window per entry of `wins` (four values in scan order), side by side, the same in every channel: [1, c, 2, 2 * len]"""
    t = torch.tensor(wins, dtype=torch.float32).view(-1, 2, 2)           # [win][row][col]
    return t.permute(1, 0, 2).reshape(1, 1, 2, -1).repeat(1, c, 1, 1).contiguous()


@pytest.mark.parametrize("c", [1, 4], ids=["vec1", "vec4"])
def test_max_pool2_ties(ops, c):
    """All ties (a constant tensor) and a tie at each window position against each earlier one: the first in scan order wins."""
    wins = [[9. if k in (i, j) else float(k) for k in range(4)] for j in range(4) for i in range(j)]
    for x in (_windows(c, wins), torch.full((2, c, 4, 6), 3.0)):
        gy = rnd(x.shape[0], c, x.shape[2] // 2, x.shape[3] // 2, seed=76)
        xr = x.clone().requires_grad_(True)
        ref = F.max_pool2d(xr, 2, 2)
        ref.backward(gy)
        xd = leaf(x)
        out = ops.max_pool2(xd)
        out.backward(cl(gy.cuda()))
        assert torch.equal(out.detach().cpu(), ref.detach()) and torch.equal(xd.grad.cpu(), xr.grad)
    rest = xd.grad.cpu().clone()                           # the constant tensor: everything goes to the window's first element
    assert torch.equal(rest[:, :, ::2, ::2], gy)
    rest[:, :, ::2, ::2] = 0
    assert not bool(rest.any())


@pytest.mark.parametrize("c", [1, 4], ids=["vec1", "vec4"])
def test_max_pool2_nan(ops, c):
    """NaN propagates to the output and the LAST NaN in scan order takes the gradient -- torch's CPU result on the same input."""
    nan = float("nan")
    wins = [[nan, 1, 2, 3], [0, nan, 2, 3], [0, 1, nan, 3], [0, 1, 2, nan], [nan, 1, nan, 3], [nan, nan, 2, 9], [0, nan, 5, nan],
            [nan, nan, nan, nan], [nan, 7, 7, 1]]
    x = _windows(c, wins)
    gy = rnd(1, c, 1, len(wins), seed=77)
    xr = x.clone().requires_grad_(True)
    ref = F.max_pool2d(xr, 2, 2)
    ref.backward(gy)
    xd = leaf(x)
    out = ops.max_pool2(xd)
    out.backward(cl(gy.cuda()))
    got = out.detach().cpu()
    assert bool(torch.isnan(ref).all()) and torch.equal(torch.isnan(got), torch.isnan(ref.detach()))
    assert torch.equal(xd.grad.cpu(), xr.grad)


BIL_SHAPES = [pytest.param(3, c, h, w, id=f"C{c}-{h}x{w}") for c in (1, 6, 8) for h, w in ((1, 1), (1, 5), (5, 1), (3, 5))] + \
             [pytest.param(3, 1, 419, 421, id="C1-419x421-gridstride-vec1"), pytest.param(3, 8, 297, 299, id="C8-297x299-gridstride-vec4")]


@pytest.mark.parametrize("n,c,h,w", BIL_SHAPES)
def test_bilinear_up2(ops, n, c, h, w):
    items = n * h * w * c // (4 if c % 4 == 0 else 1)      # of the backward; the forward has four times as many
    assert sized(items)
    x, gy = rnd(n, c, h, w, seed=78), rnd(n, c, 2 * h, 2 * w, seed=79)
    x64 = x.double().requires_grad_(True)
    ref = F.interpolate(x64, scale_factor=2, mode="bilinear", align_corners=False)
    ref.backward(gy.double())
    xd = leaf(x)
    out = ops.bilinear_up2(xd)
    out.backward(cl(gy.cuda()))
    check_tensor("bilinear fwd", out, ref.detach())
    check_tensor("bilinear grad", xd.grad, x64.grad)


BLUR_SHAPES = [pytest.param(3, c, h, w, id=f"C{c}-{h}x{w}") for c in (1, 3, 8) for h, w in ((2, 2), (7, 10), (16, 16))] + \
              [pytest.param(3, 1, 838, 842, id="C1-838x842-gridstride")]


@pytest.mark.parametrize("n,c,h,w", BLUR_SHAPES)
def test_blur_down2(ops, n, c, h, w):
    x = rnd(n, c, h, w, seed=80)
    x64 = x.double().requires_grad_(True)
    f = torch.tensor([1., 2., 1.], dtype=torch.float64)
    k = (f[:, None] * f[None, :] / 16).view(1, 1, 3, 3).repeat(c, 1, 1, 1)
    ref = F.conv2d(F.pad(x64, (1, 1, 1, 1), mode="reflect"), k, stride=2, groups=c)
    assert sized(ref.numel())
    gy = rnd(*ref.shape, seed=81)
    ref.backward(gy.double())
    xd = leaf(x)
    out = ops.blur_down2(xd)
    out.backward(cl(gy.cuda()))
    check_tensor("blur fwd", out, ref.detach())
    check_tensor("blur grad", xd.grad, x64.grad)


# (id, mode, H, W, (left, right, top, bottom))
PAD_CASES = [(f"{m}-pad-size-1", m, 4, 5, (4, 4, 3, 3)) for m in ("zero", "reflect", "replicate")] + \
            [("replicate-pad-gt-size", "replicate", 3, 4, (6, 5, 4, 7))] + \
            [(f"{m}-crop+pad", m, 5, 6, (-1, 2, 3, -2)) for m in ("zero", "reflect", "replicate")]


def _pad_check(ops, n, c, h, w, mode, pads):
    x = rnd(n, c, h, w, seed=82)
    tmode = "constant" if mode == "zero" else mode
    x64 = x.double().requires_grad_(True)
    ref = F.pad(x64, pads, mode=tmode)
    gy = rnd(*ref.shape, seed=83)
    ref.backward(gy.double())
    xd = leaf(x)
    out = ops.pad2d(xd, pads, mode)
    out.backward(cl(gy.cuda()))
    assert torch.equal(out.detach().cpu(), F.pad(x, pads, mode=tmode))
    check_tensor("pad grad", xd.grad, x64.grad)
    return ref.numel()


@pytest.mark.parametrize("c", [1, 4])
@pytest.mark.parametrize("name,mode,h,w,pads", [pytest.param(*p, id=p[0]) for p in PAD_CASES])
def test_pad2d(ops, name, mode, h, w, pads, c):
    _pad_check(ops, 2, c, h, w, mode, pads)


def test_pad2d_small_and_gridstride(ops):
    assert _pad_check(ops, 1, 1, 5, 6, "reflect", (1, 2, 2, 1)) < 256
    big = _pad_check(ops, 3, 1, 419, 421, "reflect", (1, 1, 1, 1))        # forward and backward both past one capped trip
    assert big > EW_CAP_ITEMS and sized(big) and 3 * 419 * 421 > EW_CAP_ITEMS and sized(3 * 419 * 421)


# concat2 (both channel counts multiples of 4, one float4 per lane) | two smsut_copy_channels on its scalar path
CONCAT_CASES = [pytest.param(2, 3, 5, ca, cb, id=f"concat-{ca}+{cb}-{'concat2' if ca % 4 == 0 and cb % 4 == 0 else 'scalar'}")
                for ca, cb in ((4, 8), (8, 4), (16, 16), (4, 5), (3, 8))] + \
               [pytest.param(3, 241, 243, 4, 8, id="concat-4+8-concat2-gridstride"), pytest.param(3, 241, 243, 4, 5, id="concat-4+5-scalar-gridstride")]


@pytest.mark.parametrize("grads", ["concat-both", "concat-only-a", "concat-only-b"])
@pytest.mark.parametrize("n,h,w,ca,cb", CONCAT_CASES)
def test_concat_channels(ops, n, h, w, ca, cb, grads):
    a, b = cl(rnd(n, ca, h, w, seed=84)), cl(rnd(n, cb, h, w, seed=85))
    gy = cl(rnd(n, ca + cb, h, w, seed=86))
    ad, bd = a.cuda(), b.cuda()
    if grads != "concat-only-b":
        ad.requires_grad_(True)
    if grads != "concat-only-a":
        bd.requires_grad_(True)
    out = ops.concat_channels(ad, bd)
    out.backward(gy.cuda())
    assert torch.equal(out.detach().cpu(), torch.cat([a, b], 1))
    for t, want in ((ad, gy[:, :ca]), (bd, gy[:, ca:])):
        if t.requires_grad:
            assert torch.equal(t.grad.cpu(), want)
        else:
            assert t.grad is None                          # (that half's pointer is null in the split kernel)


@pytest.mark.parametrize("p", [pytest.param(37, id="P37"), pytest.param(600_001, id="P600001-gridstride")])
@pytest.mark.parametrize("cs,so,cd,do,cc", [pytest.param(16, 0, 12, 0, 4, id="copy-vec-off0-0"), pytest.param(16, 4, 12, 8, 4, id="copy-vec-off4-8"),
                                            pytest.param(16, 8, 12, 4, 8, id="copy-vec-off8-4"), pytest.param(16, 1, 12, 6, 4, id="copy-scalar-off1-6"),
                                            pytest.param(16, 6, 12, 1, 8, id="copy-scalar-off6-1"), pytest.param(9, 6, 7, 1, 3, id="copy-scalar-odd-widths")])
def test_copy_channels_offsets(H, p, cs, so, cd, do, cc):
    """smsut_copy_channels itself: the slice arrives, every other channel of the destination and the guard behind it keep the sentinel"""
    src = rnd(p, cs, seed=87)
    buf, guard = guarded_out(p * cd)
    H.call("smsut_copy_channels", src.cuda(), cs, so, buf, cd, do, cc, p, H.stream_ptr())
    want = torch.full((p, cd), SENT)
    want[:, do:do + cc] = src[:, so:so + cc]
    assert torch.equal(buf[:p * cd].view(p, cd).cpu(), want) and untouched(guard)


# ------------------------------------------------------------------------------------------------ 5. the two linear closures
@pytest.mark.parametrize("gp_pass", [True, False], ids=["input_grads_only", "plain"])
@pytest.mark.parametrize("s", [0.2, 0.0])
@pytest.mark.parametrize("c", [6, 8], ids=["C6-vec1", "C8-vec4"])
def test_act_avgpool_double_backward(ops, c, s, gp_pass):
    """ActBwdFn / AvgPool2BwdFn as the WGAN-GP pass differentiates them: gx = d(avg_pool2(lrelu(x)))/dx . gy, then d(gx . v)/dgy.
    Both are linear in gy with a piecewise-constant mask, so nothing of second order reaches x."""
    x, gy, v = rnd(2, c, 8, 12, seed=91), rnd(2, c, 4, 6, seed=92), rnd(2, c, 8, 12, seed=93)
    x64, gy64 = x.double().requires_grad_(True), gy.double().requires_grad_(True)
    (r_gx,) = torch.autograd.grad(F.avg_pool2d(F.leaky_relu(x64, s), 2), x64, gy64, create_graph=True)
    r_ggy, r_gxx = torch.autograd.grad((r_gx * v.double()).sum(), [gy64, x64], allow_unused=True)
    assert r_gxx is None or not bool(r_gxx.any())
    with (ops.input_grads_only() if gp_pass else contextlib.nullcontext()):
        xd, gyd = leaf(x), leaf(gy)
        (d_gx,) = torch.autograd.grad(ops.avg_pool2(ops.leaky_relu(xd, s)), xd, gyd, create_graph=True)
        d_ggy, d_gxx = torch.autograd.grad((d_gx * cl(v.cuda())).sum(), [gyd, xd], allow_unused=True)
    check_tensor("first order gx", d_gx, r_gx.detach())
    check_tensor("second order d/dgy", d_ggy, r_ggy)
    assert d_gxx is None or not bool(d_gxx.any())
