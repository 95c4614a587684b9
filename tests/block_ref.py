"""fp64 reference of the fused BasicBlock (``ops.BasicBlockFn``; tests/test_block_fp64_gpu.py, pinned to torch autograd of the ordinary
``F.leaky_relu`` / ``F.instance_norm`` / ``F.conv2d`` / ``F.max_pool2d`` composition by tests/test_block_ref_cpu.py): the reference's
``network/blocks.py:53-80`` restated in functional torch on the CPU, for a plain input, a ``cat([xa, xb], 1)`` input, a conv or an
identity shortcut and an optional ``max_pool2d(out, 2)`` second output.  Tensors are logical NCHW / OIHW.

No discrete event is left to rounding.  Both activations go through ``gp_ref.act`` with a GIVEN mask (sites "act1" and "out"), and the
inputs are made so that the masks cannot differ between fp32 and fp64: x, the weights, the gammas and the upstream gradients are
random, and the two shifts beta1, beta2 are PLACED, per channel, in the middle of the widest gap the sorted pre-activations of that
channel leave inside [-0.5, 0.5] (``place_beta``) -- decided by the fp64 run alone, then rounded to fp32 like every other input.
No pre-activation of either site is then closer to zero than ``MARGIN``.  The other discrete event, the argmax of a 2x2 pooling
window, is taken out the same way: windows whose two largest fp64 values are closer than ``MARGIN`` get a pooled gradient of zero,
so it does not matter where it would have been routed.  The values compared are the window's PRE-activations: the activation is
strictly increasing (pool cases have slope > 0), so they order the window as ``out`` does, and a gap between two negative ones
shrinks by the slope in ``out`` exactly as their rounding noise does -- measured on ``out`` itself the same MARGIN would take out
every window of negatives whose pre-activations are closer than MARGIN / slope, 1.3e-3 of the windows at the largest pool case.

The yardstick of a comparison is the same restatement run in fp32 on the CPU with the fp64 run's masks: ``d32`` is its max-norm
relative distance to fp64 per tensor, and a tensor's bar is ``max(4 * d32, floor of its kind)`` (``compare``), the rule of
tests/test_gp_pass_gpu.py."""
import functools
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

import gp_ref
from conftest import rel_err

IN_EPS = gp_ref.IN_EPS
SLOPE = 1e-2

# The smallest half-gap ``place_beta`` reaches over CASES, rounded down: 9.09e-5 at first-block, 9.55e-5 at res-wino-16 (131 072 values
# per channel), 1.4e-4 .. 2.8e-2 elsewhere.  test_block_ref_cpu.py asserts it for every case, together with
# MARGIN >= MARGIN_OVER_D32 x d32 of the same pre-activations (rel_err of the fp32 replay: 5e-7 .. 8e-7).
MARGIN = 9e-5
MARGIN_OVER_D32 = 20.0
MAX_ZEROED_WINDOWS = 1e-3        # share of a pool case's windows that may be taken out as near-ties

# Floors of the bars, per kind of tensor: what the kernels on the chain meet one at a time.
#   fwd        AFF_BAR of test_conv3x3_edges_gpu.py: the conv that reads its operand through the input-side InstanceNorm (conv2)
#   dgrad      gp_ref.SINGLE_OP_BARS["dydx"]: a data gradient through a whole block
#   wgrad      WGRAD_BAR / WGRAD_BAR_BIG of test_conv3x3_edges_gpu.py: weight gradients over <= 1e5 pixels / beyond
#   affine     gp_ref.SINGLE_OP_BARS["wgrad"]: the gamma / beta gradients, as test_gp_pass_gpu.py holds them
FLOORS = {"fwd": 5e-6, "dgrad": gp_ref.SINGLE_OP_BARS["dydx"], "wgrad": 3e-6, "wgrad_big": 5e-5, "affine": gp_ref.SINGLE_OP_BARS["wgrad"]}
WGRAD_BIG_PIXELS = 100000


class Case(NamedTuple):
    """form: "plain" | "cat" (basic_block_cat on the two parts) | "catmat" (basic_block on the materialised cat) | "pool".
    ci of a cat form is the width of the cat, two equal halves.  grads (pool): which of the two outputs bring a gradient, "both" | "pooled" | "skip".  needs: "all" | "no_x" (the block input does not
    want a gradient) | "frozen" (w1 and ws do not).  regime: what the id promises (checked on the CPU against the library's queries):
    "tile" per-tile kernels | "wino_l" streamed-weight Winograd | "res_wino" / "res_direct" resident weights, Winograd F(2x2) / direct."""
    id: str; n: int; ci: int; co: int; h: int; w: int                                                           # noqa: E702
    regime: str; form: str = "plain"; slope: float = SLOPE; grads: str = "both"; needs: str = "all"             # noqa: E702

    @property
    def has_sc(self):
        """conv shortcut: where the widths differ, and under every cat (``basic_block_cat`` and the split gradients exist for it only)"""
        return self.ci != self.co or self.form in ("cat", "catmat")

    @property
    def pool(self):
        return self.form == "pool"

    @property
    def ref_key(self):
        """cases with the same key share one reference (the ``needs`` variants differ in what the GPU is asked for only)"""
        return (self.n, self.ci, self.co, self.h, self.w, self.form, self.slope, self.grads if self.pool else "")


RES_DIRECT = (32, 16, 32, 40, 64)
SMALL_POOL = (2, 16, 32, 24, 32)
CASES = [
    Case("tile-identity", 3, 16, 16, 24, 20, "tile"),
    Case("tile-sc-tails", 2, 12, 20, 13, 31, "tile"),
    Case("tile-sc-k1", 2, 12, 516, 5, 9, "tile"),
    Case("tile-sc-1x1", 2, 16, 32, 24, 20, "tile"),
    Case("wino-identity", 2, 64, 64, 16, 32, "wino_l"),
    Case("wino-sc-1tile", 3, 64, 128, 16, 16, "wino_l"),
    Case("wino-sc-1image", 1, 128, 64, 32, 48, "wino_l"),
    Case("res-wino-16", 8, 16, 16, 128, 128, "res_wino"),
    Case("res-direct-32", *RES_DIRECT, "res_direct"),
    Case("res-many-images", 256, 16, 32, 8, 32, "res_direct"),
    Case("first-block", 8, 8, 16, 128, 128, "res_wino"),
    Case("cat-virtual-32", 8, 32, 32, 64, 128, "res_wino", "cat"),
    Case("cat-virtual-64", 2, 64, 64, 16, 32, "wino_l", "cat"),
    Case("cat-materialised", 2, 32, 16, 24, 20, "tile", "catmat"),
    Case("pool-both", *RES_DIRECT, "res_direct", "pool", grads="both"),
    Case("pool-only-pooled", *RES_DIRECT, "res_direct", "pool", grads="pooled"),
    Case("pool-only-skip", *RES_DIRECT, "res_direct", "pool", grads="skip"),
    Case("pool-both-tile", *SMALL_POOL, "tile", "pool", grads="both"),
    Case("pool-only-pooled-tile", *SMALL_POOL, "tile", "pool", grads="pooled"),
    Case("pool-only-skip-tile", *SMALL_POOL, "tile", "pool", grads="skip"),
    # variants: what is asked for, and the ReLU slope, on one per-tile and one persistent case each
    Case("tile-sc-1x1-no-x", 2, 16, 32, 24, 20, "tile", needs="no_x"),
    Case("tile-sc-1x1-frozen", 2, 16, 32, 24, 20, "tile", needs="frozen"),
    Case("res-direct-32-no-x", *RES_DIRECT, "res_direct", needs="no_x"),
    Case("res-direct-32-frozen", *RES_DIRECT, "res_direct", needs="frozen"),
    Case("tile-identity-relu", 3, 16, 16, 24, 20, "tile", slope=0.0),
    Case("res-direct-32-relu", *RES_DIRECT, "res_direct", slope=0.0),
]
TEETH_CASES = ("tile-sc-1x1", "res-direct-32")
PARAMS = ("w1", "g1", "b1", "w2", "g2", "b2", "ws", "gs", "bs")


def case(cid) -> Case:
    return next(c for c in CASES if c.id == cid)


# ------------------------------------------------------------------------------------------------------------------- the restatement
def _inorm(y, g, b):
    return F.instance_norm(y, weight=g, bias=b, eps=IN_EPS)


def _inorm_dropped_row(y, g, b):
    """a WRONG InstanceNorm, for the teeth test: mean and variance over H * W - W pixels (the first row is left out of the statistics)"""
    m = y[:, :, 1:, :].mean((2, 3), keepdim=True)
    v = ((y[:, :, 1:, :] - m) ** 2).mean((2, 3), keepdim=True)
    return (y - m) * torch.rsqrt(v + IN_EPS) * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def block(t, masks, slope, pool=False, mid=None, inorm2=_inorm):
    """blocks.BasicBlock.forward: out = act(IN2(conv2(act(IN1(conv1(x))))) + (INs(convs(x)) | x)), and max_pool2d(out, 2) with ``pool``.
    t: the operands by name (x or xa + xb; w1 g1 b1 w2 g2 b2 and, for a conv shortcut, ws gs bs).  ``mid`` collects graph tensors."""
    x = t["x"] if "x" in t else torch.cat([t["xa"], t["xb"]], 1)
    y1 = F.conv2d(x, t["w1"], padding=1)
    z1 = _inorm(y1, t["g1"], t["b1"])
    y2 = F.conv2d(gp_ref.act(z1, masks, "act1", slope), t["w2"], padding=1)
    idn = _inorm(F.conv2d(x, t["ws"]), t["gs"], t["bs"]) if "ws" in t else x
    pre = inorm2(y2, t["g2"], t["b2"]) + idn
    out = gp_ref.act(pre, masks, "out", slope)
    if mid is not None:
        mid.update(x=x, y1=y1, z1=z1, y2=y2, idn=idn, pre=pre)
    return out, (F.max_pool2d(out, 2) if pool else None)


# ------------------------------------------------------------------------------------------------------------------- flip-free inputs
def rnd(*shape, seed):
    """fp32 values, as test_fused_basic_block_vs_torch draws them"""
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape)).float()


def place_beta(u):
    """u [N, C, H, W] fp64, the pre-activation without its shift.  Per channel: minus the midpoint of the widest gap between consecutive
    sorted values of u[:, c] inside [-0.5, 0.5], rounded to fp32 -> beta [C] (fp64 holding fp32 values)"""
    c = u.shape[1]
    v = u.detach().transpose(0, 1).reshape(c, -1).sort(1).values
    beta = torch.empty(c, dtype=torch.float64)
    for k in range(c):
        s = v[k][(v[k] >= -0.5) & (v[k] <= 0.5)]
        assert s.numel() >= 2, "no two pre-activations inside [-0.5, 0.5]"
        gaps = s[1:] - s[:-1]
        i = int(gaps.argmax())
        beta[k] = -0.5 * (s[i] + s[i + 1])
    return beta.float().double()


def window_top2_gap(out):
    """[N, C, H/2, W/2]: largest minus second largest value of every 2x2 window"""
    n, c, h, w = out.shape
    win = out.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    top = win.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


def make_inputs(c: Case):
    """-> (operands, gradients, masks, info).  Everything holds fp32 values in fp64 tensors.  operands: x | xa, xb and the parameters;
    gradients: gout, gpooled (near-tie windows already zeroed); masks: {"act1", "out"} of the fp64 forward; info: margin (min |pre-activation|
    over both sites), zeroed (share of pooling windows taken out; zeroed_if_out: the share had the gap been measured on out)."""
    n, ci, co, h, w = c.n, c.ci, c.co, c.h, c.w
    t = {}
    if c.form in ("cat", "catmat"):
        t["xa"], t["xb"] = rnd(n, ci // 2, h, w, seed=1).double(), rnd(n, ci // 2, h, w, seed=21).double()
    else:
        t["x"] = rnd(n, ci, h, w, seed=1).double()
    t["w1"] = (rnd(co, ci, 3, 3, seed=2) / np.sqrt(9 * ci)).float().double()
    t["w2"] = (rnd(co, co, 3, 3, seed=3) / np.sqrt(9 * co)).float().double()
    t["g1"], t["g2"] = (1 + 0.1 * rnd(co, seed=4)).double(), (1 + 0.1 * rnd(co, seed=6)).double()
    if c.has_sc:
        t["ws"] = (rnd(co, ci, 1, 1, seed=11) / np.sqrt(ci)).float().double()
        t["gs"], t["bs"] = (1 + 0.1 * rnd(co, seed=8)).double(), (0.1 * rnd(co, seed=9)).double()
    grads = {"gout": rnd(n, co, h, w, seed=12).double()}
    zero = torch.zeros(co, dtype=torch.float64)
    with torch.no_grad():
        x = t["x"] if "x" in t else torch.cat([t["xa"], t["xb"]], 1)
        u1 = _inorm(F.conv2d(x, t["w1"], padding=1), t["g1"], zero)
        t["b1"] = place_beta(u1)
        pre1 = u1 + t["b1"].view(1, -1, 1, 1)
        masks = {"act1": pre1 > 0}
        a1 = gp_ref.act(pre1, masks, "act1", c.slope)
        idn = _inorm(F.conv2d(x, t["ws"]), t["gs"], t["bs"]) if c.has_sc else x
        u2 = _inorm(F.conv2d(a1, t["w2"], padding=1), t["g2"], zero) + idn
        t["b2"] = place_beta(u2)
        pre2 = u2 + t["b2"].view(1, -1, 1, 1)
        masks["out"] = pre2 > 0
        info = {"margin": float(min(pre1.abs().min(), pre2.abs().min())), "zeroed": 0.0}
        if c.pool:
            assert c.slope > 0, "the pre-activations order a window as out does under a strictly increasing activation only"
            tie = window_top2_gap(pre2) < MARGIN
            info["zeroed"] = float(tie.double().mean())
            info["zeroed_if_out"] = float((window_top2_gap(gp_ref.act(pre2, masks, "out", c.slope)) < MARGIN).double().mean())
            grads["gpooled"] = (rnd(n, co, h // 2, w // 2, seed=13).double() * (~tie))
    return t, grads, masks, info


def step(c: Case, t, grads, masks, dtype, corrupt=None, blk=None):
    """forward + backward of the restatement in ``dtype`` with the given masks (a missing one is filled in from the run's own
    pre-activation) -> {"out", "pooled", "pre1", "pre2", name: d / d name}.
    ``corrupt``: one of the wrong blocks of the teeth test (CORRUPTIONS).  ``blk``: a replay with ``block``'s signature that stands
    in for it (tests/block_f16_ref.py: the fp16 rounding model)."""
    blk = blk or block
    leaf = {k: v.detach().to(dtype).requires_grad_(True) for k, v in t.items()}            # (detach: never the shared inputs themselves)
    if corrupt == "act1_bit":                            # one mask bit flipped where the pre-activation is smallest
        masks = dict(masks)
        with torch.no_grad():
            mid = {}
            block(t, dict(masks), c.slope, mid=mid)
            flat = int(mid["z1"].abs().argmin())
        m = masks["act1"].clone()
        m.view(-1)[flat] = ~m.view(-1)[flat]
        masks["act1"] = m
    mid = {}
    out, pooled = blk(leaf, masks, c.slope, c.pool, mid, _inorm_dropped_row if corrupt == "stats2_row" else _inorm)
    outs, gs = [out], [grads["gout"].to(dtype)]
    if c.pool:
        outs, gs = {"both": ([out, pooled], [gs[0], grads["gpooled"].to(dtype)]), "pooled": ([pooled], [grads["gpooled"].to(dtype)]),
                    "skip": ([out], gs)}[c.grads]
    names = list(leaf)
    g = torch.autograd.grad(outs, [leaf[k] for k in names] + [mid["y1"], mid["pre"]], gs, retain_graph=corrupt is not None)
    res = dict(zip(names, g))
    gy1, gpre = g[-2], g[-1]
    if corrupt == "dx_sc_image":                         # the shortcut's contribution to dx left out for image 0
        assert "x" in leaf
        only0 = torch.zeros_like(gpre)
        only0[0] = gpre[0]
        res["x"] = res["x"] - (torch.autograd.grad(mid["idn"], leaf["x"], only0)[0] if c.has_sc else only0)
    elif corrupt == "w1_border_row":                     # w1's gradient without the first output row of image 0
        row = torch.zeros_like(gy1[:1])
        row[:, :, 0] = gy1[0, :, 0]
        res["w1"] = res["w1"] - torch.nn.grad.conv2d_weight(mid["x"][:1].detach(), leaf["w1"].shape, row, padding=1)
    elif corrupt == "g2_image":                          # gamma2's gradient summed over N - 1 images
        xh2 = F.instance_norm(mid["y2"].detach(), eps=IN_EPS)
        res["g2"] = res["g2"] - (gpre[0] * xh2[0]).sum((1, 2))
    res = {k: v.detach() for k, v in res.items()}
    res.update(out=out.detach(), pooled=None if pooled is None else pooled.detach(), pre1=mid["z1"].detach(), pre2=mid["pre"].detach())
    return res


CORRUPTIONS = ("act1_bit", "stats2_row", "dx_sc_image", "w1_border_row", "g2_image")


class Ref(NamedTuple):
    t: dict; grads: dict; masks: dict; info: dict; r64: dict; r32: dict                                          # noqa: E702


@functools.lru_cache(maxsize=None)
def _reference(key, cid):
    c = case(cid)
    t, grads, masks, info = make_inputs(c)
    r64 = step(c, t, grads, masks, torch.float64)
    r32 = step(c, t, grads, masks, torch.float32)
    info["pre_d32"] = max(rel_err(r32[k].numpy(), r64[k].numpy()) for k in ("pre1", "pre2"))
    info["pre_d32_abs"] = float(max((r32[k].double() - r64[k]).abs().max() for k in ("pre1", "pre2")))
    return Ref(t, grads, masks, info, r64, r32)


def reference(c: Case) -> Ref:
    """inputs, masks and both runs of a case, computed once per ``ref_key`` and shared; nothing in it may be written to"""
    first = next(k for k in CASES if k.ref_key == c.ref_key)
    return _reference(c.ref_key, first.id)


# ------------------------------------------------------------------------------------------------------------------- comparison
def kind_of(name, c: Case):
    if name in ("out", "pooled"):
        return "fwd"
    if name in ("x", "xa", "xb"):
        return "dgrad"
    if name in ("w1", "w2", "ws"):
        return "wgrad" if c.n * c.h * c.w <= WGRAD_BIG_PIXELS else "wgrad_big"
    return "affine"


def rows_of(c: Case, got, ref: Ref, names):
    return [(k, got[k], ref.r64[k], ref.r32[k], kind_of(k, c)) for k in names]


def compare(tag, rows, col="d32"):
    """rows: (name, tensor under test, fp64, fp32 replay, kind).  Prints err / d32 / bar of every tensor; -> [(name, err, bar)] of
    those that miss bar = max(4 d32, FLOORS[kind]), on max |got - fp64| / max |fp64|.  ``col``: what the yardstick column is
    called in the print ("d16" when it holds the fp16 rounding model of tests/block_f16_ref.py)."""
    fails = []
    for name, got, r64, r32, kind in rows:
        assert tuple(got.shape) == tuple(r64.shape), (tag, name, tuple(got.shape), tuple(r64.shape))
        d32 = rel_err(r32.numpy(), r64.numpy())
        bar = max(4.0 * d32, FLOORS[kind])
        e = rel_err(got.detach().cpu().numpy(), r64.numpy())
        print(f"{tag} {name}: err {e:.3g}  {col} {d32:.3g}  bar {bar:.3g} ({kind})  err/bar {e / bar:.3f}")
        if not e < bar:
            fails.append((name, e, bar))
    return fails


def grad_names(c: Case):
    """every gradient the block produces for this case when everything wants one"""
    xs = ["xa", "xb"] if c.form in ("cat", "catmat") else ["x"]
    return xs + [k for k in PARAMS if c.has_sc or k not in ("ws", "gs", "bs")]


# ------------------------------------------------------------------------------------------------------------------- the plan
def needs_of(c: Case):
    """``ctx.needs_input_grad`` of BasicBlockFn.apply(x, w1, g1, b1, w2, g2, b2, ws, gs, bs, slope, xa, xb, pool) for this case"""
    cat = c.form in ("cat", "catmat")
    x = c.needs != "no_x"
    w = c.needs != "frozen"
    return (x and not cat, w, True, True, True, True, True, c.has_sc and w, c.has_sc, c.has_sc, False, x and cat, x and cat, False)


def plans(ops, c: Case, like, fin=True):
    """(BlockPlan, BlockBwd) ``ops`` computes for the case.  like: a tensor of the block input's shape -- of one part for the virtual cat --
    on the device the block runs on (any device: only host queries are made).  fin: the in-launch-finalize probe's answer."""
    cat = (c.ci // 2, c.ci // 2) if c.form in ("cat", "catmat") else None
    p = ops._block_plan(like, cat, c.form == "cat", c.co, c.has_sc, float(c.slope), c.pool)
    b = ops._block_bwd_plan(p, needs_of(c), c.pool and c.grads == "both", lambda: fin)
    return p, b


def like_shape(c: Case):
    return (c.n, c.ci // 2 if c.form == "cat" else c.ci, c.h, c.w)


def expected_launches(H, p, b, pooled_only=False):
    """entry points of one forward + backward, in order, read from ops._bb_* (outside a wino_prepared scope; fp32 operands, and the
    fp16 plans of tests/block_f16_ref.py: their `_f16` / `_hs` twins and the launches that make the scales of the gradient operands).
    H: the library's host queries (_hip).  pooled_only: a pool block whose skip output brought no gradient (the plain pooling backward
    makes the tail's upstream gradient first)."""
    n, h, w, ci, co = p[:5]
    a16, c16 = "_f16" if p.f16a else "", "_f16" if p.f16 else ""
    if p.hs:
        f = ["smsut_conv2d_fwd_mfma_stats_sc_f16_hs"]
    else:
        f = ["smsut_conv2d_fwd_mfma_stats" + ("_sc_fin" if p.fin else "_sc" + a16 if p.fused_sc else "_cat" + a16 if p.virtual else a16)]
    if p.fin:
        f += ["smsut_conv2d_fwd_mfma_stats_inaff_fin"]
    else:
        if p.inaff:
            f += ["smsut_in_finalize_fwd", "smsut_conv2d_fwd_mfma_stats_inaff"]
        elif p.hs:
            f += ["smsut_in_finalize_fwd", "smsut_conv2d_fwd_mfma_stats_inaff_f16_hsx"]
        else:
            f += ["smsut_instnorm_fwd_partials", "smsut_conv2d_fwd_mfma_stats" + c16]
        f += ["smsut_in_finalize_fwd2" if p.fused_sc else "smsut_in_finalize_fwd"]
    if p.has_sc and not p.fused_sc:
        streaming = H.call("smsut_conv1x1_supported", ci, co) and H.call("smsut_conv1x1_tiles", n, h * w, co) > 0
        f += ["smsut_conv1x1_fwd_cat" if p.virtual else "smsut_conv1x1_fwd" if streaming else "smsut_conv2d_fwd_mfma_stats", "smsut_in_finalize_fwd"]
    f += ["smsut_restail_fwd_pool" if p.pool else "smsut_restail_fwd_hs" if p.hs else "smsut_restail_fwd"]
    g = ["smsut_maxpool2_bwd"] if pooled_only else []
    g += [{"pool": "smsut_restail_bwd_pool", "hs": "smsut_restail_bwd_hs", "amax": "smsut_restail_bwd_amax", "fin": "smsut_restail_bwd_fin",
           "plain": "smsut_restail_bwd"}[b.tail]]
    if p.f16:                                            # the scale of gy2: from the tail's maxima, else a pass over the tensor
        g += ["smsut_absmax_finish" if b.nb else "smsut_absmax_scale"]
    if not b.pers2:
        g += ["smsut_conv2d_fwd_mfma" + c16, "smsut_instnorm_bwd"]
    else:
        if p.f16:
            g += ["smsut_conv2d_dgrad_mfma_bwdstats_f16" + ("_hs" if p.hs else "")]
        else:
            g += ["smsut_conv2d_dgrad_mfma_bwdstats_fin" if b.fin_b else "smsut_conv2d_dgrad_mfma_bwdstats"]
        g += [] if b.fin_b else ["smsut_in_finalize_bwd"]
        g += ["smsut_in_apply_bwd_hs" if p.hs else "smsut_in_apply_bwd_amax" if b.amax1 else "smsut_in_apply_bwd"]
    if p.hs or b.f16w2:
        g += ["smsut_conv2d_wgrad_f16_xh_inaff" if p.hs else "smsut_conv2d_wgrad_f16"]
    else:
        g += ["smsut_conv2d_wgrad_mfma_inaff" if p.inaff else "smsut_conv2d_wgrad_mfma"]
    if p.f16a:                                           # the scale of gy1, or ONE over [gy1 | gs_t] where a fused-shortcut gradient reads both
        both = b.fused_wsc16 or b.fused_dsc16
        g += ["smsut_absmax_finish" if b.amax1 else "smsut_absmax_scale2" if both else "smsut_absmax_scale"]
    if b.fused_wsc16:
        g += ["smsut_conv2d_wgrad_sc_f16"]
    elif b.fused_wsc:
        g += ["smsut_conv2d_wgrad_mfma_sc"]
    else:
        g += ["smsut_conv2d_wgrad_f16" if b.f16w1 else "smsut_conv2d_wgrad_mfma_cat" if p.virtual else "smsut_conv2d_wgrad_mfma"]
        if p.has_sc:
            g += ["smsut_conv1x1_wgrad_cat" if p.virtual else "smsut_conv1x1_wgrad"]
    if b.dx == "sc_f16":
        g += ["smsut_conv2d_dgrad_mfma_sc_f16"]
    elif b.dx == "sc":
        g += ["smsut_conv2d_dgrad_mfma_sc"]
    elif b.dx == "split":
        g += ["smsut_conv1x1_fwd_split", "smsut_conv2d_fwd_mfma_split" + a16]
    elif b.dx is not None:
        g += ["smsut_conv2d_fwd_mfma"] if b.dx == "accum_k1" else ["smsut_conv1x1_fwd"] if p.has_sc else []
        g += ["smsut_conv2d_fwd_mfma" + a16] + (["smsut_concat2"] if p.cat is not None else [])
    return f, g


def regime_of(H, c: Case):
    """which 3x3 kernel family conv1 and conv2 of the case run, from the library's queries"""
    def one(kd, nd):
        if not H.call("smsut_conv2d_mfma_persistent", c.n, c.h, c.w, kd, nd, 3, 0):
            return "tile"
        return ("res_direct", "res_wino", "wino_l")[H.call("smsut_conv2d_mfma_form", c.n, c.h, c.w, kd, nd, 0)]
    return one(c.ci, c.co), one(c.co, c.co)
