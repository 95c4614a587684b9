"""fp16 rounding model of the fused BasicBlock under ``ops.set_conv_dtype("f16")`` (tests/test_block_f16_gpu.py; pinned without a
device by tests/test_block_f16_ref_cpu.py), and the cases that reach every branch of the fp16 plan.

The REFERENCE of a comparison stays ``block_ref.step(..., torch.float64)``, unrounded.  This file adds the yardstick: a second replay
of ``block_ref.block`` on the CPU, in fp32, that rounds to fp16 (round to nearest even) exactly where DESIGN.md 3b and the comments of
``ops._block_plan`` say the device does (``Flags``, read off the two plans by ``flags_of``):

  conv operands      both operands of a 3x3 conv with fp16 operands (conv1 under ``f16a``, conv2 under ``f16``), and of the 1x1 shortcut
                     where it runs inside conv1's fp16 pass; the products are exact in fp32 and accumulate in fp32;
  gradient operands  in the backward of such a conv the gradient operand is half(gy * s) / s, s the power of two that puts max |gy|
                     into [2^13, 2^14) -- ONE s over [gy1 | gs_t] where a fused-shortcut gradient kernel reads both; the other operand
                     keeps the bits the forward rounded.  A gradient the plan leaves to an fp32 kernel (the weight gradient of a ragged
                     plane, a separate 1x1 shortcut) reads the unrounded operands;
  half storage       under ``hs`` y1, y2 and s are rounded at the store and every reader -- the InstanceNorm apply forward and
                     backward, both tail passes -- sees the rounded values, with the statistics of the UNROUNDED fp32 values; conv2's
                     operand is half(lrelu(IN(widened y1)));
  the 8 -> 16 block  ``f16a`` false, ``hs`` true: conv1 and the shortcut keep fp32 operands and store fp16.

``d16`` of a tensor is the max-norm relative distance of the model to fp64, and its bar is max(4 d16, block_ref.FLOORS[kind]) on
max |got - fp64| / max |fp64|: ``block_ref.compare`` with the model in the fp32 column.  The model is a yardstick: the device differs
from it by fp32 accumulation order and rare rounding ties at the stores.

A max-norm comparison at fp16 noise cannot tolerate a flipped LeakyReLU sign, and the half-storage plan needs >= 32 768 values per
channel, where no placement of beta buys a margin against 2e-3 of noise.  So there are two kinds of case:

  smooth cases (slope 1.0)  the slope is a runtime float: the block launches the same kernels with the same plan, and nothing but the
                            pooling argmax is discrete.  Every plan branch has one.  Pool cases: windows whose fp64 top-two gap of the
                            pre-activations is below POOL_GAP_OVER_NOISE x max |model pre2 - fp64 pre2| get no pooled gradient; at most
                            MAX_ZEROED_WINDOWS of the windows may go.
  sign cases (slope 0.01)   tiny planes on the per-tile kernels, where ``block_ref.place_beta`` still reaches
                            min |pre-activation| >= MARGIN_OVER_NOISE x max |model pre-activation - fp64 pre-activation| over both sites.

The upstream gradients are ``block_ref``'s times 2^-22 (2.4e-7, their magnitude at 512^2): a power of two scales every fp64 and fp32
figure exactly, and a gradient operand converted without its scale underflows there (the corruption "noscale")."""
import functools
import math
from typing import NamedTuple

import torch
import torch.nn.functional as F
from torch.autograd import Function

import block_ref as R
import gp_ref

GRAD_SCALE = 2.0 ** -22
MARGIN_OVER_NOISE = 6.0
POOL_GAP_OVER_NOISE = 6.0
MAX_ZEROED_WINDOWS = 0.03


class Case(NamedTuple):
    """``block_ref.Case`` with the plan branch the case claims in place of the regime (``check_plan``), and ``sc``: a conv shortcut
    between equal widths (the block takes one wherever ``ws`` is given)."""
    id: str; n: int; ci: int; co: int; h: int; w: int                                                           # noqa: E702
    branch: str; form: str = "plain"; slope: float = 1.0; grads: str = "both"; needs: str = "all"; sc: bool = False   # noqa: E702

    @property
    def has_sc(self):
        return self.sc or self.ci != self.co or self.form in ("cat", "catmat")

    @property
    def pool(self):
        return self.form == "pool"

    @property
    def ref_key(self):
        return (self.n, self.ci, self.co, self.h, self.w, self.form, self.slope, self.grads if self.pool else "", self.sc)


HS_FUSED = (256, 32, 32, 8, 32)          # 1024 items for conv1, conv2 and the fused-shortcut data-gradient (reduction 2 x 32)
HS_POOL = (32, 16, 32, 40, 64)           # H % 16 != 0, 20 statistics tiles per image
F16_CASES = [
    # ---- smooth, slope 1.0: one per plan branch
    Case("hs-16-32", 256, 16, 32, 8, 32, "hs"),                                   # dx: fp32 1x1 + accumulating fp16 3x3
    Case("hs-32-32", *HS_FUSED, "hs_fused", sc=True),                            # fully fused: dx sc_f16
    Case("hs-64-64", 128, 64, 64, 8, 32, "hs", sc=True),
    Case("hs-first-8-16", 128, 8, 16, 16, 64, "hs_first"),
    Case("hs-cat-32", 256, 64, 32, 8, 32, "hs_cat", "cat"),
    Case("hs-cat-64", 128, 64, 64, 8, 32, "hs_cat", "cat"),
    Case("hs-pool-both", *HS_POOL, "hs_pool", "pool", grads="both"),
    Case("hs-pool-pooled", *HS_POOL, "hs_pool", "pool", grads="pooled"),
    Case("identity-persistent", 128, 16, 16, 16, 64, "identity_pers"),
    Case("tile-whole", 2, 16, 32, 24, 32, "tile"),
    Case("tile-ragged", 2, 16, 32, 13, 31, "tile_ragged"),
    Case("tile-deep-128", 2, 128, 128, 16, 16, "tile_deep"),
    Case("conv1-fp32-24-16", 2, 24, 16, 24, 32, "conv2_only"),
    Case("hs-32-32-no-x", *HS_FUSED, "hs_fused", needs="no_x", sc=True),
    Case("hs-32-32-frozen", *HS_FUSED, "hs_fused", needs="frozen", sc=True),
    # ---- signs, slope 0.01: tiny planes, per-tile kernels
    Case("sign-16-16", 1, 16, 16, 8, 16, "sign", slope=R.SLOPE),
    Case("sign-16-32", 1, 16, 32, 8, 16, "sign", slope=R.SLOPE),
    Case("sign-64-64", 1, 64, 64, 8, 8, "sign", slope=R.SLOPE),
    Case("sign-16-16-n2", 2, 16, 16, 8, 16, "sign", slope=R.SLOPE),
    Case("sign-32-32", 1, 32, 32, 16, 16, "sign", slope=R.SLOPE),
]
TEETH_CASES = ("hs-32-32", "sign-16-32")
FP32_TWIN_CASE = "hs-16-32"              # the case on which the GPU test also runs the fp32 mode: out must differ


def case(cid) -> Case:
    return next(c for c in F16_CASES if c.id == cid)


def check_plan(c: Case, p, b):
    """the plan fields of the branch the case claims (p, b: ``block_ref.plans`` under fp16)"""
    got = f"{c.id}: {p} {b}"
    assert p.f16 and b.nb > 0 and not (p.fin or p.inaff or p.pair or b.fin_ok or b.fin_b or b.pair1 or b.pair2), got
    assert (p.has_sc, p.pool, p.virtual) == (c.has_sc, c.pool, c.form == "cat"), got
    assert (b.dx is None) == (c.needs == "no_x"), got
    br = c.branch
    if br.startswith("hs"):
        assert p.hs and p.fused_sc and b.pers2 and b.amax1 and b.f16w2, got
        assert b.tail == ("pool" if c.pool and c.grads == "both" else "hs"), got
    else:
        assert not p.hs and b.tail == "amax", got
    if br in ("hs", "hs_fused", "hs_cat", "hs_pool"):
        assert p.f16a and b.f16w1 and b.fused_wsc16, got
    if br in ("hs", "hs_pool"):                          # too few items for the fused-shortcut data-gradient: fp32 1x1 + accumulating fp16 3x3
        assert not b.fused_dsc16 and b.dx == "accum", got
    if br == "hs_fused":                                 # ONE scale over [gy1 | gs_t] serves both fused-shortcut gradient kernels
        assert b.fused_dsc16 == (c.needs != "no_x") and b.dx == ("sc_f16" if c.needs != "no_x" else None), got
    elif br == "hs_first":                               # fp32 operands, half storage: conv1 + shortcut gradients on the fp32 fused kernels
        assert c.ci == 8 and not p.f16a and not b.f16w1 and not b.fused_wsc16 and b.fused_wsc and b.dx == "sc", got
    elif br == "hs_cat":                                 # the block-input gradient goes into the two parts
        assert p.cat is not None and b.dx == ("sc_f16" if c.co <= 32 else "split") and b.fused_dsc16 == (c.co <= 32), got
    elif br == "identity_pers":                          # a1 built in fp32; persistent data-gradient + apply with the maxima of gy1
        assert p.f16a and not p.has_sc and b.pers2 and b.amax1 and b.f16w1 and b.f16w2 and b.dx == "accum", got
    elif br in ("tile", "tile_deep", "sign"):
        assert p.f16a and not b.pers2 and not b.amax1 and b.dx == "accum", got
        assert b.f16w2 == (c.h % 8 == 0 and c.w % 16 == 0) and (b.f16w2 or br == "sign"), got      # (sign-64-64: an 8 x 8 plane)
        if br == "tile_deep":
            assert min(c.ci, c.co) >= 128, got
    elif br == "tile_ragged":                            # both weight gradients fall back to fp32 operands
        assert p.f16a and not b.pers2 and not b.f16w1 and not b.f16w2 and not b.fused_wsc16, got
        assert c.h % 8 and c.w % 16, got
    elif br == "conv2_only":                             # conv1 and a separate shortcut stay fp32, conv2 is fp16
        assert c.ci % 16 and not p.f16a and not p.fused_sc and p.has_sc and not b.f16w1 and b.f16w2 and not b.pers2, got


# ------------------------------------------------------------------------------------------------------------------- the rounding model
class Flags(NamedTuple):
    """where the device rounds to fp16.  f16a, f16, hs: the three plan flags.  The rest says which of conv1's neighbours share its fp16
    pass: sc16 the shortcut's forward (``fused_sc`` under ``f16a``); joint ONE gradient scale over [gy1 | gs_t]; w1h / w2h / wsh the
    weight gradient of conv1 / conv2 / the shortcut on fp16 operands; dsh the shortcut's data-gradient.  noscale: the corruption."""
    f16a: bool = False; f16: bool = False; hs: bool = False                                                       # noqa: E702
    sc16: bool = False; joint: bool = False; w1h: bool = False; w2h: bool = False; wsh: bool = False; dsh: bool = False   # noqa: E702
    noscale: bool = False


def flags_of(p, b) -> Flags:
    return Flags(p.f16a, p.f16, p.hs, p.fused_sc and p.f16a, p.f16a and (b.fused_wsc16 or b.fused_dsc16), b.f16w1, p.hs or b.f16w2,
                 b.fused_wsc16, b.dx == "sc_f16")


def half(t):
    return t.half().float()


def grad_scale(*ts):
    """csrc/conv_mfma.hip k_absmax_final: m = f * 2^e, f in [0.5, 1) -> s = 2^(14 - e); 1 for an all-zero tensor"""
    m = max(float(t.abs().max()) for t in ts)
    if not (0.0 < m < 3.0e38):
        return 1.0
    return 2.0 ** (14 - math.frexp(m)[1])


def _conv_bwd(gy, x, w, pad, which):
    """one of the three gradients of conv2d(x, w, padding=pad), by the kernel autograd itself calls"""
    mask = [which == "x", which == "w", False]
    return torch.ops.aten.convolution_backward(gy, x, w, None, [1, 1], [pad, pad], [1, 1], False, [0, 0], 1, mask)[0 if which == "x" else 1]


class _Conv16(Function):
    """y = conv3x3(half(x), half(w)) and, with ``ws``, s = conv1x1(x, ws) on rounded (``f.sc16``) or plain operands; the backward rounds
    the gradient operands under their power-of-two scale and reads the operand bits of the forward (cfg: 3x3 weight gradient on fp16
    operands, the shortcut's weight / data gradient on fp16 operands, one scale for both gradients, no scale at all)."""

    @staticmethod
    def forward(ctx, x, w, ws, cfg):
        sc16, wh, wsh, dsh, joint, noscale = cfg
        xr, wr = half(x), half(w)
        ctx.cfg = cfg
        ctx.save_for_backward(x, w, ws)
        y = F.conv2d(xr, wr, padding=1)
        if ws is None:
            return y
        return y, (F.conv2d(xr, half(ws)) if sc16 else F.conv2d(x, ws))

    @staticmethod
    def backward(ctx, gy, gs=None):
        sc16, wh, wsh, dsh, joint, noscale = ctx.cfg
        x, w, ws = ctx.saved_tensors
        xr, wr = half(x), half(w)
        s = 1.0 if noscale else grad_scale(gy, gs) if (joint and ws is not None) else grad_scale(gy)
        gyr = half(gy * s) / s
        gx = _conv_bwd(gyr, xr, wr, 1, "x")
        gw = _conv_bwd(gyr, xr, wr, 1, "w") if wh else _conv_bwd(gy, x, w, 1, "w")
        if ws is None:
            return gx, gw, None, None
        gsr = half(gs * s) / s
        gx = gx + (_conv_bwd(gsr, xr, half(ws), 0, "x") if dsh else _conv_bwd(gs, x, ws, 0, "x"))
        gws = _conv_bwd(gsr, xr, half(ws), 0, "w") if wsh else _conv_bwd(gs, x, ws, 0, "w")
        return gx, gw, gws, None


class _InormStored(Function):
    """InstanceNorm of a tensor stored as fp16: mean and rstd of the fp32 values, applied to the rounded ones, forward and backward
    (the readers widen what was stored and compute as before)."""

    @staticmethod
    def forward(ctx, y, g, b):
        m = y.mean((2, 3), keepdim=True)
        r = torch.rsqrt(((y - m) ** 2).mean((2, 3), keepdim=True) + R.IN_EPS)
        xh = (half(y) - m) * r
        ctx.save_for_backward(xh, r, g)
        return xh * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)

    @staticmethod
    def backward(ctx, gz):
        xh, r, g = ctx.saved_tensors
        gy = r * g.view(1, -1, 1, 1) * (gz - gz.mean((2, 3), keepdim=True) - xh * (gz * xh).mean((2, 3), keepdim=True))
        return gy, (gz * xh).sum((0, 2, 3)), gz.sum((0, 2, 3))


def block16(f: Flags):
    """``block_ref.block`` with the roundings of ``f``; with none set it runs block's own operations (bit-identical results)"""
    def blk(t, masks, slope, pool=False, mid=None, inorm2=R._inorm):
        x = t["x"] if "x" in t else torch.cat([t["xa"], t["xb"]], 1)
        ws = t.get("ws")
        inorm = (lambda y, g, b: _InormStored.apply(y, g, b)) if f.hs else R._inorm
        if f.f16a:
            r = _Conv16.apply(x, t["w1"], ws, (f.sc16, f.w1h, f.wsh, f.dsh, f.joint, f.noscale))
            y1, s = r if ws is not None else (r, None)
        else:
            y1, s = F.conv2d(x, t["w1"], padding=1), (F.conv2d(x, ws) if ws is not None else None)
        z1 = inorm(y1, t["g1"], t["b1"])
        a1 = gp_ref.act(z1, masks, "act1", slope)
        y2 = _Conv16.apply(a1, t["w2"], None, (False, f.w2h, False, False, False, f.noscale)) if f.f16 else F.conv2d(a1, t["w2"], padding=1)
        idn = inorm(s, t["gs"], t["bs"]) if ws is not None else x
        pre = (inorm if inorm2 is R._inorm else inorm2)(y2, t["g2"], t["b2"]) + idn
        out = gp_ref.act(pre, masks, "out", slope)
        if mid is not None:
            mid.update(x=x, y1=y1, z1=z1, y2=y2, idn=idn, pre=pre)
        return out, (F.max_pool2d(out, 2) if pool else None)
    return blk


def step16(c: Case, t, grads, masks, f: Flags, corrupt=None):
    """``block_ref.step`` of the model: fp32, the given masks, the roundings of ``f``"""
    return R.step(c, t, grads, masks, torch.float32, corrupt=corrupt, blk=block16(f))


CORRUPTIONS = R.CORRUPTIONS + ("noscale",)


def corrupted(c: Case, ref, wrong):
    """a subtly wrong block run through the model: one of block_ref's, or a gradient operand converted to fp16 without its scale"""
    if wrong == "noscale":
        return step16(c, ref.t, ref.grads, ref.masks, ref.flags._replace(noscale=True))
    return step16(c, ref.t, ref.grads, ref.masks, ref.flags, corrupt=wrong)


# ------------------------------------------------------------------------------------------------------------------- inputs, reference
class Ref(NamedTuple):
    """r32 holds the MODEL's results: the column ``block_ref.rows_of`` / ``compare`` take the yardstick from"""
    t: dict; grads: dict; masks: dict; info: dict; r64: dict; r32: dict; flags: Flags                            # noqa: E702


@functools.lru_cache(maxsize=None)
def _reference(cid, f: Flags):
    c = case(cid)
    t, grads, masks, info = R.make_inputs(c)
    grads = {"gout": grads["gout"] * GRAD_SCALE}
    with torch.no_grad():                                # the forward alone: how far the model's pre-activations sit from fp64
        m64, m16 = {}, {}
        R.block(t, masks, c.slope, mid=m64)
        block16(f)({k: v.float() for k, v in t.items()}, masks, c.slope, mid=m16)
    noise = [float((m16[k].double() - m64[k]).abs().max()) for k in ("z1", "pre")]
    info.update(noise1=noise[0], noise2=noise[1], zeroed=0.0, gap=0.0)
    if c.pool:
        info["gap"] = POOL_GAP_OVER_NOISE * noise[1]
        tie = R.window_top2_gap(m64["pre"]) < info["gap"]
        info["zeroed"] = float(tie.double().mean())
        grads["gpooled"] = R.rnd(c.n, c.co, c.h // 2, c.w // 2, seed=13).double() * (~tie) * GRAD_SCALE
    r64 = R.step(c, t, grads, masks, torch.float64)
    return Ref(t, grads, masks, info, r64, step16(c, t, grads, masks, f), f)


def reference(c: Case, f: Flags) -> Ref:
    """inputs, masks, the fp64 run and the model's run under ``f``, computed once per (``ref_key``, flags) and shared; read-only"""
    first = next(k for k in F16_CASES if k.ref_key == c.ref_key)
    return _reference(first.id, f)


_PLANS = {}


def plans_cpu(c: Case, ops=None):
    """(BlockPlan, BlockBwd) of the case under fp16, from the library's host queries alone (a meta tensor, no device); the conv dtype
    is put back.  ops: the imported library (default: built and imported here)."""
    if c.id not in _PLANS:
        if ops is None:
            import __graft_entry__ as ge
            ge.build()
            import smsut_amd  # noqa: F401
            from smsut_amd import ops
        prev = ops.conv_dtype()
        ops.set_conv_dtype("f16")
        try:
            _PLANS[c.id] = R.plans(ops, c, torch.empty(R.like_shape(c), device="meta"), fin=False)
        finally:
            ops.set_conv_dtype(prev)
    return _PLANS[c.id]
