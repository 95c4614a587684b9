"""The convolution kernels outside the Winograd / persistent 3x3 families against fp64 on the CPU, each through its own C-ABI
entry point, at the shapes where its launch plan or its tile configuration changes:

  1. the streaming 1x1 GEMM (``csrc/conv1x1.hip``: ``conv1x1_fwd<MR, NR>``, ``conv1x1_wgrad<CIT, COT>``, ``sum_parts``),
  2. the thin 1x1 heads (``thin1x1_dgrad`` / ``thin1x1_wgrad`` / ``thin1x1_wsum``),
  3. ConvTranspose2d(k=2, s=2): the per-tap MFMA form (``dispatch_fwd<1>`` with osc = 2 / isc = 2, ``launch_wgrad<1, ..>(.., 2, 4)``)
     and the pixel-shuffle form of the 1x1 kernels,
  4. the 4x4 stride-1 pad-1 kernels (``conv_k4_fwd<TH, NT>``, ``conv_k4_wgrad<COT>``),
  5. the small-channel direct kernels and the flattened-M weight gradient (``csrc/conv_small.hip``, non-stem shapes),
  6. the naive fallbacks (``csrc/conv_naive.hip``).

Conventions: tensors are NHWC, weights HWIO (``[tap][Cin][Cout]``); every reference is fp64 (matmul on doubles, ``F.conv2d`` on
doubles); outputs and workspaces are NaN inside and carry a sentinel guard behind them in the same allocation, a workspace is exactly
its ``*_ws`` query; the ``*_supported`` predicate is asserted before a launch.  Bars are the ones ``test_ops_gpu.py`` holds these
kernels to, on ``conftest.rel_err``: 1e-5 forward / data-gradient, 5e-5 weight gradient; each case prints its figure.  One test per
family ties ``ops.conv2d`` / ``ops.conv_transpose2x2`` to the direct call bit for bit."""
import pytest
import torch

from conv_edge_helpers import cdiv, check, conv_ref, gen, guarded_out, out_buf, poisoned, rn, untouched

pytestmark = pytest.mark.gpu

FWD_BAR = 1e-5
WGRAD_BAR = 5e-5
EW_CAP_ITEMS = 2048 * 256          # work items of one trip of a capped elementwise grid (ew_grid)


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
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _hip


# ================================================================================================ 1. the 1x1 GEMM
# conv1x1_fwd_launch (conv1x1.hip:421-436): MR = 4 when P / 256 >= 512 (P = N * HW >= 131072) else 1; NR = 1 when Ndim <= 16 else 2
# (a workgroup owns a 16 * NR channel slab, grid.y walks the slabs); the reduction runs in 16-channel chunks whose 4-channel quads
# are masked by `kok` (conv1x1.hip:83).  Per case below: P -> MR; Ndim -> NR and the slab picture (5: one ragged 16-tile | 16: one
# exact | 20: second 16-tile ragged | 40: second 32-slab ragged | 64: two full slabs); Kdim (4 / 12: one partial chunk | 20: a
# partial second chunk | 64: four chunks | 512: 32 chunks = the 64 KiB weight image at NR = 2).  3*7*9 = 189 pixels: P % 64 != 0, the
# last workgroup has waves past P; 511*256 = 130816: P / 256 = 511, the last MR = 1 size; 2*256*256 = 131072: the first MR = 4 size;
# 2*257*257 = 132098 = 516 * 256 + 2: MR = 4 with a ragged last wave step.
# (mr_of / nr_of restate the launch rule cited above; the library exports no query for the chosen instantiation -- only
#  smsut_conv1x1_tiles reflects MR, and the statistics test checks it.  Edit them together with conv1x1.hip:421-423.)
def mr_of(P):
    return 4 if P // 256 >= 512 else 1


def nr_of(ndim):
    return 1 if ndim <= 16 else 2


def _fwd1_id(n, h, w, k, nd, tr):
    return f"mr{mr_of(n * h * w)}-nr{nr_of(nd)}-P{n * h * w}-k{k}-n{nd}-{'dgrad' if tr else 'fwd'}"


FWD1 = [(3, 7, 9, 4, 5, 0), (3, 7, 9, 12, 16, 1), (2, 16, 20, 20, 20, 0), (2, 16, 20, 64, 40, 1), (1, 16, 16, 512, 64, 1),
        (1, 16, 16, 512, 40, 0), (1, 511, 256, 4, 16, 0),
        (2, 256, 256, 4, 16, 0), (2, 256, 256, 12, 5, 1), (2, 257, 257, 20, 20, 0), (2, 257, 257, 4, 40, 1),
        (2, 256, 256, 64, 64, 0), (2, 256, 256, 512, 5, 0)]


def _mk1(n, h, w, k, nd, tr, seed):
    g = gen(seed)
    x = rn(g, n * h * w, k)
    wt = rn(g, nd, k, scale=k ** -0.5) if tr else rn(g, k, nd, scale=k ** -0.5)     # data-gradient: [Cin = Ndim][Cout = Kdim] memory
    ref = x.double() @ (wt.double().t() if tr else wt.double())
    return x.cuda(), wt.cuda(), ref


@pytest.mark.parametrize("n,h,w,k,nd,tr", [pytest.param(*c, id=_fwd1_id(*c)) for c in FWD1])
def test_conv1x1_forward(H, n, h, w, k, nd, tr):
    assert H.call("smsut_conv1x1_supported", k, nd) == 1
    x, wt, ref = _mk1(n, h, w, k, nd, tr, 11)
    y, guard = out_buf(n * h * w, nd)
    H.call("smsut_conv1x1_fwd", x, wt, y, None, n, h * w, k, nd, tr, H.stream_ptr())
    check("conv1x1_fwd", y, ref, FWD_BAR)
    assert untouched(guard)


def test_conv1x1_table_is_covered():
    """every MR x NR cell, and every Ndim / Kdim value of the lists above with both MRs"""
    cells = {(mr_of(n * h * w), nr_of(nd)) for n, h, w, k, nd, tr in FWD1}
    assert cells == {(1, 1), (1, 2), (4, 1), (4, 2)}
    for mr in (1, 4):
        assert {nd for n, h, w, k, nd, tr in FWD1 if mr_of(n * h * w) == mr} >= {5, 16, 20, 40, 64}
        assert {k for n, h, w, k, nd, tr in FWD1 if mr_of(n * h * w) == mr} >= {4, 12, 20, 64, 512}
        assert {tr for n, h, w, k, nd, tr in FWD1 if mr_of(n * h * w) == mr} == {0, 1}


# virtual cat (conv1x1.hip:68-88, DUAL): chunk c comes from xb when 16 c >= ca; Kdim - ca = 4: xb's only chunk has one live quad |
# 16: one full chunk | 20: a full chunk and a one-quad chunk; ca = 32, Kdim = 64: two chunks from each tensor.  MR = 1, both NRs.
CAT1 = [(3, 7, 9, 16, 20, 20), (2, 16, 20, 16, 32, 16), (3, 7, 9, 16, 36, 40), (2, 16, 20, 32, 64, 32)]


@pytest.mark.parametrize("n,h,w,ca,k,nd", CAT1, ids=[f"ca{c[3]}-k{c[4]}-n{c[5]}" for c in CAT1])
def test_conv1x1_forward_virtual_cat(H, n, h, w, ca, k, nd):
    assert H.call("smsut_conv1x1_supported", k, nd) == 1
    P, st = n * h * w, H.stream_ptr()
    g = gen(12)
    xa, xb, wt = rn(g, P, ca), rn(g, P, k - ca), rn(g, k, nd, scale=k ** -0.5)
    cat = torch.cat([xa, xb], 1).contiguous()
    ref = cat.double() @ wt.double()
    y, guard = out_buf(P, nd)
    H.call("smsut_conv1x1_fwd_cat", xa.cuda(), xb.cuda(), ca, wt.cuda(), y, None, n, h * w, k, nd, st)
    check("conv1x1_fwd_cat", y, ref, FWD_BAR)
    ym, guard_m = out_buf(P, nd)
    H.call("smsut_conv1x1_fwd", cat.cuda(), wt.cuda(), ym, None, n, h * w, k, nd, 0, st)
    assert torch.equal(y, ym), "the virtual cat must give the bits of the materialised one"
    assert untouched(guard, guard_m)


# split output (conv1x1.hip:100-106): Ndim > 16 -> NR = 2, 32-channel slabs; the 16-tile j of slab co0 goes to yb when co0 + 16 j >=
# split.  split 16 / Ndim 32: the two tiles of ONE slab part | split 16 / Ndim 40: yb = 24 channels, ragged second slab | split 32 /
# Ndim 48: the split is a slab boundary.  Both weight readings (transposed = 0 / 1).
SPLIT1 = [(16, 32), (16, 40), (32, 48)]


@pytest.mark.parametrize("tr", [0, 1], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("split,nd", SPLIT1, ids=[f"split{s}-n{n}" for s, n in SPLIT1])
def test_conv1x1_forward_split(H, split, nd, tr):
    n, h, w, k = 3, 7, 9, 20
    assert H.call("smsut_conv1x1_supported", k, nd) == 1
    P, st = n * h * w, H.stream_ptr()
    x, wt, ref = _mk1(n, h, w, k, nd, tr, 13)
    ya, ga = out_buf(P, split)
    yb, gb = out_buf(P, nd - split)
    H.call("smsut_conv1x1_fwd_split", x, wt, ya, yb, split, n, h * w, k, nd, tr, st)
    check("split low", ya, ref[:, :split], FWD_BAR)
    check("split high", yb, ref[:, split:], FWD_BAR)
    y, gy_ = out_buf(P, nd)
    H.call("smsut_conv1x1_fwd", x, wt, y, None, n, h * w, k, nd, tr, st)
    assert torch.equal(ya, y[:, :split]) and torch.equal(yb, y[:, split:])
    assert untouched(ga, gb, gy_)


# statistics partials (conv1x1.hip:135-145): one {sum, sum of squares} per wave step of 16 MR pixels, tiles = HW / (16 MR) per image
# (smsut_conv1x1_tiles, conv1x1.hip:407-412).  3 x (16*20) pixels: MR = 1, 20 tiles per image, Ndim 20 -> NR = 2 with a ragged second
# tile | 2 x 256^2: MR = 4, 1024 tiles per image, Ndim 16 -> NR = 1.
STATS1 = [pytest.param(3, 16 * 20, 12, 20, id="mr1-nr2-20tiles"), pytest.param(2, 256 * 256, 4, 16, id="mr4-nr1-1024tiles")]


@pytest.mark.parametrize("n,hw,k,nd", STATS1)
def test_conv1x1_statistics_partials(H, n, hw, k, nd):
    st = H.stream_ptr()
    tiles = H.call("smsut_conv1x1_tiles", n, hw, nd)
    assert tiles == hw // (16 * mr_of(n * hw)) and hw % (16 * mr_of(n * hw)) == 0
    x, wt, ref = _mk1(n, hw, 1, k, nd, 0, 14)
    y, gy_ = out_buf(n * hw, nd)
    H.call("smsut_conv1x1_fwd", x, wt, y, None, n, hw, k, nd, 0, st)
    ys, gs = out_buf(n * hw, nd)
    part, gp = poisoned(n * tiles * nd * 2)
    H.call("smsut_conv1x1_fwd", x, wt, ys, part, n, hw, k, nd, 0, st)
    check("conv1x1_fwd + stats", ys, ref, FWD_BAR)
    assert torch.equal(ys, y), "the statistics epilogue must not change y"
    p = part[:n * tiles * nd * 2].view(n, tiles, nd, 2).double().sum(1).cpu()
    yd = ys.double().view(n, hw, nd).cpu()
    assert torch.allclose(p[..., 0], yd.sum(1), rtol=1e-5, atol=1e-3)
    assert torch.allclose(p[..., 1], (yd ** 2).sum(1), rtol=1e-5, atol=1e-3)
    assert untouched(gy_, gs, gp)


def test_conv1x1_statistics_refused_when_tiles_do_not_divide(H):
    n, hw, k, nd = 3, 63, 4, 16                           # MR = 1: 63 % 16 != 0
    assert H.call("smsut_conv1x1_tiles", n, hw, nd) == 0
    assert H.call("smsut_conv1x1_tiles", 2, 256 * 256 + 16, nd) == 0      # MR = 4: HW % 64 == 16
    x, wt, _ = _mk1(n, hw, 1, k, nd, 0, 15)
    ybuf, yg = guarded_out(n * hw * nd)
    pbuf, pg = guarded_out(64)
    with pytest.raises(H.SmsutHipError):
        H.call("smsut_conv1x1_fwd", x, wt, ybuf, pbuf, n, hw, k, nd, 0, H.stream_ptr())
    torch.cuda.synchronize()
    assert untouched(ybuf, pbuf), "a refused call launches nothing"


# conv1x1_wgrad_launch (conv1x1.hip:530-537): CIT = 2 when Cin > 16, COT = 2 when Cout > 16 -> (4, 4) 1x1 one ragged tile each |
# (16, 16) 1x1 exact | (12, 20) 1x2, both ragged | (32, 12) 2x1 | (20, 40) 2x2, ragged second tiles | (64, 32) 2x2, two Cin slabs.
# plan_wgrad1 (conv1x1.hip:283-293): want = min(ceil(1024 / slabs), max(P / 256, 1)), pps = ceil(P / want) rounded up to 16, splits =
# ceil(P / pps) -- with <= 4 slabs the pixel count alone decides.  sum_parts (conv1x1.hip:252-280): 16 split lanes; lane sl runs the
# four-accumulator loop while sl + 48 < splits and the single loop for the rest:
#   P 189   -> 1 split of 189 pixels (< 256: one short split)            P 12288 -> 48 splits: the last count without the first loop
#   P 3940  -> 15 splits (pps 272, last 132)                              P 12544 -> 49: lane 0 alone enters the first loop
#   P 4096  -> 16 splits of 256: every lane one single-loop trip          P 16384 -> 64: every lane one four-accumulator trip, no tail
#   P 4353  -> 17 splits of 272, the last holds ONE pixel (< a 16-pixel trip)   P 25637 -> 95: first loop, then a 16-stride tail
WGRAD1_CH = [(4, 4), (16, 16), (12, 20), (32, 12), (20, 40), (64, 32)]
WGRAD1_P = {189: 1, 3940: 15, 4096: 16, 4353: 17, 12288: 48, 12544: 49, 16384: 64, 25637: 95}


def plan1(P, ci, co):
    cit, cot = (2 if ci > 16 else 1), (2 if co > 16 else 1)
    slabs = cdiv(ci, 16 * cit) * cdiv(co, 16 * cot)
    want = max(min(cdiv(1024, slabs), max(P // 256, 1)), 1)
    pps = cdiv(cdiv(P, want), 16) * 16
    return cdiv(P, pps), pps


def _wgrad1(H, P, ci, co, ca=0, seed=16):
    st = H.stream_ptr()
    g = gen(seed)
    x, gy = rn(g, P, ci), rn(g, P, co)
    ref = x.double().t() @ gy.double()
    ws_n = H.call("smsut_conv1x1_wgrad_ws", 1, P, ci, co)
    splits, pps = plan1(P, ci, co)
    assert ws_n == splits * ci * co, "the workspace query must describe the plan this test derived"
    gw, gg = out_buf(ci, co)
    ws, wg = poisoned(ws_n)
    if ca:
        H.call("smsut_conv1x1_wgrad_cat", x[:, :ca].contiguous().cuda(), x[:, ca:].contiguous().cuda(), ca, gy.cuda(), gw, ws, 1, P, ci, co, st)
    else:
        H.call("smsut_conv1x1_wgrad", x.cuda(), gy.cuda(), gw, ws, 1, P, ci, co, st)
    check(f"conv1x1_wgrad splits {splits} pps {pps} last {P - (splits - 1) * pps}", gw, ref, WGRAD_BAR)
    assert bool(torch.isfinite(ws[:ws_n]).all()), "every slab element of every split is written"
    assert untouched(gg, wg)
    return splits, pps


@pytest.mark.parametrize("P", list(WGRAD1_P), ids=[f"P{p}-splits{s}" for p, s in WGRAD1_P.items()])
@pytest.mark.parametrize("ci,co", WGRAD1_CH, ids=[f"{a}to{b}-cit{1 + (a > 16)}cot{1 + (b > 16)}" for a, b in WGRAD1_CH])
def test_conv1x1_wgrad(H, ci, co, P):
    splits, pps = _wgrad1(H, P, ci, co)
    assert splits == WGRAD1_P[P]
    if P == 4353:
        assert P - (splits - 1) * pps == 1
    if P == 189:
        assert splits == 1 and P < 256


# cat_src (common.h:106-109) picks the tensor per 16-channel tile: ca = 16 with 4 (a one-quad tile of xb, CIT 2) or 16 channels behind
@pytest.mark.parametrize("ci,co,P", [(20, 40, 4353), (32, 12, 12544), (20, 16, 189)], ids=["16+4", "16+16", "16+4-one-split"])
def test_conv1x1_wgrad_virtual_cat(H, ci, co, P):
    _wgrad1(H, P, ci, co, ca=16, seed=17)


@pytest.mark.parametrize("ci,co", [(5, 3), (6, 5)])
@pytest.mark.parametrize("cat", [False, True], ids=["plain", "cat"])
def test_conv1x1_wgrad_refuses_slabs_that_are_not_float4s(H, ci, co, cat):
    """sum_parts reads and writes the [Cin][Cout] slabs as float4s: (Cin * Cout) % 4 != 0 is refused before anything is launched"""
    P, st = 300, H.stream_ptr()
    g = gen(18)
    x, gy = rn(g, P, 32).cuda(), rn(g, P, co).cuda()          # (x is wider than Cin: nothing here is out of bounds even if it ran)
    gw, gg = guarded_out(64)
    ws, wg = guarded_out(4096)
    with pytest.raises(H.SmsutHipError):
        if cat:
            H.call("smsut_conv1x1_wgrad_cat", x, x, 16, gy, gw, ws, 1, P, 16 + ci, co, st)
        else:
            H.call("smsut_conv1x1_wgrad", x, gy, gw, ws, 1, P, ci, co, st)
    torch.cuda.synchronize()
    assert untouched(gw, ws, gg, wg), "a refused call launches nothing"


def test_ops_conv2d_1x1_is_the_direct_call(ops, H):
    """ops.conv2d on a 1x1 layer = smsut_conv1x1_fwd / (transposed) / smsut_conv1x1_wgrad, bit for bit"""
    n, h, w, ci, co, st = 2, 16, 20, 20, 40, H.stream_ptr()
    assert H.call("smsut_conv1x1_supported", ci, co) == 1 and H.call("smsut_conv1x1_supported", co, ci) == 1
    g = gen(19)
    x, wt, gy = rn(g, n, h, w, ci).cuda(), rn(g, 1, 1, ci, co, scale=ci ** -0.5).cuda(), rn(g, n, h, w, co).cuda()
    xd, wd = x.permute(0, 3, 1, 2).requires_grad_(True), wt.permute(3, 2, 0, 1).requires_grad_(True)
    yd = ops.conv2d(xd, wd, None, 1, 0)
    yd.backward(gy.permute(0, 3, 1, 2))
    y, gx, gw = out_buf(n, h, w, co)[0], out_buf(n, h, w, ci)[0], out_buf(ci, co)[0]
    H.call("smsut_conv1x1_fwd", x, wt, y, None, n, h * w, ci, co, 0, st)
    H.call("smsut_conv1x1_fwd", gy, wt, gx, None, n, h * w, co, ci, 1, st)
    H.call("smsut_conv1x1_wgrad", x, gy, gw, poisoned(H.call("smsut_conv1x1_wgrad_ws", n, h * w, ci, co))[0], n, h * w, ci, co, st)
    assert torch.equal(yd.detach().permute(0, 2, 3, 1), y)
    assert torch.equal(xd.grad.permute(0, 2, 3, 1), gx)
    assert torch.equal(wd.grad.permute(2, 3, 1, 0).reshape(ci, co), gw)


# ================================================================================================ 2. thin heads
# thin1x1_dgrad (conv1x1.hip:305-325): one work item = (pixel, 4 wide channels), Q = Cin / 4 items per pixel, grid = ew_grid(P Q)
# capped at 2048 blocks.  thin1x1_wgrad (conv1x1.hip:330-375, launch :586-587): blocks = min(ceil(P Q / 512), 1024), a thread takes items
# i, i + stride, ... in pairs (`step(i); step(i + stride)`) with a single-step tail.  thin1x1_wsum (conv1x1.hip:379-394): float4 column
# col of the [Cin][8] slab = (ci = col / 2, half = col & 1); Cout 4 fills half 0 exactly, 5 one element of half 1, 8 both, 1 one element.
#   1 pixel            : Q items, one block, every thread at most one single step
#   7 pixels           : 7 Q <= 112 items: below one block
#   P Q = 700 + 4k     : 2 blocks, stride 512: threads below P Q - 512 take a pair, the rest the single-step tail
#   183 x 185 (Cin 64) : P = 33855 > 32768: P Q = 541680 > 1024 * 512 -> the 1024-block cap binds, stride 262144, threads below 17392 make
#                        three steps (a pair and the tail); the data-gradient grid is capped too (541680 > 2048 * 256, 541680 % 256 = 240)
THIN_CI = [8, 16, 32, 64]
THIN_CO = [1, 4, 5, 8]


def _thin(H, P, ci, co, seed=21):
    assert H.call("smsut_conv1x1_thin_supported", ci, co) == 1
    st = H.stream_ptr()
    g = gen(seed)
    x, gy, wt = rn(g, P, ci), rn(g, P, co), rn(g, ci, co, scale=ci ** -0.5)
    gx, ggx = out_buf(P, ci)
    H.call("smsut_conv1x1_thin_dgrad", gy.cuda(), wt.cuda(), gx, 1, P, ci, co, st)
    check(f"thin_dgrad P {P} {ci}->{co}", gx, gy.double() @ wt.double().t(), FWD_BAR)
    ws_n = H.call("smsut_conv1x1_thin_wgrad_ws", ci)
    assert ws_n == 1024 * ci * 8
    ws, wg = poisoned(ws_n)
    gw, ggw = out_buf(ci, co)
    H.call("smsut_conv1x1_thin_wgrad", x.cuda(), gy.cuda(), gw, ws, 1, P, ci, co, st)
    check(f"thin_wgrad P {P} {ci}->{co}", gw, x.double().t() @ gy.double(), WGRAD_BAR)
    assert untouched(ggx, wg, ggw)


@pytest.mark.parametrize("regime", ["1pixel", "below-one-block", "pair-and-tail"])
@pytest.mark.parametrize("co", THIN_CO)
@pytest.mark.parametrize("ci", THIN_CI)
def test_thin_heads(H, ci, co, regime):
    q = ci // 4
    P = {"1pixel": 1, "below-one-block": 7, "pair-and-tail": cdiv(700, q) + 1}[regime]
    if regime == "below-one-block":
        assert P * q < 256
    if regime == "pair-and-tail":
        assert 512 < P * q < 1024 and cdiv(P * q, 512) == 2
    _thin(H, P, ci, co)


@pytest.mark.parametrize("co", THIN_CO)
def test_thin_heads_block_cap(H, co):
    P, ci = 183 * 185, 64
    items = P * (ci // 4)
    assert P > 32768 and cdiv(items, 512) > 1024 and 2 * 262144 < items < 3 * 262144       # wgrad: capped, an odd number of strides
    assert items > EW_CAP_ITEMS and items % 256 != 0                                        # dgrad: capped grid, ragged last block
    _thin(H, P, ci, co, seed=22)


def test_ops_conv2d_thin_head_is_the_direct_call(ops, H):
    n, h, w, ci, co, st = 2, 9, 13, 16, 5, H.stream_ptr()
    assert H.call("smsut_conv1x1_thin_supported", ci, co) == 1
    g = gen(23)
    x, wt, gy = rn(g, n, h, w, ci).cuda(), rn(g, 1, 1, ci, co, scale=ci ** -0.5).cuda(), rn(g, n, h, w, co).cuda()
    xd, wd = x.permute(0, 3, 1, 2).requires_grad_(True), wt.permute(3, 2, 0, 1).requires_grad_(True)
    ops.conv2d(xd, wd, None, 1, 0).backward(gy.permute(0, 3, 1, 2))
    gx, gw = out_buf(n, h, w, ci)[0], out_buf(ci, co)[0]
    H.call("smsut_conv1x1_thin_dgrad", gy, wt, gx, n, h * w, ci, co, st)
    H.call("smsut_conv1x1_thin_wgrad", x, gy, gw, poisoned(H.call("smsut_conv1x1_thin_wgrad_ws", ci))[0], n, h * w, ci, co, st)
    assert torch.equal(xd.grad.permute(0, 2, 3, 1), gx)
    assert torch.equal(wd.grad.permute(2, 3, 1, 0).reshape(ci, co), gw)


# ================================================================================================ 3. ConvTranspose2d(k=2, s=2)
def convT_ref(x, wt, gy):
    """fp64: y [N,2H,2W,Co], gx [N,H,W,Ci], gw [2][2][Ci][Co] of ConvTranspose2d(k=2, s=2) on NHWC x and [kh][kw][Ci][Co] weights"""
    n, h, w, ci = x.shape
    co = wt.shape[3]
    x2, w2 = x.double().reshape(-1, ci), wt.double().permute(2, 0, 1, 3).reshape(ci, 4 * co)          # columns (a, b, co)
    y = (x2 @ w2).view(n, h, w, 2, 2, co).permute(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, co)
    g2 = gy.double().view(n, h, 2, w, 2, co).permute(0, 1, 3, 2, 4, 5).reshape(-1, 4 * co)            # rows p, columns (a, b, co)
    gx = (g2 @ w2.t()).view(n, h, w, ci)
    gw = (x2.t() @ g2).view(ci, 2, 2, co).permute(1, 2, 0, 3).contiguous()
    return y, gx, gw


def convT_branch(N, Hh, W, ndim, ntap_out, transposed):
    """dispatch_fwd<1> as the transposed conv reaches it (its launch_fwd rows, conv_mfma.hip; osc = 2 or isc = 2, so neither the 8x8-plane nor the
    `H <= 4 && isc == 1 && osc == 1` branch applies).  A restatement, checked against nothing in the library (the tile configuration
    has no query): whoever moves the wg16 >= 512 / wg8 >= 256 thresholds there must edit this function and the CONVT shapes with
    them, or the case ids name a branch the cases no longer take.  The same holds for k4_nt (smsut_conv2d_k4_fwd, conv_mfma.hip), flat_mt
    (conv_small.hip:552-556) and is_stem (conv_small.hip:429-432) below."""
    nt, tx = cdiv(ndim, 16), cdiv(W, 16)
    wg16 = tx * cdiv(Hh, 16) * N * ((nt + 1) // 2) * ntap_out
    wg8 = tx * cdiv(Hh, 8) * N * ((nt + 1) // 2) * ntap_out
    if nt == 1:
        return "nt1"
    if wg16 >= 512:
        return "16x4x1x2"
    if wg8 >= 256 and not transposed:
        return "8x4x1x2"
    return "8x4x1x1"


def plan_wgrad(N, Hh, W, ci, co, taps_k=9, tw=16, th=8):
    """plan_wgrad (conv_mfma_wgrad.hip): (cit, cot, splits, tiles_per_split)"""
    cit, cot = (2 if ci > 16 else 1), (2 if co > 16 else 1)
    total = N * cdiv(W, tw) * cdiv(Hh, th)
    slabs = cdiv(ci, 16 * cit) * cdiv(co, 16 * cot)
    want = cdiv(768 if cit == 1 and cot == 1 else 512, slabs)
    want = max(min(want, max((8 << 20) // (ci * co * taps_k), 1), total), 1)
    tps = cdiv(total, want)
    return cit, cot, cdiv(total, tps), tps


def sum_splits_form(wsize, splits):
    """launch_sum_splits (conv_mfma_wgrad.hip): columns per block by wsize, and whether a lane enters the four-accumulator loop
    (`c + 3 LANES < splits`, LANES = 256 / COLS)"""
    cols = 64 if wsize >= 32768 else (32 if wsize >= 8192 else 16)
    return f"cols{cols}-{'4acc' if splits > 3 * (256 // cols) else 'tail'}"


# Forward: Kdim = Cin, Ndim = Cout, ntap_out = 4.  Data-gradient: Kdim = Cout, Ndim = Cin, transposed, ntap_out = 1, G = 4.  With nt =
# ceil(Ndim / 16), tx = ceil(W / 16): wg16 = tx ceil(H / 16) N ceil(nt / 2) ntap_out, wg8 the same on ceil(H / 8).
#   (2,128,128,64,32)  fwd nt 2: wg16 = 8*8*2*1*4 = 512 -> <16,4,1,2> | dgrad nt 4: wg16 = 8*8*2*2 = 256, wg8 = 512 but transposed -> <8,4,1,1>
#   (2,64,64,64,32)    fwd wg16 = 4*4*2*1*4 = 128, wg8 = 256 -> <8,4,1,2> | dgrad wg16 = 64, wg8 = 128 -> <8,4,1,1>
#   (4,128,128,64,16)  fwd nt 1 | dgrad nt 4: wg16 = 8*8*4*2 = 512 -> <16,4,1,2>; wgrad: 512 tiles, want 256 -> 2 tiles per split
#   (4,64,64,64,8)     fwd nt 1 | dgrad wg16 = 4*4*4*2 = 128, wg8 = 256: the forward-only branch, a data-gradient stays on <8,4,1,1>
#   (3,20,24,12,20)    ragged plane (H % 8, W % 16 != 0), fwd nt 2: wg16 = 2*2*3*1*4 = 48, wg8 = 72 -> <8,4,1,1> with nt > 1 | dgrad nt 1
#   (3,20,24,20,12)    fwd nt 1 | dgrad nt 2 small grid -> <8,4,1,1>
#   (2,9,7,20,4), (2,9,7,4,12)   one ragged tile column, channel tails 4 / 12 / 20 on both sides: nt 1
#   (2,4,5,4,20)       a plane of H <= 4: the 4-row tile is for isc = osc = 1 only, the transposed conv stays on <8,4,1,1> (fwd nt 2)
#   (1,1,1,4,4)        one pixel
#   (2,16,16,128,64), (4,32,32,128,64), (1,16,32,64,32), (1,80,88,4,12): weight-gradient sum forms, see WGRAD_T below (the second
#                      also reaches <8,4,1,2> forward with FOUR 16-channel tiles: wg8 = 2*4*4*2*4 = 256, grid.z walks two 32-channel slabs)
CONVT = [(2, 128, 128, 64, 32, "16x4x1x2", "8x4x1x1"), (2, 64, 64, 64, 32, "8x4x1x2", "8x4x1x1"),
         (4, 128, 128, 64, 16, "nt1", "16x4x1x2"), (4, 64, 64, 64, 8, "nt1", "8x4x1x1"),
         (3, 20, 24, 12, 20, "8x4x1x1", "nt1"), (3, 20, 24, 20, 12, "nt1", "8x4x1x1"), (2, 9, 7, 20, 4, "nt1", "8x4x1x1"),
         (2, 9, 7, 4, 12, "nt1", "nt1"), (2, 4, 5, 4, 20, "8x4x1x1", "nt1"), (1, 1, 1, 4, 4, "nt1", "nt1"),
         (2, 16, 16, 128, 64, "8x4x1x1", "8x4x1x1"), (4, 32, 32, 128, 64, "8x4x1x2", "8x4x1x1"),
         (1, 16, 32, 64, 32, "8x4x1x1", "8x4x1x1"), (1, 80, 88, 4, 12, "nt1", "nt1")]
# plan_wgrad / launch_sum_splits per case: (cit x cot, splits, tiles per split, sum form) -- asserted against the *_ws query
WGRAD_T = {(2, 128, 128, 64, 32): (2, 2, 256, 1, "cols32-4acc"), (2, 64, 64, 64, 32): (2, 2, 64, 1, "cols32-4acc"),
           (4, 128, 128, 64, 16): (2, 1, 256, 2, "cols16-4acc"), (4, 64, 64, 64, 8): (2, 1, 128, 1, "cols16-4acc"),
           (3, 20, 24, 12, 20): (1, 2, 18, 1, "cols16-tail"), (3, 20, 24, 20, 12): (2, 1, 18, 1, "cols16-tail"),
           (2, 9, 7, 20, 4): (2, 1, 4, 1, "cols16-tail"), (2, 9, 7, 4, 12): (1, 1, 4, 1, "cols16-tail"),
           (2, 4, 5, 4, 20): (1, 2, 2, 1, "cols16-tail"), (1, 1, 1, 4, 4): (1, 1, 1, 1, "cols16-tail"),
           (2, 16, 16, 128, 64): (2, 2, 4, 1, "cols64-tail"), (4, 32, 32, 128, 64): (2, 2, 32, 1, "cols64-4acc"),
           (1, 16, 32, 64, 32): (2, 2, 4, 1, "cols32-tail"), (1, 80, 88, 4, 12): (1, 1, 60, 1, "cols16-4acc")}


def _convT_id(c):
    n, h, w, ci, co, fb, db = c
    p = WGRAD_T[c[:5]]
    return f"{n}x{h}x{w}-{ci}to{co}-fwd_{fb}-dgrad_{db}-wgrad_{p[0]}x{p[1]}_{p[4]}"


@pytest.mark.parametrize("case", CONVT, ids=[_convT_id(c) for c in CONVT])
def test_convT2x2_per_tap_mfma(H, case):
    n, h, w, ci, co, fwd_branch, dgrad_branch = case
    assert H.call("smsut_convT2x2_mfma_supported", ci, co) == 1
    assert convT_branch(n, h, w, co, 4, False) == fwd_branch
    assert convT_branch(n, h, w, ci, 1, True) == dgrad_branch
    st = H.stream_ptr()
    g = gen(31)
    x, wt, gy = rn(g, n, h, w, ci), rn(g, 2, 2, ci, co, scale=ci ** -0.5), rn(g, n, 2 * h, 2 * w, co)
    ry, rgx, rgw = convT_ref(x, wt, gy)
    xd, wd, gyd = x.cuda(), wt.cuda(), gy.cuda()
    y, g1 = out_buf(n, 2 * h, 2 * w, co)
    H.call("smsut_convT2x2_fwd_mfma", xd, wd, y, n, h, w, ci, co, st)
    check("convT fwd", y, ry, FWD_BAR)
    gx, g2 = out_buf(n, h, w, ci)
    H.call("smsut_convT2x2_dgrad_mfma", gyd, wd, gx, n, h, w, ci, co, st)
    check("convT dgrad", gx, rgx, FWD_BAR)
    cit, cot, splits, tps = plan_wgrad(n, h, w, ci, co)
    ws_n = H.call("smsut_convT2x2_wgrad_mfma_ws", n, h, w, ci, co)
    assert ws_n == splits * 4 * ci * co
    assert (cit, cot, splits, tps, sum_splits_form(4 * ci * co, splits)) == WGRAD_T[case[:5]]
    ws, g3 = poisoned(ws_n)
    gw, g4 = out_buf(2, 2, ci, co)
    H.call("smsut_convT2x2_wgrad_mfma", xd, gyd, gw, ws, n, h, w, ci, co, st)
    check(f"convT wgrad splits {splits} x {tps} tiles", gw, rgw, WGRAD_BAR)
    assert untouched(g1, g2, g3, g4)


def test_convT2x2_branch_table_is_covered():
    fwd, dgr = {c[5] for c in CONVT}, {c[6] for c in CONVT}
    assert fwd == {"nt1", "16x4x1x2", "8x4x1x2", "8x4x1x1"}
    assert dgr == {"nt1", "16x4x1x2", "8x4x1x1"}                      # the wg8 branch is forward-only
    n, h, w, ci, co = 4, 64, 64, 64, 8                                # ... on a shape whose grid WOULD take it
    assert convT_branch(n, h, w, ci, 1, False) == "8x4x1x2" and convT_branch(n, h, w, ci, 1, True) == "8x4x1x1"
    plans = set(WGRAD_T.values())
    assert {(p[0], p[1]) for p in plans} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert {p[4] for p in plans} == {f"cols{c}-{k}" for c in (16, 32, 64) for k in ("4acc", "tail")}
    assert {p[3] > 1 for p in plans} == {False, True}


# Pixel-shuffle form (conv1x1.hip:464-516): Cout = 16 -> Nd = 64 columns, NR = 4 (one workgroup owns all four taps), MR by P as in
# section 1; the weight image is [Cin / 16][4][64][4] floats = 256 B per input channel: 64 KiB at Cin 256, the largest the predicate
# admits.  Weight gradient: conv1x1_wgrad<CIT, 2, PS> with plan_wgrad1(P, Cin, 64, cit, 2).
#   (3,20,23,4)    MR 1, odd W: row = p / 23 off the powers of two, one partial chunk     (2,9,7,20)    MR 1, ragged second chunk
#   (2,16,16,256)  MR 1, the 64 KiB image                                                  (2,256,256,20) MR 4, P = 131072 exactly
#   (2,257,257,32) MR 4, odd W, P = 132098 = 516 * 256 + 2
CONVT_PS = [(3, 20, 23, 4), (2, 9, 7, 20), (2, 16, 16, 256), (2, 256, 256, 20), (2, 257, 257, 32)]


@pytest.mark.parametrize("n,h,w,ci", CONVT_PS, ids=[f"mr{mr_of(c[0] * c[1] * c[2])}-{c[0]}x{c[1]}x{c[2]}-{c[3]}to16" for c in CONVT_PS])
def test_convT2x2_pixel_shuffle(H, n, h, w, ci):
    co, st = 16, H.stream_ptr()
    assert H.call("smsut_convT2x2_ps_supported", ci, co) == 1 and n * h * w * 4 * co < 2 ** 31
    g = gen(32)
    x, wt, gy = rn(g, n, h, w, ci), rn(g, 2, 2, ci, co, scale=ci ** -0.5), rn(g, n, 2 * h, 2 * w, co)
    ry, _, rgw = convT_ref(x, wt, gy)
    xd, wd, gyd = x.cuda(), wt.cuda(), gy.cuda()
    y, g1 = out_buf(n, 2 * h, 2 * w, co)
    H.call("smsut_convT2x2_fwd_ps", xd, wd, y, n, h, w, ci, co, st)
    check("convT ps fwd", y, ry, FWD_BAR)
    ws_n = H.call("smsut_convT2x2_wgrad_ps_ws", n, h, w, ci, co)
    P = n * h * w
    cit = 2 if ci > 16 else 1
    slabs = cdiv(ci, 16 * cit) * 2
    want = max(min(cdiv(1024, slabs), max(P // 256, 1)), 1)
    pps = cdiv(cdiv(P, want), 16) * 16
    assert ws_n == cdiv(P, pps) * ci * 64
    ws, g2 = poisoned(ws_n)
    gw, g3 = out_buf(2, 2, ci, co)
    H.call("smsut_convT2x2_wgrad_ps", xd, gyd, gw, ws, n, h, w, ci, co, st)
    check(f"convT ps wgrad splits {cdiv(P, pps)}", gw, rgw, WGRAD_BAR)
    # the per-tap MFMA kernels compute the same operation independently
    assert H.call("smsut_convT2x2_mfma_supported", ci, co) == 1
    y2, g4 = out_buf(n, 2 * h, 2 * w, co)
    H.call("smsut_convT2x2_fwd_mfma", xd, wd, y2, n, h, w, ci, co, st)
    check("convT ps fwd vs per-tap", y, y2.double().cpu(), FWD_BAR)
    ws2, g5 = poisoned(H.call("smsut_convT2x2_wgrad_mfma_ws", n, h, w, ci, co))
    gw2, g6 = out_buf(2, 2, ci, co)
    H.call("smsut_convT2x2_wgrad_mfma", xd, gyd, gw2, ws2, n, h, w, ci, co, st)
    check("convT ps wgrad vs per-tap", gw, gw2.double().cpu(), WGRAD_BAR)
    assert untouched(g1, g2, g3, g4, g5, g6)


def test_convT2x2_pixel_shuffle_predicate_matches_its_launch(ops, H):
    """the pixel-shuffle forward asks for 256 B of LDS per input channel: the predicate stops at the 64 KiB image (Cin 256), and
    a 512-channel layer goes through ops.conv_transpose2x2 to the per-tap kernels"""
    assert H.call("smsut_convT2x2_ps_supported", 256, 16) == 1
    assert H.call("smsut_convT2x2_ps_supported", 260, 16) == 0 and H.call("smsut_convT2x2_ps_supported", 512, 16) == 0
    assert H.call("smsut_convT2x2_ps_supported", 32, 32) == 0
    n, h, w, ci, co, st = 1, 8, 8, 512, 16, H.stream_ptr()
    assert H.call("smsut_convT2x2_mfma_supported", ci, co) == 1
    g = gen(33)
    x, wt, gy = rn(g, n, h, w, ci), rn(g, 2, 2, ci, co, scale=ci ** -0.5), rn(g, n, 2 * h, 2 * w, co)
    ry, rgx, rgw = convT_ref(x, wt, gy)
    ybuf, yg = guarded_out(n * 4 * h * w * co)
    with pytest.raises(H.SmsutHipError):
        H.call("smsut_convT2x2_fwd_ps", x.cuda(), wt.cuda(), ybuf, n, h, w, ci, co, st)
    torch.cuda.synchronize()
    assert untouched(ybuf, yg)
    xd, wd = x.cuda().permute(0, 3, 1, 2).requires_grad_(True), wt.cuda().permute(2, 3, 0, 1).requires_grad_(True)
    yd = ops.conv_transpose2x2(xd, wd)
    yd.backward(gy.cuda().permute(0, 3, 1, 2))
    check("ops convT 512->16 fwd", yd.detach().permute(0, 2, 3, 1), ry, FWD_BAR)
    check("ops convT 512->16 dgrad", xd.grad.permute(0, 2, 3, 1), rgx, FWD_BAR)
    check("ops convT 512->16 wgrad", wd.grad.permute(2, 3, 0, 1), rgw, WGRAD_BAR)


@pytest.mark.parametrize("ci,co,form", [(64, 32, "mfma"), (32, 16, "ps")])
def test_ops_conv_transpose2x2_is_the_direct_call(ops, H, ci, co, form):
    n, h, w, st = 2, 12, 20, H.stream_ptr()
    assert H.call("smsut_convT2x2_ps_supported", ci, co) == (form == "ps") and H.call("smsut_convT2x2_mfma_supported", ci, co) == 1
    g = gen(34)
    x, wt, gy = rn(g, n, h, w, ci).cuda(), rn(g, 2, 2, ci, co, scale=ci ** -0.5).cuda(), rn(g, n, 2 * h, 2 * w, co).cuda()
    xd, wd = x.permute(0, 3, 1, 2).requires_grad_(True), wt.permute(2, 3, 0, 1).requires_grad_(True)
    yd = ops.conv_transpose2x2(xd, wd)
    yd.backward(gy.permute(0, 3, 1, 2))
    y, gx, gw = out_buf(n, 2 * h, 2 * w, co)[0], out_buf(n, h, w, ci)[0], out_buf(2, 2, ci, co)[0]
    H.call(f"smsut_convT2x2_fwd_{form}", x, wt, y, n, h, w, ci, co, st)
    H.call("smsut_convT2x2_dgrad_mfma", gy, wt, gx, n, h, w, ci, co, st)
    H.call(f"smsut_convT2x2_wgrad_{form}", x, gy, gw, poisoned(H.call(f"smsut_convT2x2_wgrad_{form}_ws", n, h, w, ci, co))[0],
           n, h, w, ci, co, st)
    assert torch.equal(yd.detach().permute(0, 2, 3, 1), y)
    assert torch.equal(xd.grad.permute(0, 2, 3, 1), gx)
    assert torch.equal(wd.grad.permute(2, 3, 0, 1), gw)


# ================================================================================================ 4. 4x4 stride 1 pad 1
# smsut_conv2d_k4_fwd (conv_mfma.hip): NT = 2 (32-channel slabs) when Ndim % 32 == 0 || Ndim > 16, else NT = 1; forward Ndim =
# Cout, Kdim = Cin, tiles over the (H-1) x (W-1) output; transposed Ndim = Cin, Kdim = Cout, pad 2, tiles over the H x W result.  Tiles
# are 8 x 16.  The channel pairs give, forward | transposed:  Ndim 4, 16 -> NT 1;  20, 24 -> NT 2 with a ragged slab;  32 -> NT 2 exact;
# 48 -> NT 2, ragged second slab;  64 -> two slabs.  Kdim 4: one partial chunk, 20: a partial second chunk, 64: four chunks.
# Planes (H, W of the forward input): 2x2 -> a 1x1 output (every halo read is masked by in_off = -1 in conv_k4_fwd, conv_mfma.hip; the store by
# gy_ < Ho, gx_ < Wo in its epilogue) | 2x9 -> one output row | 9x10 -> output 8x9: one tile, exactly full rows | 17x33 -> output 16x32: 2 x 2
# exactly full tiles forward, 3 x 3 tiles with one row and one column in the last ones transposed | 10x18 -> output 9x17: one row and one
# column into the next tile forward.
K4_CH = [(4, 4), (20, 16), (64, 20), (4, 24), (20, 32), (64, 48), (16, 4), (24, 20), (32, 64), (48, 4)]
K4_PLANES = [(2, 2), (2, 9), (9, 10), (17, 33), (10, 18)]


def k4_nt(ndim):
    return 2 if (ndim % 32 == 0 or ndim > 16) else 1


def plan_k4(N, Hh, W, ci, co):
    """plan_wgrad_k4 (conv_mfma_wgrad.hip): (cot, splits, tiles_per_split)"""
    cot = 2 if co > 16 else 1
    total = N * cdiv(W - 1, 16) * cdiv(Hh - 1, 8)
    slabs = cdiv(ci, 16) * cdiv(co, 16 * cot)
    want = max(min(cdiv(512, slabs), max((8 << 20) // (ci * co * 16), 1), total), 1)
    tps = cdiv(total, want)
    return cot, cdiv(total, tps), tps, total


def _k4(H, n, h, w, ci, co, seed=41):
    assert H.call("smsut_conv2d_k4_supported", ci, co) == 1
    st = H.stream_ptr()
    g = gen(seed)
    x, wt, gy = rn(g, n, h, w, ci), rn(g, 4, 4, ci, co, scale=(16 * ci) ** -0.5), rn(g, n, h - 1, w - 1, co)
    ry, rgx, rgw, _ = conv_ref(x, wt, None, 1, 1, gy)
    xd, wd, gyd = x.cuda(), wt.cuda(), gy.cuda()
    y, g1 = out_buf(n, h - 1, w - 1, co)
    H.call("smsut_conv2d_k4_fwd", xd, wd, y, n, h, w, ci, co, 0, st)
    check(f"k4 fwd NT{k4_nt(co)}", y, ry, FWD_BAR)
    gx, g2 = out_buf(n, h, w, ci)
    H.call("smsut_conv2d_k4_fwd", gyd, wd, gx, n, h, w, ci, co, 1, st)
    check(f"k4 dgrad NT{k4_nt(ci)}", gx, rgx, FWD_BAR)
    cot, splits, tps, total = plan_k4(n, h, w, ci, co)
    ws_n = H.call("smsut_conv2d_k4_wgrad_ws", n, h, w, ci, co)
    assert ws_n == splits * 16 * ci * co
    ws, g3 = poisoned(ws_n)
    gw, g4 = out_buf(4, 4, ci, co)
    H.call("smsut_conv2d_k4_wgrad", xd, gyd, gw, ws, n, h, w, ci, co, st)
    check(f"k4 wgrad cot{cot} splits {splits} x {tps} of {total}", gw, rgw, WGRAD_BAR)
    assert untouched(g1, g2, g3, g4)
    return cot, splits, tps, total


@pytest.mark.parametrize("h,w", K4_PLANES, ids=[f"{a}x{b}" for a, b in K4_PLANES])
@pytest.mark.parametrize("ci,co", K4_CH, ids=[f"{a}to{b}-fwdNT{k4_nt(b)}-dgradNT{k4_nt(a)}" for a, b in K4_CH])
def test_conv_k4(H, ci, co, h, w):
    cot, splits, tps, total = _k4(H, 2, h, w, ci, co)
    assert splits == total and tps == 1                  # small problems: one tile per split


def test_conv_k4_table_is_covered():
    assert {co for ci, co in K4_CH} >= {4, 16, 20, 24, 32, 48} and {ci for ci, co in K4_CH} >= {4, 16, 20, 24, 32, 48}
    assert {ci for ci, co in K4_CH} >= {4, 20, 64} and {co for ci, co in K4_CH} >= {4, 20, 64}


# plan_wgrad_k4: want = min(ceil(512 / slabs), total).  (1, 2x2): total = 1 -> one split of one tile | (5, 41x49, 64 -> 48): cot 2, slabs
# 4 * 2 = 8, want 64, total 5 * 5 * 3 = 75 -> 2 tiles per split, 38 splits, the last holds one | (9, 41x49, 64 -> 16): cot 1, slabs 4,
# want 128, total 135 -> 2 tiles per split, 68 splits, the last holds one
@pytest.mark.parametrize("n,h,w,ci,co,want", [(1, 2, 2, 20, 24, (2, 1, 1, 1)), (5, 41, 49, 64, 48, (2, 38, 2, 75)),
                                              (9, 41, 49, 64, 16, (1, 68, 2, 135))],
                         ids=["total1", "cot2-2tiles-short-last", "cot1-2tiles-short-last"])
def test_conv_k4_wgrad_plans(H, n, h, w, ci, co, want):
    assert _k4(H, n, h, w, ci, co, seed=42) == want


def test_ops_conv2d_k4_is_the_direct_call(ops, H):
    n, h, w, ci, co, st = 2, 10, 18, 20, 24, H.stream_ptr()
    assert H.call("smsut_conv2d_k4_supported", ci, co) == 1
    g = gen(43)
    x, wt, gy = rn(g, n, h, w, ci).cuda(), rn(g, 4, 4, ci, co, scale=(16 * ci) ** -0.5).cuda(), rn(g, n, h - 1, w - 1, co).cuda()
    xd, wd = x.permute(0, 3, 1, 2).requires_grad_(True), wt.permute(3, 2, 0, 1).requires_grad_(True)
    yd = ops.conv2d(xd, wd, None, 1, 1)
    yd.backward(gy.permute(0, 3, 1, 2))
    y, gx, gw = out_buf(n, h - 1, w - 1, co)[0], out_buf(n, h, w, ci)[0], out_buf(4, 4, ci, co)[0]
    H.call("smsut_conv2d_k4_fwd", x, wt, y, n, h, w, ci, co, 0, st)
    H.call("smsut_conv2d_k4_fwd", gy, wt, gx, n, h, w, ci, co, 1, st)
    H.call("smsut_conv2d_k4_wgrad", x, gy, gw, poisoned(H.call("smsut_conv2d_k4_wgrad_ws", n, h, w, ci, co))[0], n, h, w, ci, co, st)
    assert torch.equal(yd.detach().permute(0, 2, 3, 1), y)
    assert torch.equal(xd.grad.permute(0, 2, 3, 1), gx)
    assert torch.equal(wd.grad.permute(2, 3, 1, 0), gw)


# ================================================================================================ 5. small-channel direct kernels
def osz(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def _direct(H, family, n, h, w, ci, co, kh, kw, s, p, bias, seed, wgrad="auto"):
    """forward, data-gradient and weight gradient of one conv through the `small` or the `generic` entry points against fp64; the
    weight gradient of a `small` shape is the flattened-M kernel where its predicate admits the shape and the naive one elsewhere,
    as in ops._conv_wgrad_launch (k4 s2 / k3 s2 with Cin 8: the staged tile exceeds MAXT; k5 with Cin 8: 200 rows > 128)"""
    st = H.stream_ptr()
    ho, wo = osz(h, kh, s, p), osz(w, kw, s, p)
    g = gen(seed)
    x, wt, gy = rn(g, n, h, w, ci), rn(g, kh, kw, ci, co, scale=(kh * kw * ci) ** -0.5), rn(g, n, ho, wo, co)
    b = rn(g, co) if bias else None
    ry, rgx, rgw, _ = conv_ref(x, wt, b, s, p, gy)
    xd, wd, gyd, bd = x.cuda(), wt.cuda(), gy.cuda(), (b.cuda() if bias else None)
    y, g1 = out_buf(n, ho, wo, co)
    gx, g2 = out_buf(n, h, w, ci)
    gw, g3 = out_buf(kh, kw, ci, co)
    if family == "small":
        assert kh == kw and H.call("smsut_conv2d_small_supported", kh, ci, co) == 1
        H.call("smsut_conv2d_small_fwd", xd, wd, bd, y, n, h, w, ci, ho, wo, co, kh, s, p, st)
        H.call("smsut_conv2d_small_dgrad", gyd, wd, gx, n, h, w, ci, ho, wo, co, kh, s, p, st)
    else:
        H.call("smsut_conv2d_fwd_generic", xd, wd, bd, y, n, h, w, ci, ho, wo, co, kh, kw, s, p, st)
        H.call("smsut_conv2d_dgrad_generic", gyd, wd, gx, n, h, w, ci, ho, wo, co, kh, kw, s, p, st)
    check(f"{family} fwd", y, ry, FWD_BAR)
    check(f"{family} dgrad", gx, rgx, FWD_BAR)
    if family == "small" and wgrad and H.call("smsut_conv2d_flat_wgrad_supported", kh, s, ci, co) == 1:
        ws_n = H.call("smsut_conv2d_flat_wgrad_ws", n, ho, wo, ci, co, kh)
        ws, g4 = poisoned(ws_n)
        H.call("smsut_conv2d_flat_wgrad", xd, gyd, gw, ws, n, h, w, ci, ho, wo, co, kh, s, p, st)
        check(f"flat wgrad MT{flat_mt(kh, ci)}", gw, rgw, WGRAD_BAR)
        assert untouched(g3, g4)
    elif wgrad:
        ws_n = H.call("smsut_conv2d_wgrad_generic_ws", n, ho, wo, ci, co, kh, kw)
        ws, g4 = poisoned(ws_n)
        H.call("smsut_conv2d_wgrad_generic", xd, gyd, gw, ws, n, h, w, ci, ho, wo, co, kh, kw, s, p, st)
        check("generic wgrad", gw, rgw, WGRAD_BAR)
        assert untouched(g3, g4)
    assert untouched(g1, g2)


def flat_mt(k, ci):
    m = cdiv(k * k * ci, 16)
    return 1 if m <= 1 else (2 if m <= 2 else (4 if m <= 4 else 8))


def is_stem(h, w, ci, co, k, s, p):
    return k == 5 and s == 1 and p == 2 and co == 8 and ci in (1, 5) and h % 16 == 0 and w % 64 == 0


# smsut_conv2d_small_fwd / _dgrad (conv_small.hip:467-514): CQ = Cout / 4 selects small_fwd<1..4> / small_dgrad<1..4, S1>, S1 = (stride
# == 1) drops the `% stride` tests; weights live in LDS, KS^2 Cin Cout <= MAXW = 2048 floats.  Geometries (none is a stem shape:
# stem_shape needs H % 16 == 0 and W % 64 == 0):
#   k4 s2 p1 on 33x31 -> 16x15: odd planes, the `% stride` path of small_dgrad, the last input row / column reached by one tap only
#   k3 s2 p0 on 9x10  -> 4x4 : Wo = (10 - 3) / 2 + 1 is a floor, the last input column belongs to no output
#   k5 s1 p2 on 13x21 -> same: the S1 form off the stems' 16 x 64 tiles
#   k1 s1 p0 on 7x9 with Cin 5: a 1x1 layer that smsut_conv1x1_supported refuses (Cin % 4 != 0)
# x Cout 4 / 8 / 12 / 16 (CQ 1-4) x Cin 1 / 3 / 8, wherever the weights fit; bias on the odd (Cin + CQ).
SMALL_GEOM = [(4, 2, 1, 33, 31), (3, 2, 0, 9, 10), (5, 1, 2, 13, 21)]
SMALL = [(k, s, p, h, w, ci, co) for k, s, p, h, w in SMALL_GEOM for co in (4, 8, 12, 16) for ci in (1, 3, 8) if k * k * ci * co <= 2048]
SMALL += [(1, 1, 0, 7, 9, 5, co) for co in (4, 8, 12, 16)]


@pytest.mark.parametrize("k,s,p,h,w,ci,co", SMALL, ids=[f"k{c[0]}s{c[1]}p{c[2]}-{c[3]}x{c[4]}-{c[5]}to{c[6]}-CQ{c[6] // 4}" for c in SMALL])
def test_small_channel_kernels(H, k, s, p, h, w, ci, co):
    assert not is_stem(h, w, ci, co, k, s, p)
    if k == 1:
        assert H.call("smsut_conv1x1_supported", ci, co) == 0
    _direct(H, "small", 3, h, w, ci, co, k, k, s, p, bias=(ci + co // 4) % 2 == 1, seed=51)


def test_small_channel_table_is_covered():
    for k, s, p, h, w in SMALL_GEOM:
        assert {c[6] for c in SMALL if c[0] == k} == {4, 8, 12, 16}
        assert {c[5] for c in SMALL if c[0] == k} == {1, 3, 8}
    assert (4, 2, 1, 33, 31, 8, 16) in SMALL                     # 4 * 4 * 8 * 16 = 2048 = MAXW exactly


def test_small_channel_maxw_boundary(H):
    """4x4, 8 -> 16 is 2048 weights = MAXW and runs on the small kernels (SMALL above); 5x5, 8 -> 16 is 3200: refused by the predicate and
    by the entry point, and taken by the naive kernels"""
    assert H.call("smsut_conv2d_small_supported", 4, 8, 16) == 1
    assert H.call("smsut_conv2d_small_supported", 5, 8, 16) == 0
    n, h, w, st = 2, 9, 11, H.stream_ptr()
    g = gen(52)
    x, wt = rn(g, n, h, w, 8).cuda(), rn(g, 5, 5, 8, 16).cuda()
    ybuf, yg = guarded_out(n * h * w * 16)
    with pytest.raises(H.SmsutHipError):
        H.call("smsut_conv2d_small_fwd", x, wt, None, ybuf, n, h, w, 8, h, w, 16, 5, 1, 2, st)
    torch.cuda.synchronize()
    assert untouched(ybuf, yg)
    _direct(H, "generic", n, h, w, 8, 16, 5, 5, 1, 2, bias=True, seed=52)


def test_small_channel_capped_grid(H):
    """grid = 2 ew_grid(pixels) (conv_small.hip:472,496): 1 x 1025 x 1031 = 1056775 pixels is past the 2 * 2048 * 256 threads of the
    capped grid by 8199, not a multiple of 256: the grid-stride loop makes a second, ragged trip; forward and data-gradient"""
    n, h, w = 1, 1025, 1031
    px = n * h * w
    assert px > 2 * EW_CAP_ITEMS and (px - 2 * EW_CAP_ITEMS) % 256 != 0
    _direct(H, "small", n, h, w, 1, 4, 3, 3, 1, 1, bias=True, seed=53, wgrad=None)


# smsut_conv2d_flat_wgrad (conv_small.hip:527-561): MT = ceil(KS^2 Cin / 16) rounded up to 1 / 2 / 4 / 8 M-tiles of the flattened (tap, ci)
# dimension; flat_plan (:447-456): 8 x 16 output tiles, want = min(total, 2048), tiles_per_split = ceil(total / want).
#   k3 Cin 1 -> 9 rows, MT 1 | k4 Cin 1 s2 -> 16 rows, MT 1 exactly | k5 Cin 1 -> 25, MT 2 | k5 Cin 2 -> 50, MT 4 | k5 Cin 5 -> 125, MT 8
#   (on 13x21 / Cout 16: not a stem).  One single-tile problem (1 x 8 x 16 outputs), and 5 x 264 x 272 (264 % 16 = 8: not a stem), 1 -> 8,
#   k5 p2: 5 * 33 * 17 = 2805 tiles > 2048 -> 2 tiles per split, 1403 splits, the last holds one.
FLAT = [pytest.param(3, 13, 21, 1, 8, 3, 1, 1, id="rows9-MT1"), pytest.param(3, 33, 31, 1, 16, 4, 2, 1, id="rows16-MT1"),
        pytest.param(3, 13, 21, 1, 4, 5, 1, 2, id="rows25-MT2"), pytest.param(3, 13, 21, 2, 12, 5, 1, 2, id="rows50-MT4"),
        pytest.param(3, 13, 21, 5, 16, 5, 1, 2, id="rows125-MT8"), pytest.param(1, 8, 16, 3, 8, 3, 1, 1, id="single-tile-rows27-MT2")]


@pytest.mark.parametrize("n,h,w,ci,co,k,s,p", FLAT)
def test_flat_wgrad(H, n, h, w, ci, co, k, s, p, request):
    assert not is_stem(h, w, ci, co, k, s, p) and f"MT{flat_mt(k, ci)}" in request.node.callspec.id
    st = H.stream_ptr()
    ho, wo = osz(h, k, s, p), osz(w, k, s, p)
    total = n * cdiv(ho, 8) * cdiv(wo, 16)
    assert H.call("smsut_conv2d_flat_wgrad_supported", k, s, ci, co) == 1
    ws_n = H.call("smsut_conv2d_flat_wgrad_ws", n, ho, wo, ci, co, k)
    assert total <= 2048 and ws_n == total * k * k * ci * co         # one tile per split
    if "single-tile" in request.node.callspec.id:
        assert total == 1
    g = gen(54)
    x, gy = rn(g, n, h, w, ci), rn(g, n, ho, wo, co)
    _, _, rgw, _ = conv_ref(x, torch.zeros(k, k, ci, co), None, s, p, gy)
    ws, g1 = poisoned(ws_n)
    gw, g2 = out_buf(k, k, ci, co)
    H.call("smsut_conv2d_flat_wgrad", x.cuda(), gy.cuda(), gw, ws, n, h, w, ci, ho, wo, co, k, s, p, st)
    check("flat wgrad", gw, rgw, WGRAD_BAR)
    assert untouched(g1, g2)


def test_flat_wgrad_two_tiles_per_split(H):
    n, h, w, ci, co, k, s, p = 5, 264, 272, 1, 8, 5, 1, 2
    assert not is_stem(h, w, ci, co, k, s, p)
    st = H.stream_ptr()
    total = n * cdiv(h, 8) * cdiv(w, 16)
    tps = cdiv(total, 2048)
    splits = cdiv(total, tps)
    assert (total, tps, splits) == (2805, 2, 1403) and total - (splits - 1) * tps == 1
    assert H.call("smsut_conv2d_flat_wgrad_supported", k, s, ci, co) == 1
    ws_n = H.call("smsut_conv2d_flat_wgrad_ws", n, h, w, ci, co, k)
    assert ws_n == splits * k * k * ci * co
    g = gen(55)
    x, gy = rn(g, n, h, w, ci), rn(g, n, h, w, co)
    _, _, rgw, _ = conv_ref(x, torch.zeros(k, k, ci, co), None, s, p, gy)
    ws, g1 = poisoned(ws_n)
    gw, g2 = out_buf(k, k, ci, co)
    H.call("smsut_conv2d_flat_wgrad", x.cuda(), gy.cuda(), gw, ws, n, h, w, ci, h, w, co, k, s, p, st)
    check("flat wgrad 2 tiles per split", gw, rgw, WGRAD_BAR)
    assert untouched(g1, g2)


def _ops_conv(ops, H, n, h, w, ci, co, kh, kw, s, p, seed):
    """ops.conv2d with a bias, forward and backward, in the kernels' layouts: (x, wt, b, gy, y, gx, gw)"""
    g = gen(seed)
    ho, wo = osz(h, kh, s, p), osz(w, kw, s, p)
    x, wt = rn(g, n, h, w, ci).cuda(), rn(g, kh, kw, ci, co, scale=(kh * kw * ci) ** -0.5).cuda()
    b, gy = rn(g, co).cuda(), rn(g, n, ho, wo, co).cuda()
    xd, wd = x.permute(0, 3, 1, 2).requires_grad_(True), wt.permute(3, 2, 0, 1).requires_grad_(True)
    yd = ops.conv2d(xd, wd, b, s, p)
    yd.backward(gy.permute(0, 3, 1, 2))
    return x, wt, b, gy, yd.detach().permute(0, 2, 3, 1), xd.grad.permute(0, 2, 3, 1), wd.grad.permute(2, 3, 1, 0)


def test_ops_conv2d_small_channel_is_the_direct_call(ops, H):
    n, h, w, ci, co, k, s, p, st = 3, 33, 31, 1, 4, 4, 2, 1, H.stream_ptr()
    assert H.call("smsut_conv2d_small_supported", k, ci, co) == 1 and H.call("smsut_conv2d_flat_wgrad_supported", k, s, ci, co) == 1
    ho, wo = osz(h, k, s, p), osz(w, k, s, p)
    x, wt, b, gy, yo, gxo, gwo = _ops_conv(ops, H, n, h, w, ci, co, k, k, s, p, 56)
    y, gx, gw = out_buf(n, ho, wo, co)[0], out_buf(n, h, w, ci)[0], out_buf(k, k, ci, co)[0]
    H.call("smsut_conv2d_small_fwd", x, wt, b, y, n, h, w, ci, ho, wo, co, k, s, p, st)
    H.call("smsut_conv2d_small_dgrad", gy, wt, gx, n, h, w, ci, ho, wo, co, k, s, p, st)
    H.call("smsut_conv2d_flat_wgrad", x, gy, gw, poisoned(H.call("smsut_conv2d_flat_wgrad_ws", n, ho, wo, ci, co, k))[0],
           n, h, w, ci, ho, wo, co, k, s, p, st)
    assert torch.equal(yo, y) and torch.equal(gxo, gx) and torch.equal(gwo, gw)


# ================================================================================================ 6. naive fallbacks
# conv_fwd_naive / conv_dgrad_naive / conv_wgrad_partial (conv_naive.hip:22-129) index the weights as (kh * KW + kw): a KH != KW kernel
# shows a swapped extent; stride 2 takes the `% stride` tests of the data-gradient; Cout 10 the scalar loop of the data-gradient (Cout % 4
# != 0), Cout 8 its float4 loop.  None of the planes equals the kernel (the full-window form is D's classifier, tested with the networks).
NAIVE = [pytest.param(2, 9, 14, 6, 10, 1, 3, 2, 0, True, id="1x3-s2-cout10-bias"),
         pytest.param(2, 14, 9, 3, 8, 3, 1, 2, 0, False, id="3x1-s2-cout8"),
         pytest.param(3, 7, 6, 5, 10, 3, 3, 1, 1, True, id="3x3-s1-p1-cout10-bias")]


@pytest.mark.parametrize("n,h,w,ci,co,kh,kw,s,p,bias", NAIVE)
def test_naive_kernels(H, n, h, w, ci, co, kh, kw, s, p, bias):
    _direct(H, "generic", n, h, w, ci, co, kh, kw, s, p, bias, seed=61)


def test_ops_conv2d_naive_is_the_direct_call(ops, H):
    n, h, w, ci, co, kh, kw, s, p, st = 2, 9, 14, 6, 10, 1, 3, 2, 0, H.stream_ptr()
    ho, wo = osz(h, kh, s, p), osz(w, kw, s, p)
    x, wt, b, gy, yo, gxo, gwo = _ops_conv(ops, H, n, h, w, ci, co, kh, kw, s, p, 62)
    y, gx, gw = out_buf(n, ho, wo, co)[0], out_buf(n, h, w, ci)[0], out_buf(kh, kw, ci, co)[0]
    H.call("smsut_conv2d_fwd_generic", x, wt, b, y, n, h, w, ci, ho, wo, co, kh, kw, s, p, st)
    H.call("smsut_conv2d_dgrad_generic", gy, wt, gx, n, h, w, ci, ho, wo, co, kh, kw, s, p, st)
    H.call("smsut_conv2d_wgrad_generic", x, gy, gw, poisoned(H.call("smsut_conv2d_wgrad_generic_ws", n, ho, wo, ci, co, kh, kw))[0],
           n, h, w, ci, ho, wo, co, kh, kw, s, p, st)
    assert torch.equal(yo, y) and torch.equal(gxo, gx) and torch.equal(gwo, gw)
