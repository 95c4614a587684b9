"""The 5x5 stem kernels (``csrc/conv_small.hip``: ``stem_fwd<1 / 5>``, ``stem_dgrad1``, ``stem_wgrad<1 / 5>``) through their C-ABI
entry points against fp64, on every image, tile seam and slab.  Cases, the restated launch plan and the references are in
``stem_cases.py``; ``test_stem_cases_cpu.py`` proves, without a GPU, what each case claims to reach.  The shapes A-F run both
templates of every stem kernel with 1, 2 and 3 tiles per workgroup: E (171 x 48 x 64) is tpw 2 / nwg 257 with a one-tile last workgroup,
F (205 x 16 x 320) tpw 3 / nwg 342 with workgroups that straddle images.  Two planes one step outside the predicate (24 x 64, 16 x 96) get the
same comparisons on ``small_fwd`` / ``small_dgrad`` / ``flat_wgrad``, so the dispatch boundary is pinned from both sides.

Outputs are NaN inside with a sentinel guard behind them, a workspace is exactly its ``_ws`` query, NaN inside, guard behind.

  integer   bit equality with fp64 on every element of every image (conditions: ``stem_cases.integer_conditions``)
  one-hot   a one-hot weight copies the shifted plane / a one-hot gradient pixel reads its 5x5 window, bit for bit, tap by tap
  float     |got - ref64| <= (K + 2) 2^-24 A elementwise (K = 25 Cin + 1 forward, 200 data-gradient; A = the convolution of the absolute
            values in fp64) and ``conftest.rel_err`` below the bars of ``test_conv_families_gpu.py``: 1e-5 forward / data-gradient,
            5e-5 weight gradient

Measured on an MI355X (``test_float_operands_against_fp64``; "bound" = max over the elements of |got - ref64| / ((K + 2) 2^-24 A), which
must stay <= 1; the others are rel_err against their bar):

    case Cin | fwd bound  dgrad bound | fwd rel_err  dgrad rel_err (bar 1e-5) | wgrad rel_err (bar 5e-5)
    A    1   |   0.136      0.0116    |  1.62e-07     4.47e-07               |  7.86e-08
    A    5   |   0.0361     0.0184    |  4.94e-07     4.53e-07               |  1.19e-07
    B    1   |   0.177      0.0157    |  2.01e-07     4.22e-07               |  9.02e-08
    B    5   |   0.0418     0.0182    |  5.36e-07     4.49e-07               |  1.63e-07
    C    1   |   0.189      0.0165    |  3.13e-07     5.34e-07               |  1.17e-07
    C    5   |   0.0573     0.0186    |  6.61e-07     4.68e-07               |  1.03e-07
    D    1   |   0.169      0.0120    |  3.31e-07     4.02e-07               |  1.09e-07
    D    5   |   0.0304     0.0170    |  3.64e-07     4.62e-07               |  1.47e-07
    E    1   |   0.236      0.0228    |  2.22e-07     5.90e-07               |  1.09e-07
    E    5   |   0.0676     0.0285    |  6.37e-07     6.15e-07               |  1.76e-07
    F    1   |   0.208      0.0241    |  2.47e-07     4.91e-07               |  1.52e-07
    F    5   |   0.0605     0.0268    |  4.80e-07     5.41e-07               |  1.65e-07

The largest figure is 0.236 of its bound (forward, E, Cin 1: within a factor of 4.3 of the elementwise bound, which is a worst-case
bound that an fma chain of 26 terms is expected to approach); every rel_err is more than 15 x below its bar, none within a factor of 4.
"""
import pytest
import torch

import stem_cases as C
from conv_edge_helpers import check, out_buf, poisoned, untouched
from test_conv_families_gpu import FWD_BAR, WGRAD_BAR

pytestmark = pytest.mark.gpu

SHAPES = list(C.ALL)
STEM = list(C.STEM)


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


@pytest.fixture(scope="module")
def bank():
    """operands on the device and their fp64 references, built once per (family, case, Cin) and never written"""
    store = {}

    def get(family, cid, ci):
        key = (family, cid, ci)
        if key not in store:
            mk = C.integer_operands if family == "integer" else C.float_operands
            dev = {k: v.cuda() for k, v in mk(cid, ci).items()}
            store[key] = {"ops": dev, "refs": C.refs64(dev), "y_nobias": C.fwd64(dev["x"], dev["w"])}
        return store[key]
    return get


def run_fwd(H, cid, ci, x, wt, b):
    n, h, w = C.ALL[cid]
    y, guard = out_buf(n, h, w, C.CO)
    H.call("smsut_conv2d_small_fwd", x, wt, b, y, n, h, w, ci, h, w, C.CO, C.KS, 1, C.PAD, H.stream_ptr())
    return y, guard


def run_dgrad(H, cid, ci, gy, wt):
    n, h, w = C.ALL[cid]
    gx, guard = out_buf(n, h, w, ci)
    H.call("smsut_conv2d_small_dgrad", gy, wt, gx, n, h, w, ci, h, w, C.CO, C.KS, 1, C.PAD, H.stream_ptr())
    return gx, guard


def run_wgrad(H, cid, ci, x, gy, fill=None):
    """(gw, workspace, guards); the workspace is exactly the query, NaN inside (or `fill`)"""
    n, h, w = C.ALL[cid]
    assert H.call("smsut_conv2d_flat_wgrad_supported", C.KS, 1, ci, C.CO) == 1
    ws_n = H.call("smsut_conv2d_flat_wgrad_ws", n, h, w, ci, C.CO, C.KS)
    assert ws_n == C.flat_ws(n, h, w, ci), "the workspace query must describe the plan stem_cases restates"
    ws, g1 = poisoned(ws_n)
    if fill is not None:
        ws[:ws_n] = fill
    gw, g2 = out_buf(C.KS, C.KS, ci, C.CO)
    H.call("smsut_conv2d_flat_wgrad", x, gy, gw, ws, n, h, w, ci, h, w, C.CO, C.KS, 1, C.PAD, H.stream_ptr())
    return gw, ws[:ws_n], (g1, g2)


def assert_plane_equal(tag, cid, got, ref):
    idx = C.first_mismatch(got, ref)
    if idx is not None:
        pytest.fail(f"{tag} {cid}: first mismatch at {C.where(cid, idx)}: got {float(got[idx])!r}, fp64 gives {float(ref[idx])!r}; "
                    f"{int(((got != ref) | torch.isnan(got)).sum())} of {got.numel()} elements differ")


def assert_taps_equal(tag, cid, got, ref):
    idx = C.first_mismatch(got, ref)
    if idx is not None:
        kh, kw, ci, co = idx
        pytest.fail(f"{tag} {cid}: first mismatch at tap (kh {kh}, kw {kw}, ci {ci}, co {co}): got {float(got[idx])!r}, fp64 gives "
                    f"{float(ref[idx])!r}; {int(((got != ref) | torch.isnan(got)).sum())} of {got.numel()} taps differ")


# ================================================================================================ integer operands
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("ci", C.CINS, ids=["cin1", "cin5"])
@pytest.mark.parametrize("cid", SHAPES)
def test_integer_operands_are_exact(H, bank, cid, ci, bias):
    """y, gx and gw equal the fp64 reference rounded to fp32 on every element of every image: any summation order is exact here, so
    one misplaced tile, halo column or slab is a mismatch, not an error within a bar"""
    C.assert_claims(cid)
    assert (H.call("smsut_conv2d_small_supported", C.KS, ci, C.CO) == 1)
    B = bank("integer", cid, ci)
    o, r = B["ops"], B["refs"]
    y, g1 = run_fwd(H, cid, ci, o["x"], o["w"], o["b"] if bias else None)
    assert_plane_equal("forward", cid, y, (r["y"] if bias else B["y_nobias"]).float())
    gx, g2 = run_dgrad(H, cid, ci, o["gy"], o["w"])
    assert_plane_equal("data-gradient", cid, gx, r["gx"].float())
    gw, ws, g3 = run_wgrad(H, cid, ci, o["x"], o["gy"])
    assert_taps_equal("weight gradient", cid, gw, r["gw"].float())
    if cid in C.STEM:                                             # slab g of the workspace is workgroup g's partial: all written
        p = C.StemPlan(*C.STEM[cid])
        assert bool(torch.isfinite(ws[:p.nwg * 25 * ci * C.CO]).all()), "a slab of the weight gradient was not written"
    assert untouched(g1, g2, *g3)


# ================================================================================================ one-hot operands
@pytest.mark.parametrize("ci", C.CINS, ids=["cin1", "cin5"])
@pytest.mark.parametrize("cid", C.ONE_HOT_SHAPES)
def test_one_hot_taps_copy_the_plane_bit_for_bit(H, cid, ci):
    """a weight that is 1.0 at one (kh, kw, ci, co): forward (no bias) is x's channel ci shifted by the tap in channel co, the
    data-gradient gy's channel co shifted the other way in channel ci, zero-padded, the other channels 0 -- with full-mantissa data"""
    n, h, w = C.ALL[cid]
    g = C.gen(90 + ci)
    x, gy = C.rn(g, n, h, w, ci).cuda(), C.rn(g, n, h, w, C.CO).cuda()
    st = H.stream_ptr()
    y, g1 = out_buf(n, h, w, C.CO)
    gx, g2 = out_buf(n, h, w, ci)
    for kh, kw, c, co in C.one_hot_taps(ci):
        wt = C.one_hot_weight(kh, kw, c, co, ci).cuda()
        y.fill_(float("nan"))
        gx.fill_(float("nan"))
        H.call("smsut_conv2d_small_fwd", x, wt, None, y, n, h, w, ci, h, w, C.CO, C.KS, 1, C.PAD, st)
        H.call("smsut_conv2d_small_dgrad", gy, wt, gx, n, h, w, ci, h, w, C.CO, C.KS, 1, C.PAD, st)
        assert_plane_equal(f"forward, one-hot weight (kh {kh}, kw {kw}, ci {c}, co {co}),", cid, y, C.one_hot_fwd_ref(x, kh, kw, c, co))
        assert_plane_equal(f"data-gradient, one-hot weight (kh {kh}, kw {kw}, ci {c}, co {co}),", cid, gx,
                           C.one_hot_dgrad_ref(gy, kh, kw, c, co, ci))
    assert untouched(g1, g2)


@pytest.mark.parametrize("ci", C.CINS, ids=["cin1", "cin5"])
@pytest.mark.parametrize("cid", C.ONE_HOT_SHAPES)
def test_one_hot_gradient_pixel_reads_its_window(H, cid, ci):
    """a gy that is 1.0 at one pixel and channel: gw[kh][kw][ci][co] = x[y + kh - 2][x + kw - 2][ci] or 0 outside the image, bit for bit;
    pixels at the image corners and on both sides of the tile seams"""
    n, h, w = C.ALL[cid]
    x = C.rn(C.gen(92 + ci), n, h, w, ci).cuda()
    guards = []
    for n0, py, px in C.one_hot_pixels(cid):
        for co in C.ONE_HOT_CO:
            gw, _, g = run_wgrad(H, cid, ci, x, C.one_hot_gy(cid, n0, py, px, co).cuda())
            assert_taps_equal(f"weight gradient, one-hot gy at (n {n0}, y {py}, x {px}, co {co}): in-tile (row {py % C.STY}, col "
                              f"{px % C.STX}),", cid, gw, C.one_hot_wgrad_ref(x, n0, py, px, co))
            guards += g
    assert untouched(*guards)


# ================================================================================================ float operands
@pytest.mark.parametrize("ci", C.CINS, ids=["cin1", "cin5"])
@pytest.mark.parametrize("cid", STEM)
def test_float_operands_against_fp64(H, bank, cid, ci):
    """Gaussian operands: forward and data-gradient inside the K-term dot-product bound ELEMENT BY ELEMENT (bound and reference in fp64,
    nothing taken from the kernel's output), and all three at the bars the project holds its other convolution kernels to"""
    B = bank("float", cid, ci)
    o, r = B["ops"], B["refs"]
    a = C.abs_refs64(o)
    y, g1 = run_fwd(H, cid, ci, o["x"], o["w"], o["b"])
    gx, g2 = run_dgrad(H, cid, ci, o["gy"], o["w"])
    gw, _, g3 = run_wgrad(H, cid, ci, o["x"], o["gy"])
    worst = {}
    for name, got, k in (("fwd", y, 25 * ci + 1), ("dgrad", gx, 200)):
        ref = r["y" if name == "fwd" else "gx"]
        bound = (k + 2) * C.U * a["y" if name == "fwd" else "gx"]
        err = (got.double() - ref).abs()
        assert float(bound.min()) > 0
        worst[name] = float((err / bound).max())
        print(f"stem {cid} cin{ci} {name}: max |got - ref64| / ((K + 2) 2^-24 A) = {worst[name]:.3g} (K = {k}; must be <= 1)"
              + (" WITHIN A FACTOR OF 4 of the bound" if 4 * worst[name] >= 1 else ""))
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(gx).all())
    assert worst["fwd"] <= 1.0, f"forward {cid}: an element is {worst['fwd']:.3g} x its dot-product bound from fp64"
    assert worst["dgrad"] <= 1.0, f"data-gradient {cid}: an element is {worst['dgrad']:.3g} x its dot-product bound from fp64"
    e = {"fwd": check(f"stem {cid} cin{ci} fwd", y, r["y"].cpu(), FWD_BAR),
         "dgrad": check(f"stem {cid} cin{ci} dgrad", gx, r["gx"].cpu(), FWD_BAR),
         "wgrad": check(f"stem {cid} cin{ci} wgrad", gw, r["gw"].cpu(), WGRAD_BAR)}
    for name, v in e.items():
        bar = WGRAD_BAR if name == "wgrad" else FWD_BAR
        if 4 * v >= bar:
            print(f"stem {cid} cin{ci} {name}: rel_err {v:.3g} is WITHIN A FACTOR OF 4 of its bar {bar:.3g}")
    assert untouched(g1, g2, *g3)


# ================================================================================================ determinism
@pytest.mark.parametrize("ci", C.CINS, ids=["cin1", "cin5"])
@pytest.mark.parametrize("cid", ["E", "F"])
def test_two_calls_are_bitwise_equal(H, bank, cid, ci):
    """no atomics, register accumulation in tile order, a fixed xor tree, a fixed-order slab sum: the bits repeat, whatever the
    workspace held before (the second call's is filled with a finite value instead of NaN)"""
    o = bank("float", cid, ci)["ops"]
    gw1, ws1, ga = run_wgrad(H, cid, ci, o["x"], o["gy"])
    gw2, ws2, gb = run_wgrad(H, cid, ci, o["x"], o["gy"], fill=-7.5e37)
    p = C.StemPlan(*C.STEM[cid])
    used = p.nwg * 25 * ci * C.CO
    assert bool(torch.isfinite(gw1).all()) and torch.equal(gw1, gw2)
    assert torch.equal(ws1[:used], ws2[:used]), "the slabs themselves repeat"
    assert bool(torch.isnan(ws1[used:]).all()) and bool((ws2[used:] == -7.5e37).all()), "nothing behind the last slab is written"
    assert untouched(*ga, *gb)


# ================================================================================================ the public op
@pytest.mark.parametrize("ci", C.CINS, ids=["cin1", "cin5"])
def test_autograd_entry_takes_the_same_kernels(ops, H, bank, ci):
    """ops.conv2d / Conv2dFn as the networks' first layer calls it (logical NCHW over NHWC memory, OIHW over HWIO) on shape B with integer
    operands: output, input gradient, weight gradient and bias gradient are exact against fp64 and no layout copy is made"""
    cid = "B"
    n, h, w = C.ALL[cid]
    assert H.call("smsut_conv2d_mfma_supported", C.KS, 1, C.PAD, ci, C.CO) == 0
    assert H.call("smsut_conv2d_wgrad_mfma_supported", C.KS, 1, C.PAD, ci, C.CO) == 0
    assert H.call("smsut_conv2d_small_supported", C.KS, ci, C.CO) == 1 and H.call("smsut_conv2d_flat_wgrad_supported", C.KS, 1, ci, C.CO) == 1
    B = bank("integer", cid, ci)
    o, r = B["ops"], B["refs"]
    copies = ops.layout_copies()
    xd = o["x"].clone().permute(0, 3, 1, 2).requires_grad_(True)
    wd = o["w"].clone().permute(3, 2, 0, 1).requires_grad_(True)
    bd = o["b"].clone().requires_grad_(True)
    y = ops.conv2d(xd, wd, bd, 1, C.PAD)
    y.backward(o["gy"].permute(0, 3, 1, 2))
    assert ops.layout_copies() == copies
    assert tuple(y.shape) == (n, C.CO, h, w)
    assert_plane_equal("ops.conv2d forward", cid, y.detach().permute(0, 2, 3, 1), r["y"].float())
    assert_plane_equal("ops.conv2d input gradient", cid, xd.grad.permute(0, 2, 3, 1), r["gx"].float())
    assert_taps_equal("ops.conv2d weight gradient", cid, wd.grad.permute(2, 3, 1, 0), r["gw"].float())
    gb = o["gy"].double().sum((0, 1, 2))
    assert float(o["gy"].abs().sum()) < 2.0 ** 24 and torch.equal(bd.grad, gb.float()), "bias gradient"
    # ... and they are the bits of the direct calls
    yk, g1 = run_fwd(H, cid, ci, o["x"], o["w"], o["b"])
    gxk, g2 = run_dgrad(H, cid, ci, o["gy"], o["w"])
    gwk, _, g3 = run_wgrad(H, cid, ci, o["x"], o["gy"])
    assert torch.equal(y.detach().permute(0, 2, 3, 1), yk) and torch.equal(xd.grad.permute(0, 2, 3, 1), gxk)
    assert torch.equal(wd.grad.permute(2, 3, 1, 0), gwk)
    assert untouched(g1, g2, *g3)
