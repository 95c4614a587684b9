"""The fp16-operand convolution kernels (BASELINE config 5's whole conv path) against fp64 on the CPU, each through its own C-ABI
entry point, at the shapes where the launch plan, the tile walk or the staging changes:

  1. the per-tile kernel ``conv_mfma_fwd<.., F16, MW, CKW>`` with 16- and 32-channel passes (csrc/conv_mfma.hip),
  2. the persistent kernel ``conv_mfma_fwd_p<.., F16, ..>`` in its plain, statistics, virtual-cat, split, fused-shortcut, BST and
     half-storage forms,
  3. the weight gradient ``conv_f16_wgrad<CIT, COT, DUAL, SC, XH, INAFF>``.

Two tiers of reference, neither limited by fp16 operand rounding (``f16_edge_cases.py`` holds the tables, the generators and the
conditions; ``test_f16_edges_cases_cpu.py`` checks those without a GPU):

  A  exact: small-integer operands (gradients times 2^-23, the scale from ``smsut_absmax_scale`` / ``_scale2``) -- every result, every
     half-storage result and every statistics partial is asserted BIT-EQUAL (``torch.equal``) to the fp64 reference cast to fp32, for
     one-hot taps 0, 4, 7, 8 and the full 3x3 kernel.
  B  rounded operands: Gaussian inputs at real magnitudes against fp64 of the operands as the kernel rounds them, at the fp32 twins'
     bars from ``test_conv3x3_edges_gpu.py``: 2e-6 forward / data-gradient, 5e-6 input-side InstanceNorm, 3e-6 weight gradients
     over <= ~1e5 pixels (5e-5 beyond), statistics rtol 1e-5 atol 1e-3; a half-storage result lies within half an fp16 ulp of the
     reference plus that bar.  Each leg prints its figure.

Conventions as in ``test_conv3x3_edges_gpu.py``: NHWC tensors, ``[3][3][Cin][Cout]`` weights, outputs of NaN with a sentinel guard
behind them, statistics buffers and workspaces of exactly their query's size, every ``*_supported`` predicate asserted before a launch,
the kernel family asserted through ``smsut_conv2d_mfma_persistent(.., f16=1)`` / ``_tiles(.., f16=1)`` or restated from the cited
source lines where there is no query."""
import pytest
import torch

import f16_edge_cases as C
from conv_edge_helpers import based_buf, cdiv, out_buf, out_buf_h, poisoned, tile_sums, untouched

pytestmark = pytest.mark.gpu

FWD_BAR = 2e-6
AFF_BAR = 5e-6
WGRAD_BAR = 3e-6
WGRAD_BAR_BIG = 5e-5


@pytest.fixture(scope="module")
def H():
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _hip


@pytest.fixture(scope="module")
def cus(H):
    return torch.cuda.get_device_properties(0).multi_processor_count


_REFS = {}


def refs_for(cls, *key, **kw):
    """one shape at a time: the taps of a case are neighbours and share inputs and references"""
    k = (cls.__name__,) + key + tuple(sorted(kw.items()))
    if k not in _REFS:
        _REFS.clear()
        _REFS[k] = cls(*key, **kw)
    return _REFS[k]


def exact(tag, got, ref64):
    """bit equality with the fp64 reference cast to the output's type (a NaN left in `got` fails it)"""
    want = ref64.float().to(got.dtype).cuda()
    ok = torch.equal(got, want.view_as(got))
    if not ok:
        bad = (got != want.view_as(got))
        print(f"{tag}: {int(bad.sum())} of {bad.numel()} elements differ, first at {tuple(bad.nonzero()[0].tolist())}")
    assert ok, tag


def close(tag, got, ref64, bar):
    r = ref64.cuda()
    e = float((got.double() - r).abs().max() / r.abs().max())
    print(f"{tag}: rel_err {e:.3g} bar {bar:.3g}")
    assert e < bar, tag


def close_half(tag, got16, ref64, bar):
    """an fp16 store of an fp32 result within `bar` of the reference: at most half an fp16 ulp of the reference away, plus the bar"""
    r = ref64.cuda()
    ulp = 2.0 ** (torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -14))) - 10)
    over = float(((got16.double() - r).abs() - ulp / 2).max() / r.abs().max())
    print(f"{tag}: beyond half an fp16 ulp by {over:.3g} of max |ref|, bar {bar:.3g}")
    assert over < bar, tag


def grad_scale(H, t, t2=None):
    """{s, 1/s} from smsut_absmax_scale / _scale2, asserted to put the maximum into [2^13, 2^14]; returns (device pair, s)"""
    out, g1 = out_buf(2)
    ws, g2 = poisoned(H.call("smsut_absmax_scale_ws", t.numel() + (t2.numel() if t2 is not None else 0)))
    if t2 is None:
        H.call("smsut_absmax_scale", t, t.numel(), out, ws, H.stream_ptr())
    else:
        H.call("smsut_absmax_scale2", t, t.numel(), t2, t2.numel(), out, ws, H.stream_ptr())
    s, si = out.tolist()
    m = max(float(t.abs().max()), float(t2.abs().max()) if t2 is not None else 0.0)
    assert 2.0 ** 13 <= m * s <= 2.0 ** 14 and s * si == 1.0, (m, s, si)
    assert untouched(g1, g2)
    return out, s


def partials_ref(v64, th, second=None):
    """[n][tiles][c][2] = per-tile {sum v, sum v^2} (or {sum v, sum v * second}) in fp64"""
    return torch.stack([tile_sums(v64, th, 16), tile_sums(v64 * (v64 if second is None else second), th, 16)], -1)


class Run:
    """one case's launches: buffers with guards, the stream, the shape"""

    def __init__(self, H, n, h, w, ci, co, ks=3):
        self.H, self.st, self.shape, self.ks, self.guards = H, H.stream_ptr(), (n, h, w, ci, co), ks, []
        self.tag = f"{n}x{h}x{w} {ci}->{co}" + (" 1x1" if ks == 1 else "")

    def out(self, c, half=False):
        n, h, w = self.shape[:3]
        t, g = (out_buf_h if half else out_buf)(n, h, w, c)
        self.guards.append(g)
        return t

    def stats(self, c, tiles):
        buf, g = poisoned(self.shape[0] * tiles * c * 2)
        self.guards.append(g)
        return buf

    def based(self, base):
        t, g = based_buf(base)
        self.guards.append(g)
        return t

    def done(self):
        torch.cuda.synchronize()
        assert untouched(*self.guards), f"{self.tag}: a guard behind an output or a statistics buffer was written"


def halves(t):
    c = t.shape[3] // 2
    return t[..., :c].contiguous(), t[..., c:].contiguous()


def run_a(H, R, legs, tap, th_f, th_d, splits_d=(), splits_f=()):
    """tier A: every listed form of the conv [ci -> co] held by R, for one weight tensor (tap), bit-equal to fp64.  th_f / th_d: rows
    of the statistics tile of the forward (Kdim ci) / the data-gradient (Kdim co) launch."""
    n, h, w, ci, co = R.shape
    ks = R.ks
    r = Run(H, n, h, w, ci, co, ks)
    st, tag = r.st, f"{r.tag} tap {tap}"
    C.conditions_a(R, legs, th_f, th_d, tap)
    on_dev = {}

    def dev(name):
        if name not in on_dev:
            on_dev[name] = R.cpu(name).cuda()
        return on_dev[name]
    wd = R.wt(tap).cuda()
    assert H.call("smsut_conv2d_f16_supported", ks, ci, co) == 1
    tiles = H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, ks, 1)
    assert tiles == cdiv(h, th_f) * cdiv(w, 16)
    back = set(legs) & {"dgrad", "acc", "split", "bst", "bsths"}
    if back:
        assert H.call("smsut_conv2d_f16_supported", ks, co, ci) == 1
        gsc, s = grad_scale(H, dev("gy"))
    y_ref = lambda: R.ref("y", tap)
    for leg in legs:
        if leg == "fwd":
            y = r.out(co)
            H.call("smsut_conv2d_fwd_mfma_f16", dev("x"), wd, y, None, n, h, w, ci, co, ks, 0, st)
            exact(f"{tag} fwd", y, y_ref())
        elif leg == "fwd+":
            y = r.based(R.cpu("basey"))
            H.call("smsut_conv2d_fwd_mfma_f16", dev("x"), wd, y, None, n, h, w, ci, co, ks, 2, st)
            exact(f"{tag} fwd accumulate", y, R.ref("y+base", tap))
        elif leg == "stats":
            y, part = r.out(co), r.stats(co, tiles)
            H.call("smsut_conv2d_fwd_mfma_stats_f16", dev("x"), wd, y, part, n, h, w, ci, co, ks, st)
            exact(f"{tag} stats y", y, y_ref())
            exact(f"{tag} stats partials", part[:n * tiles * co * 2], partials_ref(y_ref(), th_f))
        elif leg == "dgrad":
            gx = r.out(ci)
            H.call("smsut_conv2d_fwd_mfma_f16", dev("gy"), wd, gx, gsc, n, h, w, co, ci, ks, 1, st)
            exact(f"{tag} dgrad", gx, R.ref("gx", tap))
        elif leg == "acc":
            acc = r.based(R.cpu("base"))
            H.call("smsut_conv2d_fwd_mfma_f16", dev("gy"), wd, acc, gsc, n, h, w, co, ci, ks, 3, st)
            exact(f"{tag} dgrad accumulate", acc, R.ref("gx+base", tap))
        elif leg in ("cat", "hscat"):
            assert H.call("smsut_conv2d_mfma_cat_supported", n, h, w, ci, co) == 1
            xa, xb = halves(dev("x"))
            half = leg == "hscat"
            y, part = r.out(co, half), r.stats(co, tiles)
            if half:
                assert H.call("smsut_conv2d_f16_hs_supported", n, h, w, ci, co, 1) == 1
                H.call("smsut_conv2d_fwd_mfma_stats_f16_hs", xa, xb, wd, y, part, n, h, w, ci, co, st)
            else:
                H.call("smsut_conv2d_fwd_mfma_stats_cat_f16", xa, xb, wd, y, part, n, h, w, ci, co, st)
            exact(f"{tag} {leg} y", y, y_ref())
            exact(f"{tag} {leg} partials", part[:n * tiles * co * 2], partials_ref(y_ref(), th_f))
        elif leg == "split":
            for tr in (0, 1, 3):
                k, m = (co, ci) if tr & 1 else (ci, co)
                for sp in (splits_d if tr & 1 else splits_f):
                    assert H.call("smsut_conv2d_mfma_split_supported", n, h, w, k, m, sp) == 1
                    if tr == 3:
                        ga, gb = r.based(R.cpu("base")[..., :sp].contiguous()), r.based(R.cpu("base")[..., sp:].contiguous())
                    else:
                        ga, gb = r.out(sp), r.out(m - sp)
                    H.call("smsut_conv2d_fwd_mfma_split_f16", dev("gy") if tr & 1 else dev("x"), wd, ga, gb, gsc if tr & 1 else None, sp,
                           n, h, w, k, m, tr, st)
                    exact(f"{tag} split {sp}+{m - sp} transposed {tr}", torch.cat([ga, gb], 3),
                          R.ref({0: "y", 1: "gx", 3: "gx+base"}[tr], tap))
        elif leg in ("hs", "hsx"):
            assert H.call("smsut_conv2d_f16_hs_supported", n, h, w, ci, co, 0) == 1
            y, part = r.out(co, True), r.stats(co, tiles)
            if leg == "hs":
                H.call("smsut_conv2d_fwd_mfma_stats_f16_hs", dev("x"), None, wd, y, part, n, h, w, ci, co, st)
            else:
                H.call("smsut_conv2d_fwd_mfma_stats_f16_hsx", dev("x").half(), wd, y, part, n, h, w, ci, co, st)
            exact(f"{tag} {leg} y", y, y_ref())
            exact(f"{tag} {leg} partials", part[:n * tiles * co * 2], partials_ref(y_ref(), th_f))
        elif leg == "inaffhsx":
            assert H.call("smsut_conv2d_f16_hs_supported", n, h, w, ci, co, 0) == 1
            a = R.aff()
            y, part = r.out(co, True), r.stats(co, tiles)
            H.call("smsut_conv2d_fwd_mfma_stats_inaff_f16_hsx", a["y1"].half().cuda(), wd, y, part, a["mean"].cuda(), a["rstd"].cuda(),
                   a["gam"].cuda(), a["bet"].cuda(), C.SLOPE_A, n, h, w, ci, co, st)
            exact(f"{tag} input-side IN y", y, R.ref("yaff", tap))
            exact(f"{tag} input-side IN partials", part[:n * tiles * co * 2], partials_ref(R.ref("yaff", tap), th_f))
        elif leg in ("sc", "sccat", "schs", "schscat"):
            cat, half = leg.endswith("cat"), "hs" in leg
            assert H.call("smsut_conv2d_fwd_sc_f16_supported", n, h, w, ci, co, int(cat)) == 1
            xa, xb = halves(dev("x")) if cat else (dev("x"), None)
            y, s2, p, q = r.out(co, half), r.out(co, half), r.stats(co, tiles), r.stats(co, tiles)
            if half:
                assert H.call("smsut_conv2d_f16_hs_supported", n, h, w, ci, co, int(cat)) == 1
            H.call("smsut_conv2d_fwd_mfma_stats_sc_f16" + ("_hs" if half else ""), xa, xb, wd, dev("w1"), y, s2, p, q, n, h, w, ci, co, st)
            exact(f"{tag} {leg} y", y, y_ref())
            exact(f"{tag} {leg} ysc", s2, R.ref("ysc"))
            exact(f"{tag} {leg} y partials", p[:n * tiles * co * 2], partials_ref(y_ref(), th_f))
            exact(f"{tag} {leg} ysc partials", q[:n * tiles * co * 2], partials_ref(R.ref("ysc"), th_f))
        elif leg in ("dsc", "dscsplit"):
            sc2, _ = grad_scale(H, dev("gy"), dev("gs"))
            for sp in (splits_d if leg == "dscsplit" else (0,)):
                assert H.call("smsut_conv2d_dgrad_sc_f16_supported", n, h, w, co, ci, sp) == 1
                ga, gb = (r.out(sp), r.out(ci - sp)) if sp else (r.out(ci), None)
                H.call("smsut_conv2d_dgrad_mfma_sc_f16", dev("gy"), dev("gs"), wd, dev("w1d"), ga, gb, sc2, sp, n, h, w, co, ci, st)
                exact(f"{tag} fused-shortcut dgrad{f' split {sp}' if sp else ''}", torch.cat([ga, gb], 3) if sp else ga, R.ref("gxsc", tap))
        elif leg in ("bst", "bsths"):
            half = leg == "bsths"
            assert H.call("smsut_conv2d_mfma_persistent", n, h, w, co, ci, 3, 1) == 1
            if half:
                assert H.call("smsut_conv2d_f16_hs_supported", n, h, w, co, ci, 0) == 1
            a = R.aff()
            tb = H.call("smsut_conv2d_mfma_tiles", n, h, w, co, ci, 3, 1)
            assert tb == (h // th_d) * (w // 16)
            gz, pb = r.out(ci), r.stats(ci, tb)
            y1 = a["y1"].half().cuda() if half else a["y1"].cuda()
            H.call("smsut_conv2d_dgrad_mfma_bwdstats_f16" + ("_hs" if half else ""), dev("gy"), wd, gz, pb, y1, a["mean"].cuda(),
                   a["rstd"].cuda(), a["gam"].cuda(), a["bet"].cuda(), gsc, C.SLOPE_A, n, h, w, co, ci, st)
            exact(f"{tag} {leg} gz", gz, R.ref("gz", tap))
            exact(f"{tag} {leg} partials", pb[:n * tb * ci * 2], partials_ref(R.ref("gz", tap), th_d, a["xhat"]))
        else:
            raise AssertionError(leg)
    r.done()


# ================================================================================================ 1. per-tile kernel
def _pid(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}-{c[5][0]}" + (f"-{c[5][1]}" if c[5][1] else "")


def per_tile_asserts(H, case):
    n, h, w, ci, co, (rf, rd), legs, sd, sf, ks1 = case
    row_f = C.per_tile_row_f16(n, h, w, co, False)
    assert row_f[0] == rf
    assert H.call("smsut_conv2d_mfma_persistent", n, h, w, ci, co, 3, 1) == 0
    assert H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 1) == cdiv(h, row_f[1]) * cdiv(w, 16)
    row_d = None
    if rd:
        row_d = C.per_tile_row_f16(n, h, w, ci, True)
        assert row_d[0] == rd and H.call("smsut_conv2d_mfma_persistent", n, h, w, co, ci, 3, 1) == 0
    else:
        assert not set(legs) & {"dgrad", "acc", "split"}
    return row_f, row_d


@pytest.mark.parametrize("case", C.PER_TILE, ids=[_pid(c) for c in C.PER_TILE])
def test_per_tile_kernel_exact(H, case):
    n, h, w, ci, co, rows, legs, sd, sf, ks1 = case
    row_f, row_d = per_tile_asserts(H, case)
    R = refs_for(C.IntRefs, n, h, w, ci, co)
    for tap in C.PER_TILE_TAPS[case[:5]]:
        run_a(H, R, legs, tap, row_f[1], row_d[1] if row_d else None, sd, sf)


KS1 = [c for c in C.PER_TILE if c[9]]


@pytest.mark.parametrize("case", KS1, ids=[_pid(c) for c in KS1])
def test_per_tile_kernel_1x1_exact(H, case):
    """KS == 1 through the fp16-operand entry points (dispatch_fwd<1>: the same table; 16-channel passes whatever Kdim)"""
    n, h, w, ci, co, rows, legs, sd, sf, ks1 = case
    row_f = C.per_tile_row_f16(n, h, w, co, False)
    assert C.ckw_f16(1, ci, False) == 16
    assert H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 1, 1) == cdiv(h, row_f[1]) * cdiv(w, 16)
    R = refs_for(C.IntRefs, n, h, w, ci, co, ks=1)
    run_a(H, R, [l for l in legs if l in C.BASIC], -1, row_f[1], None)


def test_per_tile_table_is_covered():
    """every row of dispatch_fwd's table an fp16-operand call can reach has a case, forward and data-gradient; both pass widths, the
    cat fall-back to 16-channel passes, the channel tails and the degenerate planes are there"""
    assert {c[5][0] for c in C.PER_TILE} == C.ROWS_FWD
    assert {c[5][1] for c in C.PER_TILE if c[5][1]} == C.ROWS_DGRAD
    for c in C.PER_TILE:
        n, h, w, ci, co = c[:5]
        assert not C.fwd_p_eligible(n, h, w, ci, co) and C.per_tile_row_f16(n, h, w, co, False)[0] == c[5][0]
        if c[5][1]:
            assert not C.fwd_p_eligible(n, h, w, co, ci) and C.per_tile_row_f16(n, h, w, ci, True)[0] == c[5][1]
    assert {c[3] for c in C.PER_TILE} >= {16, 32, 48, 64, 96}
    assert {C.ckw_f16(3, c[3], False) for c in C.PER_TILE} == {16, 32}
    cats = [c for c in C.PER_TILE if "cat" in c[6]]
    assert {C.ckw_f16(3, c[3], True) for c in cats} == {16, 32} and any(C.ckw_f16(3, c[3], True) != C.ckw_f16(3, c[3], False) for c in cats)
    assert {c[4] % 16 for c in C.PER_TILE} >= {4} and any(c[4] == 20 for c in C.PER_TILE)
    assert any(c[4] == 40 and C.per_tile_row_f16(*c[:3], c[4], False)[2] == 2 for c in C.PER_TILE), "Ndim 40 on an NTN = 2 row"
    assert any(c[2] == 1 for c in C.PER_TILE) and any(c[1] == 1 for c in C.PER_TILE)
    assert any(c[1] % 8 and c[2] % 16 for c in C.PER_TILE)
    assert sum(1 for c in C.PER_TILE if c[9]) >= 2
    sp = {s for c in C.PER_TILE for s in c[7] + c[8]}
    assert 16 in sp and any(s % 32 for s in sp if s != 16)


# ================================================================================================ 2. persistent kernel
def _qid(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}-{c[5]}-th{c[6][0]}ntn{c[6][1]}nch{c[6][2]}"


def persistent_asserts(H, cus, case):
    n, h, w, ci, co, kind, inst_f, inst_d = case
    assert h != w and C.select_fwd_p_f16(h, ci, co) == inst_f
    assert H.call("smsut_conv2d_mfma_persistent", n, h, w, ci, co, 3, 1) == 1
    assert H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 1) == (h // inst_f[0]) * (w // 16)
    units = n * (h // 8) * (w // 16) * (co // 16)
    if inst_d:
        assert C.select_fwd_p_f16(h, co, ci) == inst_d and H.call("smsut_conv2d_mfma_persistent", n, h, w, co, ci, 3, 1) == 1
    if kind == "edge":
        assert 1024 <= units < 1024 + 24, "just over the persistent kernel's threshold"
    else:
        items, nz = n * (h // inst_f[0]) * (w // 16), co // (16 * inst_f[1])
        assert items * nz > C.WG_PER_CU * cus, "not a walk on this device"
        lens = C.walk_lengths(items, nz, cus)
        assert min(lens) >= 2 and all(items % ipw for ipw in lens), (items, sorted(lens))
        assert (h // inst_f[0]) * (w // 16) > 1, "walks must cross images inside a workgroup's run"


EDGE = [c for c in C.PERSISTENT if c[5] == "edge"]
WALK = [c for c in C.PERSISTENT if c[5] == "walk"]


@pytest.mark.parametrize("tap", C.TAPS, ids=[f"tap{t}" if t >= 0 else "full" for t in C.TAPS])
@pytest.mark.parametrize("case", EDGE, ids=[_qid(c) for c in EDGE])
def test_persistent_kernel_every_form_exact(H, cus, case, tap):
    n, h, w, ci, co, kind, inst_f, inst_d = case
    persistent_asserts(H, cus, case)
    legs = C.edge_legs(n, h, w, ci, co)
    if "split" in legs:
        for sp in C.persistent_splits(ci):
            assert C.select_fwd_p_f16(h, co, ci, sp) == ((8, 1, 2) if (co == 32 and sp % 32) else inst_d)
    if "dsc" in legs:
        assert C.select_fwd_p_f16(h, 2 * co, ci) in ((8, 1, 2), (8, 2, 2), (8, 1, 4))
    R = refs_for(C.IntRefs, n, h, w, ci, co)
    run_a(H, R, legs, tap, inst_f[0], inst_d[0] if inst_d else None, C.persistent_splits(ci))


@pytest.mark.parametrize("case", WALK, ids=[_qid(c) for c in WALK])
def test_persistent_kernel_walk_with_short_last_run_exact(H, cus, case):
    n, h, w, ci, co, kind, inst_f, inst_d = case
    persistent_asserts(H, cus, case)
    R = refs_for(C.IntRefs, n, h, w, ci, co)
    run_a(H, R, C.edge_legs(n, h, w, ci, co), -1, inst_f[0], inst_d[0], C.persistent_splits(ci))


def run_b(H, n, h, w, ci, co, th):
    """tier B on one persistent shape: plain, statistics, half storage, input-side IN, fused shortcut, data-gradient and accumulate"""
    R = refs_for(C.GaussRefs, n, h, w, ci, co)
    r = Run(H, n, h, w, ci, co)
    st, tag = r.st, f"tier B {r.tag}"
    dev = lambda name: R.cpu(name).cuda()
    tiles = H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 1)
    assert tiles == (h // th) * (w // 16)

    def parts(tg, part, y):
        p = part[:n * tiles * co * 2].view(n, tiles, co, 2).double().sum(1)
        d = y.double()
        c0, c1 = d.sum((1, 2)), (d * d).sum((1, 2))
        print(f"{tg}: partial sums off by {float((p[..., 0] - c0).abs().max()):.3g} / {float((p[..., 1] - c1).abs().max()):.3g}")
        assert torch.allclose(p[..., 0], c0, rtol=1e-5, atol=1e-3) and torch.allclose(p[..., 1], c1, rtol=1e-5, atol=1e-3), tg

    y = r.out(co)
    H.call("smsut_conv2d_fwd_mfma_f16", dev("x"), dev("wt"), y, None, n, h, w, ci, co, 3, 0, st)
    close(f"{tag} fwd", y, R.ref("y"), FWD_BAR)
    ys, part = r.out(co), r.stats(co, tiles)
    H.call("smsut_conv2d_fwd_mfma_stats_f16", dev("x"), dev("wt"), ys, part, n, h, w, ci, co, 3, st)
    close(f"{tag} stats y", ys, R.ref("y"), FWD_BAR)
    parts(f"{tag} stats", part, ys)
    assert H.call("smsut_conv2d_f16_hs_supported", n, h, w, ci, co, 0) == 1
    yh, ph = r.out(co, True), r.stats(co, tiles)
    H.call("smsut_conv2d_fwd_mfma_stats_f16_hs", dev("x"), None, dev("wt"), yh, ph, n, h, w, ci, co, st)
    close_half(f"{tag} half storage", yh, R.ref("y"), FWD_BAR)
    parts(f"{tag} half storage", ph, ys)
    a = R.aff()
    ya, pa = r.out(co, True), r.stats(co, tiles)
    H.call("smsut_conv2d_fwd_mfma_stats_inaff_f16_hsx", a["y1"].cuda(), dev("wt"), ya, pa, a["mean"].cuda(), a["rstd"].cuda(), a["gam"].cuda(),
           a["bet"].cuda(), C.SLOPE_B, n, h, w, ci, co, st)
    close_half(f"{tag} input-side IN, half storage", ya, R.ref("yaff"), AFF_BAR)
    assert H.call("smsut_conv2d_fwd_sc_f16_supported", n, h, w, ci, co, 0) == 1
    y2, s2, p2, q2 = r.out(co), r.out(co), r.stats(co, tiles), r.stats(co, tiles)
    H.call("smsut_conv2d_fwd_mfma_stats_sc_f16", dev("x"), None, dev("wt"), dev("w1"), y2, s2, p2, q2, n, h, w, ci, co, st)
    close(f"{tag} fused shortcut y", y2, R.ref("y"), FWD_BAR)
    close(f"{tag} fused shortcut ysc", s2, R.ref("ysc"), FWD_BAR)
    parts(f"{tag} fused shortcut ysc", q2, s2)
    if C.fwd_p_eligible(n, h, w, co, ci):
        gsc, s = grad_scale(H, dev("gy"))
        gx = r.out(ci)
        H.call("smsut_conv2d_fwd_mfma_f16", dev("gy"), dev("wt"), gx, gsc, n, h, w, co, ci, 3, 1, st)
        close(f"{tag} dgrad (scale 2^{int(torch.log2(torch.tensor(s)))})", gx, R.ref("gx", s), FWD_BAR)
        acc = r.based(R.cpu("base"))
        H.call("smsut_conv2d_fwd_mfma_f16", dev("gy"), dev("wt"), acc, gsc, n, h, w, co, ci, 3, 3, st)
        close(f"{tag} dgrad accumulate", acc, R.ref("gx+base", s), FWD_BAR)
    r.done()


@pytest.mark.parametrize("case", EDGE, ids=[_qid(c) for c in EDGE])
def test_persistent_kernel_rounded_operands(H, cus, case):
    """tier B, one shape per instantiation.  The accumulation is fp32 in both, so the fp32 twins' bars apply."""
    n, h, w, ci, co, kind, inst_f, inst_d = case
    persistent_asserts(H, cus, case)
    run_b(H, n, h, w, ci, co, inst_f[0])


def test_per_tile_kernel_rounded_operands(H):
    """tier B on the per-tile kernel: a 16-channel-pass and a 32-channel-pass shape, forward, statistics and data-gradient"""
    for case in (C.PER_TILE[3], C.PER_TILE[6]):
        n, h, w, ci, co = case[:5]
        row_f, row_d = per_tile_asserts(H, case)
        R = refs_for(C.GaussRefs, n, h, w, ci, co)
        r = Run(H, n, h, w, ci, co)
        dev = lambda name: R.cpu(name).cuda()
        tiles = H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 1)
        y, part = r.out(co), r.stats(co, tiles)
        H.call("smsut_conv2d_fwd_mfma_stats_f16", dev("x"), dev("wt"), y, part, n, h, w, ci, co, 3, r.st)
        close(f"tier B {r.tag} per-tile fwd", y, R.ref("y"), FWD_BAR)
        p = part[:n * tiles * co * 2].view(n, tiles, co, 2).double().sum(1)
        assert torch.allclose(p[..., 0], y.double().sum((1, 2)), rtol=1e-5, atol=1e-3)
        assert torch.allclose(p[..., 1], (y.double() ** 2).sum((1, 2)), rtol=1e-5, atol=1e-3)
        gsc, s = grad_scale(H, dev("gy"))
        gx = r.out(ci)
        H.call("smsut_conv2d_fwd_mfma_f16", dev("gy"), dev("wt"), gx, gsc, n, h, w, co, ci, 3, 1, r.st)
        close(f"tier B {r.tag} per-tile dgrad", gx, R.ref("gx", s), FWD_BAR)
        r.done()


def test_fused_shortcut_half_storage_at_8_input_channels(H):
    """the 8 -> 16 fused-shortcut half-storage form runs on fp32 operands (no fp16 twin of the 8-channel form): tier B only, against
    fp64 of the UNROUNDED operands"""
    n, h, w, ci, co = 130, 24, 48, 8, 16
    assert H.call("smsut_conv2d_f16_hs_supported", n, h, w, ci, co, 0) == 1
    R = refs_for(C.GaussRefs, n, h, w, ci, co)
    r = Run(H, n, h, w, ci, co)
    tiles = H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 0)
    y, s2, p, q = r.out(co, True), r.out(co, True), r.stats(co, tiles), r.stats(co, tiles)
    H.call("smsut_conv2d_fwd_mfma_stats_sc_f16_hs", R.cpu("x").cuda(), None, R.cpu("wt").cuda(), R.cpu("w1").cuda(), y, s2, p, q,
           n, h, w, ci, co, r.st)
    close_half("8->16 fused shortcut, half storage y", y, R.ref("y_unrounded"), FWD_BAR)
    close_half("8->16 fused shortcut, half storage ysc", s2, R.ref("ysc_unrounded"), FWD_BAR)
    assert bool(torch.isfinite(p[:n * tiles * co * 2]).all()) and bool(torch.isfinite(q[:n * tiles * co * 2]).all())
    r.done()


def test_persistent_table_is_covered():
    """every row of select_fwd_p an fp16-operand call can reach has an edge and a walk case; the split and fused-shortcut rows too"""
    for kind in ("edge", "walk"):
        assert {c[6] for c in C.PERSISTENT if c[5] == kind} == set(C.P_INSTANCES)
    for c in C.PERSISTENT:
        n, h, w, ci, co = c[:5]
        assert C.fwd_p_eligible(n, h, w, ci, co) and C.select_fwd_p_f16(h, ci, co) == c[6]
    legs = {leg for c in EDGE for leg in C.edge_legs(*c[:5])}
    assert legs == {"fwd", "stats", "dgrad", "acc", "cat", "split", "sc", "sccat", "dsc", "dscsplit", "bst", "hs", "hsx", "inaffhsx", "schs",
                    "schscat", "bsths", "hscat"}
    dsc = {(c[4], C.select_fwd_p_f16(c[1], 2 * c[4], c[3])) for c in EDGE if "dsc" in C.edge_legs(*c[:5])}
    assert {co for co, _ in dsc} == {16, 32} and (32, (8, 1, 4)) in dsc, "fused-shortcut data-gradient at Cout 16, 32 and sc2_64"
    assert any(c[3] == 32 and c[4] == 32 and 16 in C.persistent_splits(c[3]) for c in EDGE), "a split that forces <3,8,1,2>"


# ================================================================================================ 3. weight gradient
def run_wgrad(H, case, tier):
    n, h, w, ci, co, forms, cas, what = case
    st = H.stream_ptr()
    assert H.call("smsut_conv2d_wgrad_f16_supported", n, h, w, ci, co) == 1 and C.wgrad_f16_supported(n, h, w, ci, co)
    cit, cot, splits, tps, total = C.plan_wgrad_f16(n, h, w, ci, co)
    R = refs_for(C.WgradRefs, n, h, w, ci, co, tier)
    if tier == "A":
        C.wgrad_conditions_a(R, forms)
    x, gy, gs = R.cpu("x").cuda(), R.cpu("gy").cuda(), R.cpu("gs").cuda()
    sc1, s1 = grad_scale(H, gy)
    sc2, s2 = grad_scale(H, gy, gs)
    bar = WGRAD_BAR if n * h * w <= 100000 else WGRAD_BAR_BIG
    for form in forms:
        sc = form in ("sc", "sccat")
        rows = 10 if sc else 9
        if sc:
            assert H.call("smsut_conv2d_wgrad_sc_f16_supported", n, h, w, ci, co) == 1
        ws_n = H.call("smsut_conv2d_wgrad_sc_f16_ws" if sc else "smsut_conv2d_wgrad_f16_ws", n, h, w, ci, co)
        assert ws_n == splits * rows * ci * co, "the workspace query must describe the plan this test derived"
        for ca in (cas if form in ("cat", "sccat") else (0,)):
            gw, gg = out_buf(rows, ci, co)
            ws, wg = poisoned(ws_n)
            gsc, s = (sc2, s2) if sc else (sc1, s1)
            xa, xb = (x[..., :ca].contiguous(), x[..., ca:].contiguous()) if ca else (x, None)
            if form in ("plain", "cat"):
                H.call("smsut_conv2d_wgrad_f16", xa, xb, ca, gy, gw, ws, gsc, n, h, w, ci, co, st)
            elif sc:
                H.call("smsut_conv2d_wgrad_sc_f16", xa, xb, ca, gy, gs, gw, ws, gsc, n, h, w, ci, co, st)
            elif form == "xh":
                H.call("smsut_conv2d_wgrad_f16_xh", x.half(), gy, gw, ws, gsc, n, h, w, ci, co, st)
            else:
                a = R.aff()
                H.call("smsut_conv2d_wgrad_f16_xh_inaff", a["y1"].half().cuda(), gy, gw, ws, gsc, a["mean"].cuda(), a["rstd"].cuda(),
                       a["gam"].cuda(), a["bet"].cuda(), a["slope"], n, h, w, ci, co, st)
            tag = (f"wgrad tier {tier} {form}{f' ca {ca}' if ca else ''} {n}x{h}x{w} {ci}->{co} <{cit},{cot}> splits {splits} x {tps} "
                   f"(last {total - (splits - 1) * tps})")
            ref9, ref1 = R.ref(s, form)
            if tier == "A":
                exact(tag, gw[:9].reshape(3, 3, ci, co), ref9)
                if sc:
                    exact(tag + " shortcut row", gw[9], ref1)
            else:
                close(tag, gw[:9].reshape(3, 3, ci, co), ref9, bar)
                if sc:
                    close(tag + " shortcut row", gw[9], ref1, bar)
            assert bool(torch.isfinite(ws[:ws_n]).all()), "every slab element of every split is written"
            assert untouched(gg, wg), tag
    return cit, cot, splits, tps, total


def _wid(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}-{c[7].replace(' ', '_')}"


@pytest.mark.parametrize("case", C.WGRAD, ids=[_wid(c) for c in C.WGRAD])
def test_wgrad_exact(H, case):
    n, h, w, ci, co, forms, cas, what = case
    cit, cot, splits, tps, total = run_wgrad(H, case, "A")
    if what == "short last split":
        assert tps > 1 and total % tps != 0 and splits * tps > total


WB = [c for c in C.WGRAD if c[:5] in C.WGRAD_TIER_B]


@pytest.mark.parametrize("case", WB, ids=[_wid(c) for c in WB])
def test_wgrad_rounded_operands(H, case):
    run_wgrad(H, case, "B")


def test_wgrad_table_is_covered():
    """every (CIT, COT, DUAL, SC, XH, INAFF) instantiation launch_wgrad_f16 can launch has a case; so have the planes and the plans"""
    got = {C.wgrad_instance(c[3], c[4], f) for c in C.WGRAD for f in c[5]}
    assert got == C.WGRAD_INSTANCES and len(C.WGRAD_INSTANCES) == 24
    for c in C.WGRAD:
        assert C.wgrad_f16_supported(*c[:5])
    assert {c[7] for c in C.WGRAD} == {"one tile", "tile row", "tile column", "short last split"}
    short = [c for c in C.WGRAD if c[7] == "short last split"]
    assert {C.plan_wgrad_f16(*c[:5])[:2] for c in short} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert any(c[3] // (16 * C.plan_wgrad_f16(*c[:5])[0]) > 1 for c in C.WGRAD) and any(c[4] // (16 * C.plan_wgrad_f16(*c[:5])[1]) > 1 for c in C.WGRAD)
    assert {ca for c in C.WGRAD for ca in c[6]} == {16, 32}
