"""The residual-tail family and the pool-fused InstanceNorm kernels of csrc/norm.hip against plain fp64 references, called through the
C ABI so that the VEC = 1, identity-shortcut, no-beta and ABI-only forms are reachable.

References, bounds (derived a priori: see the docstring of restail_ref.py) and the restated launch geometry live in restail_ref.py;
test_restail_cases_cpu.py pins the regime of every case id.  Every value comparison covers every element; bit-identity, integer and
position claims are exact.  Each test prints its worst error / bound ratio."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import restail_ref as R
from norm_test_helpers import _poisoned, _tickets, aff32
from restail_ref import SLOPE, U32
from test_instnorm_gpu import accum_len, fwd_stat_bounds, gam

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 4096


@pytest.fixture(scope="module")
def H():
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _hip


def _ids(cases):
    return [k for k, _ in cases]


def dev(a, half=False):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.astype(np.float16) if half else a).cuda()


def host(t):
    return t.cpu().numpy()


def guarded(n_el, fill=NAN, dtype=torch.float32):
    """(buffer, payload view, guard view): the payload and a guard behind it start as `fill`"""
    buf = torch.full((n_el + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[:n_el], buf[n_el:]


def untouched(g, fill=NAN):
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ratio(got, ref, bound):
    """worst |got - ref| / bound over EVERY element (a NaN anywhere makes it NaN, which fails `<= 1`)"""
    return float(np.max(np.abs(got.astype(np.float64) - ref) / bound))


@functools.lru_cache(maxsize=2)
def inputs(name, half):
    """the case's inputs on the host and on the GPU (shared by the tests and forms of a case; never modified)"""
    d = R.tail_inputs(R.SHAPES[name], 100 + 7 * _ids(R.CASES).index(name), half)
    g = {k: dev(v, half and k in ("y2", "s")) for k, v in d.items()}
    return d, g


def tail_args(g, shortcut, b2=True, bs=True):
    """(y2, m2, r2, g2, b2, s, ms, rs, gs, bs) of the entry points"""
    if not shortcut:
        return (g["y2"], g["m2"], g["r2"], g["g2"], g["b2"] if b2 else None, g["s"], None, None, None, None)
    return (g["y2"], g["m2"], g["r2"], g["g2"], g["b2"] if b2 else None, g["s"], g["ms"], g["rs"], g["gs"], g["bs"] if bs else None)


def run_fwd(H, g, shape, shortcut, slope, half=False):
    n, h, w, c = shape
    buf, out, guard = guarded(n * h * w * c)
    H.call("smsut_restail_fwd_hs" if half else "smsut_restail_fwd", *tail_args(g, shortcut), out, n, h * w, c, slope, H.stream_ptr())
    torch.cuda.synchronize()
    assert untouched(guard), "the forward stored past the end of out"
    return out.view(n, h * w, c)


# ---- 1. forward --------------------------------------------------------------------------------------------------------------------
FWD_PARAMS = ([(k, f, SLOPE) for k, s in R.TAIL_CASES for f in ("conv", "identity", "hs") if f != "hs" or s[3] % 4 == 0] +
              [("cv3_general_walk", "conv", 0.0)])


@pytest.mark.parametrize("name,form,slope", FWD_PARAMS, ids=[f"{k}-{f}-{s}" for k, f, s in FWD_PARAMS])
def test_restail_fwd_vs_fp64(H, name, form, slope):
    """smsut_restail_fwd / _hs: out = lrelu(IN(y2) + (IN(s) | s)) within 5 u M + u |ref| of fp64 at every element (c_f = 5: one
    subtraction, one product rstd * gamma and one fma per branch = 3, one add, one product with the slope; restail_ref.py), on output
    memory that starts as NaN, with a NaN guard behind it that stays NaN."""
    shape = R.SHAPES[name]
    half, shortcut = form == "hs", form != "identity"
    d, g = inputs(name, half)
    out = run_fwd(H, g, shape, shortcut, slope, half)
    ref, bound = R.fwd_ref(d, shortcut, slope)
    q = ratio(host(out), ref, bound)
    print(f"restail_fwd {name} {form} slope {slope}: worst error / bound {q:.3f}")
    assert q <= 1, (name, form, q)


# ---- 2. backward -------------------------------------------------------------------------------------------------------------------
NC_FILL = 12345.0


class Bwd:
    """output buffers of one backward call, every one poisoned and guarded"""

    def __init__(self, shape, chunks, nb=0, tickets=False):
        n, h, w, c = shape
        self.n, self.c = n, c
        self.gy2 = guarded(n * h * w * c)
        self.gs = guarded(n * h * w * c)
        self.means = [guarded(n * c, NC_FILL) for _ in range(3)]
        self.aff = [guarded(c) for _ in range(4)]                       # gg2, gb2, ggs, gbs
        self.ws, self.ws_guard = _poisoned(n * chunks * c * 3, c * 3)
        self.amax = guarded(2 * nb) if nb else None
        self.nb = nb
        self.tk = _tickets(n) if tickets else None

    def io(self):
        """(gy2, gs, a, b2, bs, gg2, gb2, ggs, gbs, workspace)"""
        return (self.gy2[1], self.gs[1], *[m[1] for m in self.means], *[a[1] for a in self.aff], self.ws)

    def check(self, shortcut):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.ws_guard).all()), "a partial was stored past the last image's block"
        for t in (self.gy2, self.gs, *self.aff):
            assert untouched(t[2]), "an output was stored past its end"
        for m in self.means:
            assert untouched(m[2], NC_FILL), "a mean was stored past [N][C]"
            assert bool(torch.isfinite(m[1]).all())
        if not shortcut:                                      # identity shortcut: ggs / gbs are not the tail's to write
            assert untouched(self.aff[2][1]) and untouched(self.aff[3][1]), "ggs / gbs written without a conv shortcut"
        if self.tk is not None:
            assert int(self.tk[:self.n].abs().sum()) == 0, "tickets not zero again"
            assert bool((self.tk[self.n:] == 0x5A5A5A5A).all()), "the ticket guard was written"
        if self.amax is not None:
            assert untouched(self.amax[2]), "an amax slot past 2 B was written"
            sl = self.amax[1]
            assert bool(torch.isfinite(sl).all()), "an amax slot was left unwritten"
            assert float(sl[:self.nb].max()) == float(self.gy2[1].abs().max()), "amax[0:B) is not max |gy2|"
            assert float(sl[self.nb:].max()) == float(self.gs[1].abs().max()), "amax[B:2B) is not max |gs|"

    def results(self, shortcut):
        names = ["gy2", "gs", "a", "b2", "bs", "gg2", "gb2"] + (["ggs", "gbs"] if shortcut else [])
        ts = [self.gy2[1], self.gs[1], *[m[1] for m in self.means], *[a[1] for a in self.aff]]
        return dict(zip(names, ts))


def run_bwd(H, entry, g, gout, out, shape, shortcut, slope, b2=True, bs=True, half=False, amax=False, tickets=False):
    n, h, w, c = shape
    chunks = H.call("smsut_in_chunks", n, h * w, c)
    nb = H.call("smsut_amax_blocks", n, h * w, c) if amax else 0
    assert not amax or nb == R.regime(*shape)["full"]["blocks"] * n
    o = Bwd(shape, chunks, nb, tickets)
    extra = {"smsut_restail_bwd": (), "smsut_restail_bwd_fin": (o.tk,), "smsut_restail_bwd_amax": (o.amax[1] if amax else None,),
             "smsut_restail_bwd_hs": (o.amax[1] if amax else None,)}[entry]
    H.call(entry, gout, out, *tail_args(g, shortcut, b2, bs), *o.io(), *extra, n, h * w, c, slope, H.stream_ptr())
    o.check(shortcut)
    return o.results(shortcut)


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert same_bits(a[k], b[k]), (what, k)


def check_bwd(res, ref, shape, what):
    """every output against its fp64 reference and bound; -> the worst ratio per output"""
    n, h, w, c = shape
    qs = {}
    for k, t in res.items():
        r, bound = ref[k]
        qs[k] = ratio(host(t).reshape(r.shape), r, bound)
    print(f"{what}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in qs.items()))
    for k, v in qs.items():
        assert v <= 1, (what, k, v)
    return qs


BWD_FORMS = {"conv": (True, True, True), "identity": (False, True, True), "conv_no_b2": (True, False, True),
             "conv_no_bs": (True, True, False)}                         # (shortcut, b2 given, bs given)
BWD_PARAMS = [(k, f, SLOPE) for k, _ in R.TAIL_CASES for f in BWD_FORMS] + [("cv3_general_walk", "conv", 0.0),
                                                                           ("vec1_two_chunks", "conv_no_bs", 0.0)]


@pytest.mark.parametrize("name,form,slope", BWD_PARAMS, ids=[f"{k}-{f}-{s}" for k, f, s in BWD_PARAMS])
def test_restail_bwd_vs_fp64(H, name, form, slope):
    """smsut_restail_bwd, _fin (with tickets) and _amax on the same inputs: the three per-(n, c) means, gy2 and gs at every element
    and the four affine gradients within their derived bounds of fp64 (restail_ref.py: means as the existing finalize test with
    K = accum_len + 2; gy2 / gs with the mean bounds propagated and c_b = 7; affine gradients HW sum_n d_n); _fin and _amax give the
    plain form's bits; the amax slots are smsut_amax_blocks per tensor and their maxima the maxima of the kernel's own outputs;
    ggs / gbs stay NaN with the identity shortcut; two runs give the same bits; workspace and outputs start poisoned behind guards.
    The mask is the kernel's (fp32 pre-activation restated, or the sign of the `out` handed in), so this tests arithmetic, not signs."""
    shape = R.SHAPES[name]
    shortcut, b2, bs = BWD_FORMS[form]
    d, g = inputs(name, False)
    out = run_fwd(H, g, shape, shortcut, slope)                   # the forward's own output (its sign is the mask without remask)
    kw = dict(shortcut=shortcut, slope=slope, b2=b2, bs=bs)
    plain = run_bwd(H, "smsut_restail_bwd", g, g["gout"], out, shape, **kw)
    again = run_bwd(H, "smsut_restail_bwd", g, g["gout"], out, shape, **kw)
    assert_same(plain, again, "second run differs")
    fin = run_bwd(H, "smsut_restail_bwd_fin", g, g["gout"], out, shape, tickets=True, **kw)
    assert_same(plain, fin, "_fin differs from the plain form")
    am = run_bwd(H, "smsut_restail_bwd_amax", g, g["gout"], out, shape, amax=True, **kw)
    assert_same(plain, am, "_amax differs from the plain form")
    mask = R.tail_mask(d, shortcut, b2 and bs, host(out))
    ref = R.bwd_ref(d, d["gout"], mask, shortcut, slope, shape)
    check_bwd(plain, ref, shape, f"restail_bwd {name} {form} slope {slope}")


# ---- 3. forward with the level's pooling -------------------------------------------------------------------------------------------
IDX_FILL = 0xEE


def run_fwd_pool(H, g, shape, maxpool, half, slope=SLOPE):
    """-> out [N, HW, C], pooled [N, H/2, W/2, C], idx [N, H/2, W/2, C] bytes (None: average pooling)"""
    n, h, w, c = shape
    npool = n * (h // 2) * (w // 2) * c
    _, out, og = guarded(n * h * w * c)
    _, pooled, pg = guarded(npool)
    _, idx, ig = guarded(npool, IDX_FILL, torch.uint8) if maxpool else (None, None, None)
    H.call("smsut_restail_fwd_pool", *tail_args(g, True), out, pooled, idx, n, h, w, c, slope, int(half), H.stream_ptr())
    torch.cuda.synchronize()
    assert untouched(og) and untouched(pg), "stored past the end of out / pooled"
    assert idx is None or untouched(ig, IDX_FILL), "stored past the end of idx"
    return out.view(n, h * w, c), pooled.view(n, h // 2, w // 2, c), idx.view(n, h // 2, w // 2, c) if maxpool else None


def check_pooled(out, pooled, idx, shape):
    """pooled and idx against the kernel's OWN out, exactly (host arrays)"""
    n, h, w, c = shape
    win = R.windows(out, h, w)
    if idx is None:                                        # (a0 + a1 + a2 + a3) * 0.25f in that order, in float32
        want = ((win[..., 0] + win[..., 1]) + win[..., 2] + win[..., 3]) * np.float32(0.25)
        assert want.dtype == np.float32
        ok = ~np.isnan(want)                               # (a NaN's payload is not part of the claim)
        assert np.array_equal(np.isnan(pooled), ~ok), "pooled is NaN elsewhere than the average"
        assert np.array_equal(pooled[ok].view(np.int32), want[ok].view(np.int32)), "pooled is not the window's average in k_avgpool_fwd's order"
        return
    kk, mv = R.first_max(win)
    assert np.array_equal(idx, kk), "idx is not the first maximal position in scan order"
    assert np.array_equal(pooled.view(np.int32), mv.view(np.int32)), "pooled is not the window's maximum"
    ok = ~np.isnan(mv)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(pooled[ok], np.max(win, axis=-1)[ok])
    assert np.array_equal(pooled.view(np.int32), np.take_along_axis(win, idx[..., None].astype(np.int64), -1)[..., 0].view(np.int32)), \
        "pooled is not the value at idx"


POOL_PARAMS = [(k, p, hs) for k, _ in R.TAIL_POOL_CASES for p in ("max", "avg") for hs in (False, True)]
POOL_IDS = [f"{k}-{p}-{'hs' if hs else 'fp32'}" for k, p, hs in POOL_PARAMS]


@pytest.mark.parametrize("name,pool,half", POOL_PARAMS, ids=POOL_IDS)
def test_restail_fwd_pool(H, name, pool, half):
    """smsut_restail_fwd_pool, max and average (idx null), fp32 and fp16 storage: out has the bits of smsut_restail_fwd[_hs] and is
    within the forward bound of fp64; pooled is exactly the maximum (or the float32 average in k_avgpool_fwd's order) of the kernel's
    own out over each window; every idx byte is the first maximal position in scan order, byte j of a word being channel 4 cv + j."""
    shape = R.SHAPES[name]
    d, g = inputs(name, half)
    out, pooled, idx = run_fwd_pool(H, g, shape, pool == "max", half)
    assert same_bits(out, run_fwd(H, g, shape, True, SLOPE, half)), "out differs from smsut_restail_fwd"
    ref, bound = R.fwd_ref(d, True, SLOPE)
    q = ratio(host(out), ref, bound)
    print(f"restail_fwd_pool {name} {pool} {'hs' if half else 'fp32'}: worst error / bound {q:.3f}")
    assert q <= 1, q
    check_pooled(host(out), host(pooled), None if idx is None else host(idx), shape)


@pytest.mark.parametrize("shape", R.TIE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restail_pool_ties_are_first_wins_and_route_one_pixel(H, shape):
    """whole windows equal (and pairs equal): the first position in scan order wins (idx against the kernel's own out).  The backward's
    routing is checked by the two bit-comparisons at the end: the total gradient built in numpy from the kernel's idx is
    smsut_maxpool2_bwd_add's (which looks at `out`, not at idx), and smsut_restail_bwd_pool gives the bits of smsut_restail_bwd on
    that materialised gradient.  (The numpy statement before them -- one routed pixel per window and channel, summing to gp -- only
    says that every idx byte is a valid position and that total_grad routes as documented.)  That enough pair ties are maxima is
    pinned on the CPU by test_restail_cases_cpu.py."""
    n, h, w, c = shape
    d = R.tie_inputs(shape, R.TIE_SEED)
    g = {k: dev(v) for k, v in d.items()}
    out, pooled, idx = run_fwd_pool(H, g, shape, True, False)
    o, ix = host(out), host(idx)
    check_pooled(o, host(pooled), ix, shape)
    win = R.windows(o, h, w)
    assert (ix[..., np.arange(c) % 3 == 0] == 0).all(), "a four-way tie did not go to position 0"
    t1 = np.arange(c) % 3 == 1
    pair_wins = R.tie_pair_wins(win)
    assert pair_wins[..., t1].sum() > R.TIE_MIN_PAIRS and (ix[pair_wins] == 1).all(), "a tie of positions 1 and 3 did not go to position 1"
    assert {0, 1, 2, 3} == set(np.unique(ix).tolist())
    # the routed gradient: one pixel per window and channel, summing to gp
    gp = np.random.RandomState(302).standard_normal((n, h // 2, w // 2, c)).astype(np.float32)
    routed = R.total_grad(np.zeros_like(d["gout"]), gp, ix, h, w)
    rw = R.windows(routed, h, w)
    assert ((rw != 0).sum(-1) == 1).all() and np.array_equal(rw.sum(-1), gp)
    total = R.total_grad(d["gout"], gp, ix, h, w)
    mat = torch.empty(n, h * w, c, device="cuda")
    H.call("smsut_maxpool2_bwd_add", dev(gp), out, g["gout"], mat, n, h, w, c, H.stream_ptr())
    assert np.array_equal(host(mat).view(np.int32), total.view(np.int32)), "the routed total gradient is not smsut_maxpool2_bwd_add's"
    base = run_bwd(H, "smsut_restail_bwd", g, mat, out, shape, True, SLOPE)
    got = run_bwd_pool(H, g, g["gout"], dev(gp), idx, shape, False)
    assert_same(base, got, "smsut_restail_bwd_pool differs from smsut_restail_bwd on the materialised gradient")


@pytest.mark.parametrize("pos", [0, 1, 2, 3])
def test_restail_pool_nan_propagates_like_maxpool2(H, pos):
    """one NaN at window position `pos` (every window of channel `pos`, and scattered windows of the others): pooled is NaN there and
    idx names the NaN's position -- what smsut_maxpool2_fwd and smsut_maxpool2_bwd do on the same out."""
    shape = (2, 18, 30, 12)
    n, h, w, c = shape
    d = R.tail_inputs(shape, 311)
    hit = np.random.RandomState(312 + pos).uniform(size=(n, h // 2, w // 2, c)) < 0.1
    hit[..., pos] = True
    y = d["y2"].reshape(n, h // 2, 2, w // 2, 2, c).copy()
    y[:, :, pos >> 1, :, pos & 1, :][hit] = np.nan
    d["y2"] = y.reshape(n, h * w, c)
    g = {k: dev(v) for k, v in d.items()}
    st = H.stream_ptr()
    out, pooled, idx = run_fwd_pool(H, g, shape, True, False)
    o, pl, ix = host(out), host(pooled), host(idx)
    check_pooled(o, pl, ix, shape)
    assert np.isnan(pl[hit]).all() and not np.isnan(pl[~hit]).any() and (ix[hit] == pos).all()
    mp = torch.empty(n, h // 2, w // 2, c, device="cuda")
    H.call("smsut_maxpool2_fwd", out, mp, n, h, w, c, st)
    assert same_bits(mp, pooled), "pooled differs from smsut_maxpool2_fwd"
    gx = torch.empty(n, h * w, c, device="cuda")
    H.call("smsut_maxpool2_bwd", torch.ones_like(mp), out, gx, n, h, w, c, st)
    gw = R.windows(host(gx), h, w)
    assert ((gw == 1).sum(-1) == 1).all() and ((gw == 0).sum(-1) == 3).all()
    assert np.array_equal(np.argmax(gw, -1).astype(np.uint8), ix), "idx is not where smsut_maxpool2_bwd routes"
    _, pa, _ = run_fwd_pool(H, g, shape, False, False)
    assert np.isnan(host(pa)[hit]).all() and not np.isnan(host(pa)[~hit]).any()
    check_pooled(o, host(pa), None, shape)


# ---- 4. backward with the pooled gradient routed in --------------------------------------------------------------------------------
def run_bwd_pool(H, g, gout, gp, idx, shape, half, tickets=False, amax=False, slope=SLOPE):
    n, h, w, c = shape
    chunks = H.call("smsut_in_chunks", n, h * w, c)
    nb = H.call("smsut_amax_blocks", n, h * w, c) if amax else 0
    o = Bwd(shape, chunks, nb, tickets)
    H.call("smsut_restail_bwd_pool", gout, gp, idx, *tail_args(g, True), *o.io(), o.tk, o.amax[1] if amax else None, n, h, w, c, slope,
           int(half), H.stream_ptr())
    o.check(True)
    return o.results(True)


@pytest.mark.parametrize("name,pool,half", POOL_PARAMS, ids=POOL_IDS)
def test_restail_bwd_pool(H, name, pool, half):
    """smsut_restail_bwd_pool: the total gradient formed in numpy float32 -- (idx == pos ? gp : 0) + gout for max, gp * 0.25 + gout for
    average, one exact add -- bounds gy2, gs, the means and the affine gradients through the fp64 reference of the backward test, and
    the results have the bits of smsut_restail_bwd[_hs] fed that materialised gradient: with and without tickets, with and without
    amax."""
    shape = R.SHAPES[name]
    n, h, w, c = shape
    d, g = inputs(name, half)
    out, _, idx = run_fwd_pool(H, g, shape, pool == "max", half)
    gp = (np.random.RandomState(41).standard_normal((n, h // 2, w // 2, c)) * 0.7).astype(np.float32)
    total = R.total_grad(d["gout"], gp, None if idx is None else host(idx), h, w)
    base = run_bwd(H, "smsut_restail_bwd_hs" if half else "smsut_restail_bwd", g, dev(total), out, shape, True, SLOPE, half=half)
    gpd = dev(gp)
    for tickets in (False, True):
        for amax in (False, True):
            got = run_bwd_pool(H, g, g["gout"], gpd, idx, shape, half, tickets, amax)
            assert_same(base, got, f"tickets {tickets} amax {amax}: differs from smsut_restail_bwd on the materialised gradient")
    ref = R.bwd_ref(d, total, R.tail_mask(d, True, True, None), True, SLOPE, shape)
    check_bwd(base, ref, shape, f"restail_bwd_pool {name} {pool} {'hs' if half else 'fp32'}")


# ---- 5. InstanceNorm + LeakyReLU + AvgPool2d(2) as one op --------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape", R.IN_POOL_CASES, ids=_ids(R.IN_POOL_CASES))
def test_instnorm_pool_fwd_bwd_vs_fp64(H, name, shape):
    """smsut_instnorm_pool_fwd_partials / smsut_instnorm_pool_bwd at the raw ABI, VEC = 1 (C = 6) included.
    Forward: the partials are the exact fp64 plane sums rounded to fp32 (chunks = 1), so (mean, rstd) carry the finalize's error alone:
    fwd_stat_bounds with K = 1.  y against the fp64 average of the four activated values, built from the kernel's own (mean, rstd):
    each value within 3 u (|d p| + |b|) (subtraction, product, fma) + u for the slope product, their sum through 3 additions
    (gam(3) sum |q|), the product with 0.25 exact, + u |ref|.  y, mean, rstd have the bits of smsut_instnorm_fwd_partials +
    smsut_avgpool2_fwd.
    Backward: gz = 0.25 gyp[h/2][w/2] * mask (the product with 0.25 exact); a, b as the first-order backward of test_instnorm_gpu.py
    ((gam(K) + u) E|gz|, (gam(K) + 4 u) E|gz xhat|, K = accum_len -- the statistics are inputs here, so no term for their error); gx
    and the affine gradients as in restail_ref.py.  All have the bits of smsut_avgpool2_bwd + smsut_instnorm_bwd."""
    n, h, w, c = shape
    hw, st = h * w, H.stream_ptr()
    x = R.planes(n, hw, c, R.IN_POOL_SEED)
    gam_, bet = R.affine(c, 72)
    x64 = x.astype(np.float64)
    part = np.stack([x64.sum(1), (x64 * x64).sum(1)], -1).astype(np.float32)          # [N][1][C][2]
    xd, gd, bd, pd = dev(x), dev(gam_), dev(bet), dev(part)
    npool = n * (hw // 4) * c

    def fwd(entry):
        _, y, yg = guarded(npool if entry.startswith("smsut_instnorm_pool") else n * hw * c)
        _, m, mg = guarded(n * c)
        _, r, rg = guarded(n * c)
        dims = (n, h, w, c) if entry.startswith("smsut_instnorm_pool") else (n, hw, c)
        tail = (R.EPS, SLOPE, st) if entry.startswith("smsut_instnorm_pool") else (R.EPS, SLOPE, 1, st)
        H.call(entry, xd, gd, bd, y, m, r, pd, 1, *dims, *tail)
        torch.cuda.synchronize()
        assert untouched(yg) and untouched(mg) and untouched(rg)
        return y, m, r
    y, m, r = fwd("smsut_instnorm_pool_fwd_partials")
    yf, mf, rf = fwd("smsut_instnorm_fwd_partials")
    yp = torch.empty(npool, device="cuda")
    H.call("smsut_avgpool2_fwd", yf, yp, n, h, w, c, st)
    assert same_bits(m, mf) and same_bits(r, rf) and same_bits(y, yp), "differs from smsut_instnorm_fwd_partials + smsut_avgpool2_fwd"
    # statistics
    xt = torch.from_numpy(x64).view(n, h, w, c).permute(0, 3, 1, 2)
    dm, drel = fwd_stat_bounds(xt, 1, R.EPS)
    mh, rh = host(m).reshape(n, c), host(r).reshape(n, c)
    rm = x64.mean(1)
    rr = 1.0 / np.sqrt(np.maximum((x64 * x64).mean(1) - rm * rm, 0) + R.EPS)
    q_m, q_r = float((np.abs(mh - rm) / dm).max()), float((np.abs(rh / rr - 1) / drel).max())
    # y
    dd = x64 - mh.astype(np.float64)[:, None, :]
    p = (rh.astype(np.float64) * gam_.astype(np.float64)[None, :])[:, None, :]
    pre = dd * p + bet.astype(np.float64)[None, None, :]
    s32 = float(np.float32(SLOPE))
    act = np.where(pre > 0, pre, pre * s32)
    eb = 4 * U32 * (np.abs(dd * p) + np.abs(bet.astype(np.float64))[None, None, :])
    ref_y = R.windows(act, h, w).sum(-1) * 0.25
    bound_y = 0.25 * (R.windows(eb, h, w).sum(-1) + gam(3) * R.windows(np.abs(act), h, w).sum(-1)) + U32 * np.abs(ref_y) + 1e-300
    q_y = ratio(host(y).reshape(ref_y.shape), ref_y, bound_y)
    print(f"instnorm_pool_fwd {name}: worst error / bound mean {q_m:.3f}, rstd {q_r:.3f}, y {q_y:.3f}")
    assert q_m <= 1 and q_r <= 1 and q_y <= 1, (q_m, q_r, q_y)

    # ---- backward
    gyp = (np.random.RandomState(73).standard_normal((n, h // 2, w // 2, c)) *
           np.exp(np.random.RandomState(74).uniform(-2, 1, (n, 1, 1, 1)))).astype(np.float32)
    gypd = dev(gyp)
    chunks = H.call("smsut_in_chunks", n, hw, c)

    def bwd(entry, gy, dims):
        _, gx, gxg = guarded(n * hw * c)
        outs = [guarded(n * c) for _ in range(2)] + [guarded(c) for _ in range(2)]
        ws, wsg = _poisoned(n * chunks * c * 3, c * 3)
        H.call(entry, gy, xd, bd, m, r, gd, gx, *[o[1] for o in outs], ws, *dims, SLOPE, st)
        torch.cuda.synchronize()
        assert untouched(gxg) and bool(torch.isnan(wsg).all()) and all(untouched(o[2]) for o in outs)
        return dict(zip(("gx", "a", "b", "gg", "gb"), [gx] + [o[1] for o in outs]))
    got = bwd("smsut_instnorm_pool_bwd", gypd, (n, h, w, c))
    gfull = torch.empty(n * hw * c, device="cuda")
    H.call("smsut_avgpool2_bwd", gypd, gfull, n, h, w, c, st)
    assert_same(bwd("smsut_instnorm_bwd", gfull, (n, hw, c)), got, "differs from smsut_avgpool2_bwd + smsut_instnorm_bwd")
    mask = aff32(x, mh, rh, gam_, bet) > 0
    gz = R.upsample(gyp, h, w).astype(np.float64) * 0.25 * np.where(mask, 1.0, s32)
    xh = dd * rh.astype(np.float64)[:, None, :]
    K = accum_len(n, c, hw)
    a, b = gz.mean(1), (gz * xh).mean(1)
    da = (gam(K) + U32) * np.abs(gz).mean(1) + U32 * np.abs(a) + 1e-300
    db = (gam(K) + 4 * U32) * np.abs(gz * xh).mean(1) + U32 * np.abs(b) + 1e-300
    gr = p
    ref_gx = gr * (gz - a[:, None, :] - xh * b[:, None, :])
    bound_gx = np.abs(gr) * (da[:, None, :] + np.abs(xh) * db[:, None, :] +
                             R.C_B * U32 * (np.abs(gz) + np.abs(a)[:, None, :] + np.abs(xh * b[:, None, :]))) + 1e-300
    refs = {"gx": (ref_gx, bound_gx), "a": (a, da), "b": (b, db),
            "gg": (hw * b.sum(0), hw * db.sum(0) * (1 + U32) + U32 * np.abs(hw * b.sum(0)) + 1e-300),
            "gb": (hw * a.sum(0), hw * da.sum(0) * (1 + U32) + U32 * np.abs(hw * a.sum(0)) + 1e-300)}
    check_bwd(got, refs, shape, f"instnorm_pool_bwd {name}")


# ---- 6. argument checks ------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_return_the_error_code_and_launch_nothing(H):
    """every SMSUT_REQUIRE of the four pool entries (and the null amax / tickets of _amax / _fin): -1, no output touched -- also for
    H * W * C >= 2^31, which is passed by arguments only, on tiny buffers (a launch would index far outside them; the plain
    InstanceNorm entries, whose check precedes their first launch as well, get one such call each) -- and a valid call afterwards
    succeeds."""
    lib = H.load()
    shape = (2, 6, 10, 4)
    n, h, w, c = shape
    d = R.tail_inputs(shape, 501)
    g = {k: dev(v) for k, v in d.items()}
    st = H.stream_ptr()

    def p(t):
        return None if t is None else ctypes.c_void_p(t.data_ptr())
    outs = [torch.full((n * h * w * c + 64,), NAN, device="cuda") for _ in range(12)]
    idx = torch.full((n * h * w * c,), IDX_FILL, dtype=torch.uint8, device="cuda")
    tk = _tickets(n)
    big = (1 << 15, 1 << 15, 4)                                                 # H * W fits an int, H * W * C = 2^32
    ta = tail_args(g, True)

    def fwd_pool(hh, ww, cc, args=ta, half=0):
        return lib.smsut_restail_fwd_pool(*[p(t) for t in args], p(outs[0]), p(outs[1]), p(idx), n, hh, ww, cc, SLOPE, half, st)

    def bwd_pool(hh, ww, cc, args=ta, half=0, gp=outs[11]):
        return lib.smsut_restail_bwd_pool(p(g["gout"]), p(gp), p(idx), *[p(t) for t in args], *[p(o) for o in outs[:10]], p(tk), None,
                                          n, hh, ww, cc, SLOPE, half, st)

    def in_fwd(hh, ww, cc):
        return lib.smsut_instnorm_pool_fwd_partials(p(g["y2"]), p(g["g2"]), p(g["b2"]), p(outs[0]), p(outs[1]), p(outs[2]), p(g["s"]), 1,
                                                    n, hh, ww, cc, R.EPS, SLOPE, st)

    def in_bwd(hh, ww, cc, beta=g["b2"]):
        return lib.smsut_instnorm_pool_bwd(p(g["gout"]), p(g["y2"]), p(beta), p(g["m2"]), p(g["r2"]), p(g["g2"]), *[p(o) for o in outs[:5]],
                                           p(outs[5]), n, hh, ww, cc, SLOPE, st)
    outs[11].zero_()                                                            # (gp: an input)
    no_sc = tail_args(g, False)
    no_b2, no_bs = tail_args(g, True, b2=False), tail_args(g, True, bs=False)
    for f in (fwd_pool, bwd_pool, in_fwd, in_bwd):
        assert f(h + 1, w, c) == -1 and f(h, w + 1, c) == -1, f.__name__       # odd H or W
        assert f(*big) == -1, f.__name__                                        # H * W * C >= 2^31
        assert f(h, w, 0) == -1 and f(0, w, c) == -1, f.__name__
    assert fwd_pool(6, 10, 6) == -1 and bwd_pool(6, 10, 6) == -1                # whole channel quads
    for half in (0, 1):                                                         # no shortcut, a beta missing: fp32 and fp16 storage
        assert fwd_pool(h, w, c, no_sc, half) == -1 and bwd_pool(h, w, c, no_sc, half) == -1
        assert fwd_pool(h, w, c, no_b2, half) == -1 and bwd_pool(h, w, c, no_b2, half) == -1
        assert fwd_pool(h, w, c, no_bs, half) == -1 and bwd_pool(h, w, c, no_bs, half) == -1
    assert bwd_pool(h, w, c, gp=None) == -1 and in_bwd(h, w, c, beta=None) == -1
    common = [p(g["gout"]), p(g["gout"]), *[p(t) for t in ta], *[p(o) for o in outs[:10]]]
    assert lib.smsut_restail_bwd_amax(*common, None, n, h * w, c, SLOPE, st) == -1       # null amax
    assert lib.smsut_restail_bwd_fin(*common, None, n, h * w, c, SLOPE, st) == -1        # null tickets
    assert lib.smsut_restail_bwd_hs(*[p(g["gout"]), p(g["gout"]), *[p(t) for t in no_b2], *[p(o) for o in outs[:10]]], None, n, h * w, c,
                                    SLOPE, st) == -1                                     # fp16 storage without a beta
    assert lib.smsut_restail_fwd_hs(*[p(t) for t in no_sc], p(outs[0]), n, h * w, c, SLOPE, st) == -1
    # the plain InstanceNorm entries check H * W * C < 2^31 before their first launch too (HW = 2^30 fits an int)
    hwb, x, ga, be, m, r = 1 << 30, p(g["y2"]), p(g["g2"]), p(g["b2"]), p(g["m2"]), p(g["r2"])
    o = [p(t) for t in outs]
    assert lib.smsut_instnorm_fwd(x, ga, be, o[0], o[1], o[2], o[3], n, hwb, 4, R.EPS, SLOPE, 1, st) == -1
    for f in (lib.smsut_instnorm_fwd_partials, lib.smsut_instnorm_fwd_partials_hs, lib.smsut_instnorm_fwd_partials_hs2):
        assert f(x, ga, be, o[0], o[1], o[2], p(g["s"]), 1, n, hwb, 4, R.EPS, SLOPE, 1, st) == -1
    assert lib.smsut_instnorm_bwd(p(g["gout"]), x, be, m, r, ga, o[0], o[1], o[2], o[3], o[4], o[5], n, hwb, 4, SLOPE, st) == -1
    assert lib.smsut_instnorm_bwd2(p(g["gout"]), None, None, p(g["gout"]), x, be, m, r, ga, m, r, o[0], o[1], o[2], o[3], o[4], n, hwb, 4,
                                   SLOPE, st) == -1
    torch.cuda.synchronize()
    for o in outs[:11]:
        assert bool(torch.isnan(o).all()), "a refused call launched something"
    assert bool((idx == IDX_FILL).all()) and int(tk[:n].abs().sum()) == 0
    # ... and the device is fine afterwards: valid calls succeed
    out, pooled, ix = run_fwd_pool(H, g, shape, True, False)
    check_pooled(host(out), host(pooled), host(ix), shape)
    run_bwd_pool(H, g, g["gout"], dev(np.ones((n, h // 2, w // 2, c), np.float32)), ix, shape, False, tickets=True, amax=True)
