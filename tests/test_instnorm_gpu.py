"""InstanceNorm statistics against plain fp64 references, per (image, channel), in every reduction regime of csrc/norm.hip and of
the in-launch finalize (csrc/common.h).

The statistics are fp32 partial sums per chunk (or conv tile) combined in fp64.  Which code combines them depends on the shape:
``fin_emit`` (one chunk), ``in_moments_final`` (2-16 chunks: one lane per chunk; 17-256: strided lanes; > 256: several load
rounds; channel slabs), ``fin_image`` / ``fin_image3`` at the end of the persistent conv kernels and of the residual tail's
backward.  The regime tables below are checked on the CPU by test_instnorm_regimes_cpu.py, so a change of ``pick_chunk`` or of
the conv tile shapes that moves a case into another regime fails there instead of silently dropping the coverage.

Every bound on a statistic is derived a priori from the kernel's accumulation structure (``accum_len``) with the classic
summation bound |fl(sum) - sum| <= gamma_K * sum |x_i|, gamma_K = K u / (1 - K u), u = 2^-24 -- not fitted to GPU numbers."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import elem_rel_err, l2_rel, rel_err
from norm_test_helpers import _check_guards, _poisoned, _tickets, aff32, gpu_mask

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24            # fp32 unit roundoff
SLOPE = 0.01


@pytest.fixture(scope="module")
def ops():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops as o
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return o


@pytest.fixture(scope="module")
def H():
    from smsut_amd import _hip
    return _hip


def eps64(ops):
    return float(np.float32(ops.IN_EPS))          # the kernels get eps as a float and widen it


def planes(n, c, h, w, seed, lo=0.01, hi=3.0):
    """x[n, c] = s * (z + o): every (image, channel) its own scale (log-uniform in [lo, hi]) and offset (|o| <= 1, so mean / std
    <= ~1 here), so that a leak of one image's sums into another's cannot hide."""
    r = np.random.RandomState(seed)
    s = np.exp(r.uniform(np.log(lo), np.log(hi), (n, c, 1, 1)))
    o = r.uniform(-1.0, 1.0, (n, c, 1, 1))
    return torch.from_numpy((r.standard_normal((n, c, h, w)) + o) * s).float()


def rnd(*shape, seed=0, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape) * scale).float()


def gpu(t):
    return t.cuda().contiguous(memory_format=torch.channels_last)


def affine(c, seed):
    return 1 + 0.2 * rnd(c, seed=seed), 0.3 * rnd(c, seed=seed + 1)


# ---- the reduction structure of in_moments_partial (mirrors pick_chunk / slab_count, norm.hip) ---------------------------------
def pick_chunk(hw, c, n):
    if hw <= 256 and c % 4 == 0:
        return hw
    ppc = 2048
    while ppc > 256 and n * -(-hw // ppc) < 1024:
        ppc >>= 1
    return ppc


def slab_count(n, chunks, c, vec):
    if vec != 4:
        return 1
    cv, z = c // 4, 1
    while n * chunks * z < 512 and cv % (2 * z) == 0 and cv // (2 * z) >= 4:
        z *= 2
    return z


def in_regime(n, c, hw):
    """(pixels per chunk, chunks, channel slabs, VEC) of the partial-sum launch"""
    ppc = pick_chunk(hw, c, n)
    chunks = -(-hw // ppc)
    vec = 4 if c % 4 == 0 else 1
    return ppc, chunks, slab_count(n, chunks, c, vec), vec


def accum_len(n, c, hw):
    """K: the most fp32 additions any one term of a chunk sum goes through in in_moments_partial.  A thread adds every `rows`-th
    pixel of its chunk serially (L terms), then the block combines: power-of-two TC <= 64 -> xor tree over the rows inside the wave
    (log2(64 / TC) levels) + the 4 wave totals added from 0.f (4); otherwise one thread adds all `rows` thread totals serially.
    The fp64 combine of the chunk sums adds (chunks + 16) * 2^-53 relative -- negligible, covered by the + 1 below."""
    ppc, chunks, z, vec = in_regime(n, c, hw)
    cv = c // vec // z
    tc = min(cv, 256)
    rows = 256 // tc
    L = -(-min(ppc, hw) // rows)
    D = int(math.log2(64 // tc)) + 4 if tc <= 64 and tc & (tc - 1) == 0 else rows
    return L + D + 1


def gam(k):
    return k * U32 / (1 - k * U32)


def fwd_stat_bounds(x64, K, eps):
    """Per-(n, c) a-priori bounds of the finalised (mean, rstd) from K-step fp32 sums of x and x^2 (x^2 by fma: exact product).
      S1 = sum x   : |dS1| <= g_K sum|x|           -> |dm| <= g_K mean|x| (+ u |m|: the fp32 store)
      S2 = sum x^2 : |dS2| <= g_{K+1} sum x^2       (K + 1: in case the product is rounded on its own)
      var = S2/M - m^2: |dvar| <= g_{K+1} E[x^2] + 2 |m| g_K E|x| + (g_K E|x|)^2
      rstd = (var + eps)^-1/2: with r = |dvar| / (var + eps) < 1, |drstd| / rstd <= r / (2 (1 - r)^1.5) (+ u: the fp32 store).
    For x = mu + sigma z, E[x^2] = mu^2 + sigma^2 and E|x| <= sqrt(E[x^2]): the rstd bound is ~ 3 g_K (1 + mu^2/sigma^2) / 2 -- the
    cancellation of E[x^2] - m^2 grows with the offset.  For a constant plane (var = 0) it is 3 g_K c^2 / (2 eps): eps magnifies the
    residue of the fp32 partials -- the scheme's worst case."""
    a1 = x64.abs().mean((2, 3)).numpy()
    a2 = (x64 * x64).mean((2, 3)).numpy()
    m = x64.mean((2, 3)).numpy()
    var = x64.var((2, 3), unbiased=False).numpy()
    g, g1 = gam(K), gam(K + 1)
    dm = g * a1 + U32 * np.abs(m) + 1e-300
    dvar = g1 * a2 + 2 * np.abs(m) * g * a1 + (g * a1) ** 2
    r = dvar / (var + eps)
    assert (r < 0.5).all(), "bound outside its validity range"
    return dm, r / (2 * (1 - r) ** 1.5) + U32


def ref_stats(x64, eps):
    m = x64.mean((2, 3))
    return m.numpy(), (1.0 / torch.sqrt(x64.var((2, 3), unbiased=False) + eps)).numpy()


def ref_act(x64, g64, b64, eps, mask):
    yn = F.instance_norm(x64, weight=g64, bias=b64, eps=eps)
    return yn if mask is None else torch.where(mask, yn, yn * SLOPE)


# ---- regimes (N, C, H, W) ------------------------------------------------------------------------------------------------------
# one tuple per regime named in the id; test_instnorm_regimes_cpu.py asserts the regime of each
FWD_CASES = [
    ("one_chunk_vec4", (3, 8, 16, 16)),
    ("one_chunk_vec1_c5", (3, 5, 16, 16)),
    ("one_chunk_vec1_c6", (2, 6, 12, 12)),
    ("chunks_8_ragged", (2, 8, 40, 50)),
    ("chunks_16", (2, 8, 64, 64)),
    ("chunks_17_ragged", (2, 8, 65, 66)),
    ("chunks_47_ragged", (2, 4, 100, 120)),
    ("chunks_256", (1, 8, 256, 256)),
    ("chunks_352_ragged", (1, 8, 300, 300)),
    ("chunks_1024", (1, 16, 512, 512)),
    ("slabs_8", (16, 128, 32, 32)),
    ("slabs_16", (16, 256, 16, 16)),
    ("c12", (2, 12, 30, 30)),
    ("c20", (2, 20, 16, 16)),
    ("c24", (4, 24, 24, 24)),
    ("c96_slabs", (2, 96, 20, 20)),
    ("vec1_multi_chunk", (2, 6, 40, 50)),
    ("n16_256sq", (16, 8, 256, 256)),
    ("n32_256sq", (32, 4, 256, 256)),
]
# the backward passes: the same regimes, at sizes that keep the fp64 autograd references within the file's time budget
BWD_CASES = [(k, {"chunks_1024": (1, 4, 512, 512), "n16_256sq": (16, 4, 256, 256)}.get(k, s)) for k, s in FWD_CASES]


def _ids(cases):
    return [k for k, _ in cases]


# ---- 1a. forward statistics and output -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [True, False], ids=["lrelu", "identity"])
@pytest.mark.parametrize("name,shape", FWD_CASES, ids=_ids(FWD_CASES))
def test_forward_statistics_per_plane_vs_fp64(ops, name, shape, act):
    n, c, h, w = shape
    eps = eps64(ops)
    x = planes(n, c, h, w, seed=11)
    g, b = affine(c, 21)
    y, mean, rstd = ops.InstNormActFn.apply(gpu(x), g.cuda(), b.cuda(), SLOPE, act)
    x64 = x.double()
    rm, rr = ref_stats(x64, eps)
    dm, drel = fwd_stat_bounds(x64, accum_len(n, c, h * w), eps)
    em = np.abs(mean.cpu().numpy() - rm)
    er = np.abs(rstd.cpu().numpy() / rr - 1)
    assert (em <= dm).all(), (name, float((em / dm).max()), np.unravel_index(np.argmax(em / dm), em.shape))
    assert (er <= drel).all(), (name, float((er / drel).max()), np.unravel_index(np.argmax(er / drel), er.shape))
    mask = gpu_mask(x, mean, rstd, g, b) if act else None
    ry = ref_act(x64, g.double(), b.double(), eps, mask).numpy()
    yg = y.detach().cpu().numpy()
    assert rel_err(yg, ry) < 1e-5, (name, rel_err(yg, ry))
    assert elem_rel_err(yg, ry) < 1e-4, (name, elem_rel_err(yg, ry))


# ---- 1b. first-order backward, called through the C ABI so that a = mean(gz), b = mean(gz * xhat) are visible ---------------------
def _bwd_refs(x, g, b, mean, rstd, gy, eps, act):
    """fp64 autograd of act(IN(x)) with the kernel's mask; a, b, xhat, gz from the same fp64 statistics."""
    x64 = x.double().requires_grad_(True)
    g64, b64 = g.double().requires_grad_(True), b.double().requires_grad_(True)
    mask = gpu_mask(x, mean, rstd, g, b) if act else None
    y = ref_act(x64, g64, b64, eps, mask)
    y.backward(gy.double())
    xd = x.double()
    m = xd.mean((2, 3), keepdim=True)
    xh = (xd - m) / torch.sqrt(xd.var((2, 3), unbiased=False, keepdim=True) + eps)
    gz = gy.double() * (mask.double() * (1 - SLOPE) + SLOPE if act else 1.0)
    return x64.grad.numpy(), g64.grad.numpy(), b64.grad.numpy(), gz, xh


def _ab_bounds(gz, xh, K, dm_rs, drel):
    """|da| <= (g_K + u) E|gz| (+u|a|); |db| <= (g_K + 4u) E|gz xh| + E|gz| (dm rstd + |xh| drstd/rstd) (+u|b|): the sums of gz
    (one rounding for the slope product) and gz * xhat (xhat = (x - m) r: two roundings, the product fused or one more), and the
    kernel's xhat built from its own fp32 (mean, rstd), whose error bounds come from the forward (fwd_stat_bounds)."""
    ea = gz.abs().mean((2, 3)).numpy()
    eb = (gz * xh).abs().mean((2, 3)).numpy()
    eab = (gz.abs() * (1 + xh.abs())).mean((2, 3)).numpy()
    a = gz.mean((2, 3)).numpy()
    bb = (gz * xh).mean((2, 3)).numpy()
    da = (gam(K) + U32) * ea + U32 * np.abs(a)
    db = (gam(K) + 4 * U32) * eb + eab * np.maximum(dm_rs, drel) + U32 * np.abs(bb)
    return a, bb, da, db


@pytest.mark.parametrize("act", [True, False], ids=["lrelu", "identity"])
@pytest.mark.parametrize("name,shape", BWD_CASES, ids=_ids(BWD_CASES))
def test_first_order_backward_per_plane_vs_fp64(ops, H, name, shape, act):
    n, c, h, w = shape
    hw, eps = h * w, eps64(ops)
    x = planes(n, c, h, w, seed=12)
    g, b = affine(c, 22)
    gy = rnd(n, c, h, w, seed=32)
    xd = gpu(x)
    _, mean, rstd = ops.InstNormActFn.apply(xd, g.cuda(), b.cuda(), SLOPE, act)
    chunks = H.call("smsut_in_chunks", n, hw, c)
    ws = torch.full((n * chunks * c * 3 + 4096,), float("nan"), device="cuda")      # every partial read must have been written
    gx = torch.empty_like(xd)
    a_m, b_m = torch.empty(n, c, device="cuda"), torch.empty(n, c, device="cuda")
    gg, gb = torch.empty(c, device="cuda"), torch.empty(c, device="cuda")
    H.call("smsut_instnorm_bwd", gpu(gy), xd, b.cuda() if act else None, mean, rstd, g.cuda(), gx, a_m, b_m, gg, gb, ws, n, hw, c,
           SLOPE, H.stream_ptr())
    torch.cuda.synchronize()
    rgx, rgg, rgb, gz, xh = _bwd_refs(x, g, b, mean, rstd, gy, eps, act)
    dm, drel = fwd_stat_bounds(x.double(), accum_len(n, c, hw), eps)
    ra, rb, da, db = _ab_bounds(gz, xh, accum_len(n, c, hw), dm * rstd.cpu().double().numpy(), drel)
    ea, eb = np.abs(a_m.cpu().numpy() - ra), np.abs(b_m.cpu().numpy() - rb)
    assert (ea <= da).all(), (name, float((ea / da).max()))
    assert (eb <= db).all(), (name, float((eb / db).max()))
    # ggamma = sum_n M b, gbeta = sum_n M a: per channel, bounded by the sum of the per-image bounds (+ the fp32 store)
    egg, egb = np.abs(gg.cpu().numpy() - rgg), np.abs(gb.cpu().numpy() - rgb)
    assert (egg <= hw * db.sum(0) + U32 * np.abs(rgg) * 2).all(), (name, float((egg / (hw * db.sum(0))).max()))
    assert (egb <= hw * da.sum(0) + U32 * np.abs(rgb) * 2).all(), (name, float((egb / (hw * da.sum(0))).max()))
    gxg = gx.cpu().numpy()
    assert rel_err(gxg, rgx) < 2e-5, (name, rel_err(gxg, rgx))
    assert elem_rel_err(gxg, rgx) < 2e-4, (name, elem_rel_err(gxg, rgx))


# ---- 1c. double backward (WGAN-GP's x_hat pass) --------------------------------------------------------------------------------
def _double_backward(ops, x, g, b, gy, v, wg, wb, mode):
    """mode 'input_only': the production form -- gx alone, inside ops.input_grads_only(); 'affine': gx, ggamma, gbeta all used
    downstream (ug / ub non-null); 'affine_only': only ggamma / gbeta used (v is None in InstNormActBwdFn.backward).
    Returns d/dgy, d/dx, d/dgamma of the loss, on the GPU path and in fp64 (autograd of autograd, with the kernel's mask)."""
    xd, gd, bd = gpu(x).requires_grad_(True), g.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    gyd = gpu(gy).requires_grad_(True)
    yd, mean, rstd = ops.InstNormActFn.apply(xd, gd, bd, SLOPE, True)
    if mode == "input_only":
        with ops.input_grads_only():
            (gxd,) = torch.autograd.grad(yd, xd, gyd, create_graph=True)
        loss = (gxd * gpu(v)).sum()
    else:
        gxd, ggd, gbd = torch.autograd.grad(yd, (xd, gd, bd), gyd, create_graph=True)
        loss = (ggd * wg.cuda()).sum() + (gbd * wb.cuda()).sum()
        if mode == "affine":
            loss = loss + (gxd * gpu(v)).sum()
    got = torch.autograd.grad(loss, (gyd, xd, gd), allow_unused=True)
    got = [np.zeros(t.shape, np.float32) if r is None else r.cpu().numpy() for r, t in zip(got, (gyd, xd, gd))]

    eps = eps64(ops)
    mask = gpu_mask(x, mean.detach(), rstd.detach(), g, b)
    x64, g64, b64 = x.double().requires_grad_(True), g.double().requires_grad_(True), b.double().requires_grad_(True)
    gy64 = gy.double().requires_grad_(True)
    y64 = ref_act(x64, g64, b64, eps, mask)
    gx64, gg64, gb64 = torch.autograd.grad(y64, (x64, g64, b64), gy64, create_graph=True)
    if mode == "input_only":
        rl = (gx64 * v.double()).sum()
    else:
        rl = (gg64 * wg.double()).sum() + (gb64 * wb.double()).sum()
        if mode == "affine":
            rl = rl + (gx64 * v.double()).sum()
    ref = torch.autograd.grad(rl, (gy64, x64, g64), allow_unused=True)
    ref = [np.zeros(t.shape) if r is None else r.detach().numpy() for r, t in zip(ref, (gy64, x64, g64))]
    return got, ref


@pytest.mark.parametrize("mode", ["input_only", "affine", "affine_only"])
@pytest.mark.parametrize("name,shape", BWD_CASES, ids=_ids(BWD_CASES))
def test_double_backward_vs_fp64(ops, name, shape, mode):
    n, c, h, w = shape
    x = planes(n, c, h, w, seed=13)
    g, b = affine(c, 23)
    gy, v = rnd(n, c, h, w, seed=33), rnd(n, c, h, w, seed=43)
    wg, wb = rnd(c, seed=53), rnd(c, seed=54)
    (d_gy, d_x, d_g), (r_gy, r_x, r_g) = _double_backward(ops, x, g, b, gy, v, wg, wb, mode)
    assert rel_err(d_gy, r_gy) < 5e-5, (name, mode, rel_err(d_gy, r_gy))
    assert elem_rel_err(d_gy, r_gy) < 5e-4, (name, mode, elem_rel_err(d_gy, r_gy))
    assert rel_err(d_x, r_x) < 5e-5, (name, mode, rel_err(d_x, r_x))
    assert l2_rel(d_x, r_x) < 2e-5, (name, mode, l2_rel(d_x, r_x))
    if mode == "affine_only":               # ggamma, gbeta do not depend on gamma (the mask is fixed): exactly zero
        assert not np.any(d_g), d_g
    else:
        assert rel_err(d_g, r_g) < 5e-5, (name, mode, rel_err(d_g, r_g))
        assert elem_rel_err(d_g, r_g, floor=0.05) < 1e-3, (name, mode, elem_rel_err(d_g, r_g, floor=0.05))


# ---- 1d. edge planes -----------------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(2, 8, 16, 16), (2, 8, 40, 50), (2, 6, 16, 16), (1, 8, 300, 300)]      # one chunk (HW = 2^8), ragged chunks, VEC=1,
                                                                                      # > 256 chunks


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_constant_planes_are_exact(ops, shape):
    """All-background slices: planes of 0, 1 and 10 among random ones.  Every chunk sum of such a plane is exact in fp32, so the
    variance is exactly 0 (E[x^2] - m^2 in fp64 from exact sums; with M not a power of two 1/M is inexact: a residue ~1e-16 c^2,
    clamped at 0 from below) and rstd = fp32(1 / sqrt(fp64(fp32(eps)))) -- bit for bit when M is a power of two, within 1 ulp
    otherwise; y = act(beta) bit for bit (in_affine: fma(0, rstd * gamma, beta)).  First and second derivatives are finite and
    meet the normal bars."""
    n, c, h, w = shape
    hw, eps = h * w, eps64(ops)
    x = planes(n, c, h, w, seed=14)
    consts = {(0, 1): 0.0, (0, 2): 1.0, (n - 1, 3): 10.0, (n - 1, 0): 1.0}
    for (i, j), val in consts.items():
        x[i, j] = val
    g, b = affine(c, 24)
    b[1], b[2] = -abs(float(b[1])) - 0.1, abs(float(b[2])) + 0.1          # one plane on each side of the activation
    y, mean, rstd = ops.InstNormActFn.apply(gpu(x), g.cuda(), b.cuda(), SLOPE, True)
    yg, mg, rg = y.detach().cpu().numpy(), mean.cpu().numpy(), rstd.cpu().numpy()
    r_eps = np.float32(1.0 / math.sqrt(eps))
    for (i, j), val in consts.items():
        assert mg[i, j] == np.float32(val), (i, j, mg[i, j])
        if hw & (hw - 1) == 0:
            assert rg[i, j] == r_eps, (i, j, rg[i, j], r_eps)
        else:
            assert abs(int(rg[i, j].view(np.int32)) - int(r_eps.view(np.int32))) <= 1, (i, j, rg[i, j], r_eps)
        bj = np.float32(b[j])
        want = bj if bj > 0 else np.float32(bj * np.float32(SLOPE))
        assert np.all(yg[i, j] == want), (i, j, np.unique(yg[i, j])[:4], want)
    # derivatives: finite, and the normal bars against fp64
    gy = rnd(n, c, h, w, seed=34)
    xd, gd, bd = gpu(x).requires_grad_(True), g.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    yd, _, _ = ops.InstNormActFn.apply(xd, gd, bd, SLOPE, True)
    yd.backward(gpu(gy))
    rgx, rgg, rgb, _, _ = _bwd_refs(x, g, b, mean, rstd, gy, eps, True)
    for got, ref in ((xd.grad, rgx), (gd.grad, rgg), (bd.grad, rgb)):
        got = got.cpu().numpy()
        assert np.isfinite(got).all()
        assert rel_err(got, ref) < 2e-5, rel_err(got, ref)
    v, wg, wb = rnd(n, c, h, w, seed=44), rnd(c, seed=55), rnd(c, seed=56)
    for mode in ("input_only", "affine"):
        (d_gy, d_x, d_g), (r_gy, r_x, r_g) = _double_backward(ops, x, g, b, gy, v, wg, wb, mode)
        for got, ref in ((d_gy, r_gy), (d_x, r_x), (d_g, r_g)):
            assert np.isfinite(got).all(), mode
            assert rel_err(got, ref) < 5e-5, (mode, rel_err(got, ref))


@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_inexact_constant_plane_within_the_eps_magnified_bound(ops, shape):
    """A constant that is not exact in the sums (0.3): the fp32 partials of x and x^2 leave a variance residue |dvar| <=
    3 g_K c^2 (K = accum_len), and eps magnifies it: |drstd| / rstd <= 3 g_K c^2 / (2 eps), ~1e-2 at c = 0.3 and K = 12 -- the worst
    case of the {sum, sum^2} scheme (fwd_stat_bounds).  The mean is within g_K c."""
    n, c, h, w = shape
    eps = eps64(ops)
    x = planes(n, c, h, w, seed=15)
    x[0, 1] = 0.3
    x[n - 1, 2] = -0.3
    g, b = affine(c, 25)
    _, mean, rstd = ops.InstNormActFn.apply(gpu(x), g.cuda(), b.cuda(), SLOPE, True)
    x64 = x.double()
    rm, rr = ref_stats(x64, eps)
    dm, drel = fwd_stat_bounds(x64, accum_len(n, c, h * w), eps)
    em, er = np.abs(mean.cpu().numpy() - rm), np.abs(rstd.cpu().numpy() / rr - 1)
    K = accum_len(n, c, h * w)
    print(f"inexact constant: {shape} K {K} rstd err {float(er[0, 1]):.2e}, {float(er[n - 1, 2]):.2e} (bound {float(drel[0, 1]):.2e}); "
          f"mean err/bound {float((em / dm).max()):.3f}")
    assert (em <= dm).all(), float((em / dm).max())
    assert (er <= drel).all(), float((er / drel).max())
    # (the bound is the closed form 3 g_K c^2 / (2 eps) -- 1e-2 on the tree paths (K = 12), 5e-2 where one thread adds the `rows`
    #  thread totals serially (VEC=1, C = 6: K = 50) -- not a blanket)
    assert drel[0, 1] <= 1.25 * 1.5 * gam(K + 1) * 0.09 / eps, (float(drel[0, 1]), K)


@pytest.mark.parametrize("ratio", [10.0, 30.0])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_offset_planes_within_the_derived_bound(ops, shape, ratio):
    """x = mu + sigma z with mu / sigma = 10 and 30: E[x^2] - m^2 from fp32 partials loses ~log10(1 + mu^2/sigma^2) digits.  The
    bound (fwd_stat_bounds): |dm| <= g_K E|x|, |drstd| / rstd <~ 3 g_K (1 + mu^2/sigma^2) / 2 with K = L (per-thread serial adds) +
    D (tree depth) + 1 (fp64 combine) from accum_len -- derived from the kernel, not fitted."""
    n, c, h, w = shape
    eps = eps64(ops)
    r = np.random.RandomState(16)
    sig = np.exp(r.uniform(np.log(0.05), np.log(2.0), (n, c, 1, 1)))
    sgn = np.where(r.uniform(size=(n, c, 1, 1)) < 0.5, -1.0, 1.0)
    x = torch.from_numpy(sig * (ratio * sgn + r.standard_normal((n, c, h, w)))).float()
    g, b = affine(c, 26)
    _, mean, rstd = ops.InstNormActFn.apply(gpu(x), g.cuda(), b.cuda(), SLOPE, True)
    x64 = x.double()
    rm, rr = ref_stats(x64, eps)
    dm, drel = fwd_stat_bounds(x64, accum_len(n, c, h * w), eps)
    em, er = np.abs(mean.cpu().numpy() - rm), np.abs(rstd.cpu().numpy() / rr - 1)
    print(f"offset {ratio}: {shape} mean err/bound {float((em / dm).max()):.3f} rstd err {float(er.max()):.2e} "
          f"(bound {float(drel.max()):.2e}, err/bound {float((er / drel).max()):.3f})")
    assert (em <= dm).all(), float((em / dm).max())
    assert (er <= drel).all(), float((er / drel).max())


# ---- 1e. in-launch finalize (FinRef, common.h) against fp64, on poisoned memory ------------------------------------------------
# (N, H, W): tiles per image 1 (and 1 with every workgroup walking several images), 2, 3, 5, 16, 17, 261 and 300 (> 256, not
# multiples of 256) -- direct (H % 16 != 0) and resident-weight Winograd forms of the persistent kernel
CONV_FIN_SHAPES = [("tiles_1", (256, 16, 16)), ("tiles_1_many_images", (1536, 16, 16)), ("tiles_2", (128, 16, 32)),
                   ("tiles_3", (128, 16, 48)), ("tiles_5", (64, 16, 80)), ("tiles_16", (16, 16, 256)), ("tiles_17", (16, 16, 272)),
                   ("tiles_261", (2, 232, 144)), ("tiles_300", (1, 240, 320))]
# (N, H, W, Cin, Cout): the fused shortcut conv Cin -> Cout, conv2 and its data-gradient Cout -> Cout.  Cin 16 and Cin 32 are two
# kernel instantiations each; Cin 32 also runs the virtual-cat input (two 16-channel halves, which needs Cin % 32 == 0).  The
# 64-channel case runs the streamed-weight Winograd kernel (conv_wino.hip), which carries its own in-launch finalize.
CONV_FIN_CASES = ([(f"{k}-k{ci}", (n, h, w, ci, 32)) for ci in (16, 32) for k, (n, h, w) in CONV_FIN_SHAPES] +
                  [("tiles_16-k64", (4, 64, 64, 64, 64))])


def conv_fin_cat(ci):
    """whether the conv finalize test also runs the virtual-cat input of the fused shortcut conv for this reduction width"""
    return ci % 32 == 0
# (N, HW, C) of the residual tail's backward: chunks per image 1, 2, 3, 5, 16, 17, 352
TAIL_FIN_CASES = [("chunks_1", (2, 256, 32)), ("chunks_2", (2, 512, 32)), ("chunks_3", (3, 768, 32)), ("chunks_5", (2, 1280, 32)),
                  ("chunks_16", (2, 4096, 32)), ("chunks_17", (2, 4352, 32)), ("chunks_352", (1, 90000, 16))]


def _outs(n, c, k):
    """k outputs [N][C], each followed by a sentinel guard (returns the base tensors)"""
    return [torch.full((n * c + 64,), 12345.0, device="cuda") for _ in range(k)]


def _nc(t, n, c):
    return t[:n * c].view(n, c).cpu().double().numpy()


def _conv_k(hw, tiles):
    """K for a conv tile's partial sums: the tile's pixels added one by one (the worst case of any order) + a 64-step tree"""
    return hw // tiles + 64


def _fwd_check(y64, m, r, tiles, eps, what):
    """(mean, rstd) finalised in the launch vs fp64 statistics of the kernel's own output"""
    n, c, h, w = y64.shape
    rm, rr = ref_stats(y64, eps)
    dm, drel = fwd_stat_bounds(y64, _conv_k(h * w, tiles), eps)
    em, er = np.abs(m - rm), np.abs(r / rr - 1)
    assert (em <= dm).all(), (what, float((em / dm).max()))
    assert (er <= drel).all(), (what, float((er / drel).max()))


def _nchw(t):
    """an NHWC-memory [N,H,W,C] buffer as logical NCHW fp64 on the CPU"""
    return t.cpu().double().permute(0, 3, 1, 2)


@pytest.mark.parametrize("name,case", CONV_FIN_CASES, ids=_ids(CONV_FIN_CASES))
def test_conv_in_launch_finalize_vs_fp64_on_poisoned_memory(ops, H, name, case):
    n, h, w, ci, co = case
    hw, eps = h * w, eps64(ops)
    st = H.stream_ptr()
    torch.manual_seed(0)
    assert H.call("smsut_conv2d_fwd_sc_supported", n, h, w, ci, co, 0)
    assert H.call("smsut_conv2d_mfma_persistent", n, h, w, co, co, 3, 0)
    t1 = H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 0)
    t2 = H.call("smsut_conv2d_mfma_tiles", n, h, w, co, co, 3, 0)
    r = np.random.RandomState(17)
    sc_img = torch.from_numpy(np.exp(r.uniform(-2, 1, (n, 1, 1, 1)))).float().cuda()
    off_img = torch.from_numpy(r.uniform(-1, 1, (n, 1, 1, 1))).float().cuda()

    def act_in(c, seed):        # NHWC [N,H,W,c], each image its own scale and offset
        return (torch.randn(n, h, w, c, generator=torch.Generator("cuda").manual_seed(seed), device="cuda") + off_img) * sc_img

    def wt(co_, ci_, k, seed):  # HWIO weights [k][k][ci][co]
        return torch.randn(k, k, ci_, co_, generator=torch.Generator("cuda").manual_seed(seed), device="cuda") / math.sqrt(k * k * ci_)

    # -- conv1 + fused 1x1 shortcut, statistics of both finalised in the launch (and from the virtual cat of two halves) --
    x, xa, xb = act_in(ci, 1), None, None
    w1, wsc = wt(co, ci, 3, 2), wt(co, ci, 1, 3)
    plain = None
    for cat in ((False, True) if conv_fin_cat(ci) else (False,)):
        if cat:
            xa, xb = x[..., :ci // 2].contiguous(), x[..., ci // 2:].contiguous()
            assert H.call("smsut_conv2d_fwd_sc_supported", n, h, w, ci, co, 1)
        runs = []
        for _ in range(2):
            y, ys = torch.empty(n, h, w, co, device="cuda"), torch.empty(n, h, w, co, device="cuda")
            p1, g1 = _poisoned(n * t1 * co * 2, co * 2)
            ps, gs = _poisoned(n * t1 * co * 2, co * 2)
            tk = _tickets(n)
            outs = _outs(n, co, 4)
            H.call("smsut_conv2d_fwd_mfma_stats_sc_fin", xa if cat else x, xb, w1, wsc, y, ys, p1, ps, tk, *outs, eps, n, h, w, ci, co,
                   None, st)
            torch.cuda.synchronize()
            _check_guards([g1, gs], tk, outs, n, co)
            runs.append([y, ys, p1, ps] + outs)
        for a, b in zip(*runs):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "second run differs"
        if cat:                 # the virtual cat is read in the materialised input's order: the same bits
            for k, (a, b) in enumerate(zip(plain, runs[0])):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ("virtual cat differs", k)
        plain = runs[0]
        y, ys, p1, ps, m1, r1, ms, rs = runs[0]
        _fwd_check(_nchw(y), _nc(m1, n, co), _nc(r1, n, co), t1, eps, "conv1")
        _fwd_check(_nchw(ys), _nc(ms, n, co), _nc(rs, n, co), t1, eps, "shortcut")
        # ... and the in-launch combine is the separate launch's, bit for bit
        m_sep, r_sep = torch.empty(n, co, device="cuda"), torch.empty(n, co, device="cuda")
        H.call("smsut_in_finalize_fwd", p1, t1, m_sep, r_sep, n, hw, co, eps, st)
        assert torch.equal(m_sep.view(-1), m1[:n * co]) and torch.equal(r_sep.view(-1), r1[:n * co])

    # -- conv2 on lrelu(IN(y1)) applied while staging, statistics of y2 finalised in the launch --
    y1 = act_in(co, 4)
    m_in = torch.from_numpy(np.float32(r.uniform(-0.5, 0.5, (n, co)))).cuda() * sc_img.view(n, 1) + off_img.view(n, 1) * sc_img.view(n, 1)
    r_in = (1.0 / sc_img.view(n, 1)).expand(n, co).contiguous() * torch.from_numpy(np.float32(r.uniform(0.8, 1.2, (n, co)))).cuda()
    ga, be = (1 + 0.2 * torch.randn(co, device="cuda")), 0.3 * torch.randn(co, device="cuda")
    w2 = wt(co, co, 3, 5)
    runs = []
    for _ in range(2):
        y2 = torch.empty(n, h, w, co, device="cuda")
        p2, g2 = _poisoned(n * t2 * co * 2, co * 2)
        tk = _tickets(n)
        outs = _outs(n, co, 2)
        H.call("smsut_conv2d_fwd_mfma_stats_inaff_fin", y1, w2, y2, p2, m_in, r_in, ga, be, SLOPE, tk, *outs, eps, n, h, w, co, co,
               None, st)
        torch.cuda.synchronize()
        _check_guards([g2], tk, outs, n, co)
        runs.append([y2, p2] + outs)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "second run differs"
    y2, p2, m2, r2 = runs[0]
    _fwd_check(_nchw(y2), _nc(m2, n, co), _nc(r2, n, co), t2, eps, "conv2 inaff")

    # -- data-gradient of conv2 with the IN backward folded in: a = mean(gz), b = mean(gz * xhat(y1)) finalised in the launch --
    gy = act_in(co, 6)
    runs = []
    for _ in range(2):
        gz = torch.empty(n, h, w, co, device="cuda")
        p3, g3 = _poisoned(n * t2 * co * 2, co * 2)
        tk = _tickets(n)
        outs = _outs(n, co, 2)
        H.call("smsut_conv2d_dgrad_mfma_bwdstats_fin", gy, w2, gz, p3, y1, m_in, r_in, ga, be, SLOPE, tk, *outs, n, h, w, co, co, None, st)
        torch.cuda.synchronize()
        _check_guards([g3], tk, outs, n, co)
        runs.append([gz, p3] + outs)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "second run differs"
    gz, p3, am, bm = runs[0]
    gz64 = _nchw(gz)
    xh = (_nchw(y1) - m_in.cpu().double()[:, :, None, None]) * r_in.cpu().double()[:, :, None, None]
    K = _conv_k(hw, t2)
    ra, rb = gz64.mean((2, 3)).numpy(), (gz64 * xh).mean((2, 3)).numpy()
    da = gam(K) * gz64.abs().mean((2, 3)).numpy() + U32 * np.abs(ra)
    db = (gam(K) + 3 * U32) * (gz64 * xh).abs().mean((2, 3)).numpy() + U32 * np.abs(rb)
    ea, eb = np.abs(_nc(am, n, co) - ra), np.abs(_nc(bm, n, co) - rb)
    assert (ea <= da).all(), ("bwdstats a", float((ea / da).max()))
    assert (eb <= db).all(), ("bwdstats b", float((eb / db).max()))


@pytest.mark.parametrize("shortcut", [True, False], ids=["conv_shortcut", "identity"])
@pytest.mark.parametrize("name,nhwc", TAIL_FIN_CASES, ids=_ids(TAIL_FIN_CASES))
def test_restail_bwd_fin_vs_fp64_on_poisoned_memory(ops, H, name, nhwc, shortcut):
    """smsut_restail_bwd_fin: the last-arriving workgroup of an image combines the three sums {gz, gz * y2hat, gz * shat} (fin_image3)
    -- with the conv shortcut and both betas (the in-launch form); the identity shortcut falls back to in_moments_final<2>."""
    n, hw, c = nhwc
    st = H.stream_ptr()
    chunks = H.call("smsut_in_chunks", n, hw, c)
    r = np.random.RandomState(18)
    torch.manual_seed(0)

    def t():
        return torch.from_numpy(np.float32(r.standard_normal((n, hw, c)))).cuda()
    img = torch.from_numpy(np.float32(np.exp(r.uniform(-2, 1, (n, 1, 1))))).cuda()      # each image its own scale
    gout, out, y2, s = t() * img, t(), t() * img + 0.5, t() * img - 0.3

    def stats(v):
        v64 = v.double()
        m = v64.mean(1)
        return m.float(), (1 / torch.sqrt(v64.var(1, unbiased=False) + 1e-5)).float()
    m2, r2 = stats(y2)
    ms, rs = stats(s) if shortcut else (None, None)
    g2, b2 = 1 + 0.2 * torch.randn(c, device="cuda"), 0.3 * torch.randn(c, device="cuda")
    gs_, bs = (1 + 0.2 * torch.randn(c, device="cuda"), 0.3 * torch.randn(c, device="cuda")) if shortcut else (None, None)
    runs = []
    for _ in range(2):
        gy2, gs = torch.empty_like(y2), torch.empty_like(y2)
        ws, guard = _poisoned(n * chunks * c * 3, c * 3)
        tk = _tickets(n)
        outs = _outs(n, c, 3)
        aff = [torch.empty(c, device="cuda") for _ in range(4)]
        H.call("smsut_restail_bwd_fin", gout, out, y2, m2, r2, g2, b2, s if shortcut else y2, ms, rs, gs_, bs, gy2, gs, *outs, aff[0],
               aff[1], aff[2] if shortcut else None, aff[3] if shortcut else None, ws, tk, n, hw, c, SLOPE, st)
        torch.cuda.synchronize()
        _check_guards([guard], tk, outs, n, c)
        runs.append([gy2, gs] + outs + (aff if shortcut else aff[:2]))       # (ggs, gbs: not written without the shortcut)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "second run differs"
    am, bm2, bms = runs[0][2:5]
    # fp64 reference: gz = gout * mask, the mask as the kernel forms it (sign of in_affine(y2) + in_affine(s) in fp32 with both betas,
    # else the sign of `out`)
    y2c, m2c, r2c = y2.cpu(), m2.cpu(), r2.cpu()
    if shortcut:
        def np_(v):
            return v.cpu().numpy()
        pre = (aff32(np_(y2c), np_(m2c), np_(r2c), np_(g2), np_(b2)).astype(np.float64) +
               aff32(np_(s), np_(ms), np_(rs), np_(gs_), np_(bs)))
        mask = pre > 0
    else:
        mask = out.cpu().numpy() > 0
    gz = gout.cpu().double().numpy() * np.where(mask, 1.0, SLOPE)
    y2h = (y2c.double().numpy() - m2c.double().numpy()[:, None, :]) * r2c.double().numpy()[:, None, :]
    sums = [gz, gz * y2h]
    if shortcut:
        sh = (s.cpu().double().numpy() - ms.cpu().double().numpy()[:, None, :]) * rs.cpu().double().numpy()[:, None, :]
        sums.append(gz * sh)
    # K: the tail's partial kernel adds pixel pairs serially per thread (<= ppc / rows + 1) and combines like in_moments_partial
    K = accum_len(n, c, hw) + 2
    for got, v, k in zip((am, bm2, bms), sums, range(3)):
        ref = v.mean(1)
        bound = (gam(K) + 4 * U32) * np.abs(v).mean(1) + U32 * np.abs(ref)
        e = np.abs(_nc(got, n, c) - ref)
        assert (e <= bound).all(), (name, k, float((e / bound).max()))
