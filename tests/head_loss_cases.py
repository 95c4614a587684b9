"""Cases, references and bars of ``tests/test_head_loss_edges_gpu.py``: the CoraNet head kernels (``csrc/coranet.hip``) and the loss half
of ``csrc/dtc.hip`` at block, grid-cap and class-count edges.  CPU only; ``tests/test_head_loss_cases_cpu.py`` pins everything here.

Layout.  The kernels see pixel-major rows, so everything here is ``[N, HW, C]`` (logits, tanh head, sdf) and ``[N, HW]`` (labels, mask);
``as_nchw`` turns rows into the logical NCHW view that ``coranet_ref`` / ``dtc_ref`` take.

References.  Every compared quantity has ``ref64`` (the restatement in fp64) and ``ref32`` (the SAME restatement evaluated in fp32 on the
CPU).  The CoraNet restatement is written here in terms of the statistics the kernels exchange (``sup_stats`` -> ``sup_from_stats``,
``semi_stats`` -> ``semi_from_stats``), because (a) the statistics are compared themselves, (b) the data-parallel form adds statistics of
two half batches, and (c) it states what a label outside ``[0, L]`` does (below); on valid labels it equals ``coranet_ref`` (CPU test).
The DTC loss is ``dtc_ref.dtc_loss`` on the NCHW view.

Labels outside ``[0, L]`` (what ``coranet.hip`` does, pinned by the GPU test): such a pixel has an all-zero one-hot row.  It adds its
head-0 probabilities to ``sum_p`` (the Dice denominators) and nothing else -- no ``tp``, no count, no cross-entropy term in any head.  The
CE(h0) mean still divides by all N * HW pixels; the weighted CE of heads 1 and 2 divide by the weights of the valid pixels.  Its gradient
is therefore the Dice ``sum_p`` term alone.  The same for pseudo labels ``q`` in the pseudo-labelled loss; the mask sums count every pixel.

Bars (all from the references, none from the device):
  * scalars / statistics   |got - ref64| <= 16 max(|ref32 - ref64|, 2^-23 |ref64|)        -- 16: what tests/test_volume_gpu.py gives a
    device result over the fp32 replay; 2^-23 |ref64|: one fp32 ulp of the stored result, so that an accidentally tiny fp32 error of
    the replay does not set an impossible bar
  * gradient tensors, per element   |got_i - ref64_i| <= 16 max(U, 2^-24 |ref64_i|), U = max_i |ref32_i - ref64_i|
  * and the project's standing bars: scalars 1e-6 + 2e-5 |ref|, tensors rel_err < 2e-5
  * counts, 0/1 mask sums, pseudo labels, structurally zero gradients: exact."""
import functools
import math
import types

import numpy as np
import torch
import torch.nn.functional as F

import coranet_ref as CR
import dtc_ref as DR

SMOOTH, EPS = CR.SMOOTH, CR.EPS

# ------------------------------------------------------------------------------------------- launch geometry
TPB, PIX_PER_BLOCK, MAX_BLOCKS = 256, 512, 128          # cora_blocks / dtc_blocks: min(ceil(HW / 512), 128) workgroups of 256 per sample
HW_TABLE = [1, 63, 64, 65, 255, 256, 257, 512, 513, 1300, 65536, 65537, 3 * 65536 + 77]
LARGE = 65536


def blocks(hw):
    return max(1, min(-(-hw // PIX_PER_BLOCK), MAX_BLOCKS))


def geometry(hw):
    """(workgroups per sample, trips of the grid-stride loop, pixels of the last trip)"""
    b = blocks(hw)
    stride = b * TPB
    trips = -(-hw // stride)
    return b, trips, hw - (trips - 1) * stride


def regime(hw):
    """the row of the issue's table that ``hw`` falls in, by computation"""
    b, trips, last = geometry(hw)
    if b == MAX_BLOCKS and trips >= 2:
        if trips == 2 and last == b * TPB:
            return "cap-two-full-trips"
        if last == 1:
            return "cap-third-trip-one-thread"
        return "cap-many-trips-ragged" if trips >= 7 and last % 64 else "cap-other"
    if b == 1 and trips == 1:
        if last < 64:
            return "one-block-partial-wave" if last > 1 else "one-pixel"
        if last == 64:
            return "one-block-exact-wave"
        if last == 65:
            return "one-block-one-past-a-wave"
        return "one-block-full" if last == TPB else "one-block-partial"
    if b == 1:
        return "one-block-second-trip-thread0" if last == 1 else ("one-block-two-full-trips" if last == TPB else "one-block-other")
    if trips == 2 and last % TPB:
        return f"{b}-blocks-ragged"
    return "other"


REGIMES = {"one-pixel", "one-block-partial-wave", "one-block-exact-wave", "one-block-one-past-a-wave", "one-block-partial", "one-block-full",
           "one-block-second-trip-thread0", "one-block-two-full-trips", "2-blocks-ragged", "3-blocks-ragged", "cap-two-full-trips",
           "cap-third-trip-one-thread", "cap-many-trips-ragged"}


def cora_combos(hw):
    """(N, L) per HW: N in {1, 2, 3}, compile-time (1, 2, 4) and runtime L side by side; the large planes at N = 2 only"""
    return [(2, 1), (2, 3)] if hw >= LARGE else [(1, 4), (2, 10), (3, 1), (3, 3)]


def dtc_combos(hw):
    """(N, B, C) per HW: B in {1, N - 1, N}, compile-time (1, 2, 5) and runtime C"""
    return [(2, 1, 2), (2, 2, 3)] if hw >= LARGE else [(1, 1, 5), (2, 1, 3), (3, 2, 2), (3, 3, 16), (3, 1, 1)]


# (w_dc, w_ce), gout[0] of the supervised backward; gout = 0 is checked for exact zeros without a reference
SUP_COMBOS = [((0.5, 0.5), 1.0), ((1.0, 0.0), -1.7), ((0.0, 1.0), -1.7), ((0.5, 0.5), -1.7)]
SUP_COMBOS_LARGE = [((0.5, 0.5), -1.7), ((0.0, 1.0), 1.0)]
# gout, cw of the pseudo-labelled backward
SEMI_COMBOS = [((1.0, 0.1), 0.7), ((0.0, 1.0), 0.7), ((1.0, 0.0), 0.7), ((-0.6, 0.3), 0.7), ((1.0, 0.1), 0.0)]
SEMI_COMBOS_LARGE = [((-0.6, 0.3), 0.7), ((0.0, 1.0), 0.7)]
# k, gout of the DTC backward
DTC_COMBOS = [(1500.0, (1.0, 0.0)), (1500.0, (0.0, 1.0)), (1500.0, (0.3, 0.7)), (1.0, (-1.0, 2.0)), (1.0, (0.0, 1.0))]
DTC_COMBOS_LARGE = [(1500.0, (0.3, 0.7)), (1500.0, (0.0, 1.0)), (1.0, (-1.0, 2.0))]


# ------------------------------------------------------------------------------------------- bars
def scalar_bar(ref64, ref32):
    ref64, ref32 = np.asarray(ref64, dtype=np.float64), np.asarray(ref32, dtype=np.float64)
    return 16.0 * np.maximum(np.abs(ref32 - ref64), 2.0 ** -23 * np.abs(ref64))


def tensor_bar(ref64, ref32):
    ref64, ref32 = np.asarray(ref64, dtype=np.float64), np.asarray(ref32, dtype=np.float64)
    u = float(np.abs(ref32 - ref64).max()) if ref64.size else 0.0
    return 16.0 * np.maximum(u, 2.0 ** -24 * np.abs(ref64))


WORST = {}          # family -> worst err / bar seen in this process (printed by the GPU test, recorded in DESIGN.md section 5)


def _ratio(err, bar):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    return float(np.max(r)) if r.size else 0.0


def _note(family, ratio):
    if family is not None and math.isfinite(ratio):
        WORST[family] = max(WORST.get(family, 0.0), ratio)


def check_scalars(tag, got, ref64, ref32, family=None):
    """every entry finite, within the reference-derived bar and within the standing 1e-6 + 2e-5 |ref|"""
    got, ref64, ref32 = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape, (tag, got.shape, ref64.shape, ref32.shape)
    err, bar = np.abs(got - ref64), scalar_bar(ref64, ref32)
    ratio = _ratio(err, bar)
    print(f"{tag}: err {err.max():.3g} bar {bar[np.argmax(err)]:.3g} err/bar {ratio:.3g}")
    assert np.all(np.isfinite(got)), (tag, got)
    assert np.all(err <= bar), (tag, got, ref64, err, bar)
    assert np.all(err <= 1e-6 + 2e-5 * np.abs(ref64)), (tag, got, ref64)
    _note(family, ratio)
    return ratio


def check_tensor(tag, got, ref64, ref32, family=None):
    """every element finite and within the per-element bar; rel_err < 2e-5; an all-zero reference wants exact zeros"""
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    ref64 = np.asarray(ref64.detach().numpy() if torch.is_tensor(ref64) else ref64, dtype=np.float64)
    ref32 = np.asarray(ref32.detach().numpy() if torch.is_tensor(ref32) else ref32, dtype=np.float64)
    assert got.shape == ref64.shape == ref32.shape, (tag, got.shape, ref64.shape, ref32.shape)
    assert np.all(np.isfinite(got)), tag
    top = float(np.abs(ref64).max())
    if top == 0.0:
        assert not got.any(), (tag, "an all-zero reference wants exact zeros")
        print(f"{tag}: exactly zero")
        return 0.0
    err, bar = np.abs(got - ref64), tensor_bar(ref64, ref32)
    ratio, rel = _ratio(err, bar), float(err.max() / max(top, 1e-30))          # (conftest.rel_err, the standing bar's measure)
    print(f"{tag}: err {err.max():.3g} bar {bar.flat[np.argmax(err)]:.3g} err/bar {ratio:.3g} rel_err {rel:.3g}")
    assert np.all(err <= bar), (tag, ratio)
    assert rel < 2e-5, (tag, rel)
    _note(family, ratio)
    return ratio


def check_counts(tag, got, want):
    """exact integers (all below 2^24, so fp32 holds them)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert want.max(initial=0.0) < 2 ** 24
    assert np.array_equal(got, want), (tag, got, want)


# ------------------------------------------------------------------------------------------- layout
def as_nchw(rows):
    """rows [N, HW, C] -> the logical NCHW view [N, C, HW, 1] of the same memory; [N, HW] -> [N, HW, 1]"""
    return rows.permute(0, 2, 1).unsqueeze(-1) if rows.dim() == 3 else rows.unsqueeze(-1)


def head(z, k, L):
    return torch.cat([z[..., :1], z[..., 1 + k * L:1 + (k + 1) * L]], -1)


def one_hot(lab, L, dtype):
    """[.., L+1]; a label outside [0, L] gives an all-zero row"""
    valid = (lab >= 0) & (lab <= L)
    return F.one_hot(lab.clamp(0, L), L + 1).to(dtype) * valid.unsqueeze(-1).to(dtype)


# ------------------------------------------------------------------------------------------- CoraNet restatement (dtype of z)
def _dice_triplets(p, hot, dims):
    """[.., L+1, 3] = {tp, sum_p, count} per class, summed over ``dims``"""
    return torch.stack([(p * hot).sum(dims), p.sum(dims), hot.sum(dims)], -1)


def sup_stats(z, y, w_con, w_rad):
    """flat [3(L+1)+3] as smsut_cora_sup_stats leaves them"""
    L = (z.shape[-1] - 1) // 3
    hot = one_hot(y, L, z.dtype)
    tri = _dice_triplets(torch.softmax(head(z, 0, L), -1), hot, (0, 1))
    nll = [-(torch.log_softmax(head(z, k, L), -1) * hot).sum(-1) for k in range(3)]           # 0 at an ignored pixel
    wc, wr = (hot * w_con.to(z.dtype)).sum(-1), (hot * w_rad.to(z.dtype)).sum(-1)
    return torch.cat([tri.reshape(-1), torch.stack([nll[0].sum(), (wc * nll[1]).sum(), (wr * nll[2]).sum()])])


def _dice_coeff(tri, eps):
    return (2 * tri[..., 0] + SMOOTH) / (tri[..., 1] + tri[..., 2] + SMOOTH + eps)            # 2tp + fp + fn = sum_p + count


def sup_from_stats(stats, w_con, w_rad, npix, w_ce, w_dc, eps=EPS):
    """[S, w_dc dice + w_ce ce of head 0, con, rad] from (global) statistics; npix = the (global) N * HW"""
    L = (stats.numel() - 3) // 3 - 1
    tri, sc = stats[:3 * (L + 1)].view(L + 1, 3), stats[3 * (L + 1):]
    dice = 1 - _dice_coeff(tri[1:], eps).mean()
    h0 = w_dc * dice + w_ce * (sc[0] / npix)
    con = sc[1] / (w_con.to(stats.dtype) * tri[:, 2]).sum()
    rad = sc[2] / (w_rad.to(stats.dtype) * tri[:, 2]).sum()
    return torch.stack([(h0 + con + rad) / 4, h0, con, rad])


def sup_loss(z, y, w_con, w_rad, w_ce, w_dc, eps=EPS):
    return sup_from_stats(sup_stats(z, y, w_con, w_rad), w_con, w_rad, float(z.shape[0] * z.shape[1]), w_ce, w_dc, eps)


def semi_stats(z, e, q, m):
    """[N, 3(L+1)+4] as smsut_cora_semi_stats leaves them"""
    L = (z.shape[-1] - 1) // 3
    m = m.to(z.dtype)
    hot = one_hot(q, L, z.dtype)
    tri = _dice_triplets(torch.softmax(head(z, 0, L), -1), hot, (1,))
    nll0 = -(torch.log_softmax(head(z, 0, L), -1) * hot).sum(-1)
    d2 = sum(((torch.softmax(head(z, k, L), -1) - torch.softmax(head(e, k, L), -1)) ** 2).sum(-1) for k in range(3))
    tail = torch.stack([(m * nll0).sum(1), m.sum(1), ((1 - m) * d2).sum(1), (1 - m).sum(1)], -1)
    return torch.cat([tri.reshape(z.shape[0], -1), tail], 1)


def semi_from_stats(stats, cw, eps=EPS):
    """[certain, uncertain]"""
    n, L = stats.shape[0], (stats.shape[1] - 4) // 3 - 1
    tri, t = stats[:, :3 * (L + 1)].view(n, L + 1, 3), stats[:, 3 * (L + 1):].sum(0)
    dice = 1 - _dice_coeff(tri[:, 1:], eps).mean()
    return torch.stack([(t[0] / (t[1] + 1e-16) + dice) / 2, cw / 3 * (t[2] / (t[3] + 1e-16))])


def semi_loss(z, e, q, m, cw, eps=EPS):
    return semi_from_stats(semi_stats(z, e.detach(), q, m), cw, eps)


def _both(fn):
    """fn(dtype) -> tensors; returns (result in fp64, result in fp32), everything detached"""
    return fn(torch.float64), fn(torch.float32)


def sup_refs(c, w_ce, w_dc):
    """(stats, out, dS/dz) in fp64 and in fp32"""
    def run(dt):
        z = c.z.detach().clone().to(dt).requires_grad_(True)
        st = sup_stats(z, c.y, c.w_con, c.w_rad)
        out = sup_from_stats(st, c.w_con, c.w_rad, float(z.shape[0] * z.shape[1]), w_ce, w_dc)
        out[0].backward()
        return st.detach(), out.detach(), z.grad
    return _both(run)


def semi_refs(c, gout, cw):
    """(stats, out, gout . d out / dz) in fp64 and in fp32"""
    def run(dt):
        z = c.z.detach().clone().to(dt).requires_grad_(True)
        st = semi_stats(z, c.e.to(dt), c.q, c.m)
        out = semi_from_stats(st, cw)
        (gout[0] * out[0] + gout[1] * out[1]).backward()
        return st.detach(), out.detach(), z.grad
    return _both(run)


def dtc_refs(c, k, gout):
    """(out, gt, gz) in fp64 and in fp32: dtc_ref.dtc_loss on the NCHW view"""
    def run(dt):
        t, z = c.t.detach().clone().to(dt).requires_grad_(True), c.z.detach().clone().to(dt).requires_grad_(True)
        out = DR.dtc_loss(as_nchw(t), as_nchw(z), as_nchw(c.sdf.to(dt)), k)
        (gout[0] * out[0] + gout[1] * out[1]).backward()
        return out.detach(), t.grad, z.grad
    return _both(run)


# ------------------------------------------------------------------------------------------- CoraNet cases
def class_weights(L):
    """unequal per class (a per-class mix-up shows), all positive"""
    i = torch.arange(L + 1, dtype=torch.float32)
    return 1.0 + 0.37 * i, 5.0 - 0.41 * i


@functools.lru_cache(maxsize=4)
def cora_case(n, L, hw, seed=0, scale=2.0, mask="binary"):
    """logits ``scale * randn`` of student and teacher, labels, pseudo labels (every class drawn), mask (0/1 at 60 %, or uniform)"""
    rs = np.random.RandomState(1000 * L + 10 * n + seed + hw % 997)
    c = 3 * L + 1
    z = torch.from_numpy(scale * rs.standard_normal((n, hw, c))).float()
    e = torch.from_numpy(scale * rs.standard_normal((n, hw, c))).float()
    y = torch.from_numpy(rs.randint(0, L + 1, (n, hw)).astype(np.int64))
    q = torch.from_numpy(rs.randint(0, L + 1, (n, hw)).astype(np.int64))
    u = rs.uniform(size=(n, hw))
    m = torch.from_numpy(u if mask == "uniform" else (u < 0.6)).float()
    w_con, w_rad = class_weights(L)
    return types.SimpleNamespace(n=n, L=L, hw=hw, z=z, e=e, y=y, q=q, m=m, w_con=w_con, w_rad=w_rad)


def clone_case(c):
    return types.SimpleNamespace(**{k: (v.clone() if torch.is_tensor(v) else v) for k, v in vars(c).items()})


def planted_pixels(hw, k):
    """up to k distinct pixels, the last one first"""
    out = []
    for p in (hw - 1, 0, hw // 2, hw // 3, (2 * hw) // 3, hw // 5):
        if 0 <= p < hw and p not in out:
            out.append(p)
    return out[:k]


def saturated_case(n, L, hw, seed=0):
    """25 * randn, and planted in every sample: background +80 with every foreground -80 | the label's logit -80 under a +80 maximum in
    each head | all logits of the pixel equal | student == teacher bit for bit (its MSE term and gradient are exactly 0 in both references).  y == q at the
    planted pixels, so that both losses see them."""
    c = clone_case(cora_case(n, L, hw, seed, scale=25.0))
    pix = planted_pixels(hw, 4)
    t = c.z
    if len(pix) > 0:
        t[:, pix[0], :] = -80.0
        t[:, pix[0], 0] = 80.0
    if len(pix) > 1:
        p = pix[1]
        for s in range(n):
            lab = int(c.y[s, p])
            c.q[s, p] = lab
            if lab == 0:
                t[s, p, 0] = -80.0
                for k in range(3):
                    t[s, p, 1 + k * L] = 80.0
            else:
                t[s, p, 0] = 80.0
                for k in range(3):
                    t[s, p, k * L + lab] = -80.0
    if len(pix) > 2:
        t[:, pix[2], :] = 3.0
    if len(pix) > 3:
        c.e[:, pix[3], :] = c.z[:, pix[3], :]
        c.m[:, pix[3]] = 0.0                                      # (unmasked for the MSE term)
    c.planted = pix
    return c


def all_background_case(L, hw=64):
    """Every pixel: background +80, foreground -80, label 0.  Every foreground class has tp = count = 0 and sum_p = exp(-160) = 0: its
    Dice coefficient is smooth / (smooth + eps), the one place where the 1e-8 of the denominator is visible in fp32."""
    c = clone_case(cora_case(1, L, hw, 5))
    c.z[:] = -80.0
    c.z[..., 0] = 80.0
    c.y[:] = 0
    c.q[:] = 0
    return c


def invalid_label_case(n, L, hw, seed=0):
    """-1, L+1 and 1000 planted in labels and pseudo labels of every sample, the last pixel among them"""
    c = clone_case(cora_case(n, L, hw, seed))
    pix = planted_pixels(hw, 3)
    assert len(pix) == 3
    for lab in (c.y, c.q):
        lab[:, pix[0]], lab[:, pix[1]], lab[:, pix[2]] = -1, L + 1, 1000
    c.planted = pix
    return c


def per_sample_case(L, hw=1300):
    """N = 3: sample 0 lacks class L in q, sample 1 has m == 1, sample 2 has m == 0"""
    c = clone_case(cora_case(3, L, hw, 7))
    c.q[0][c.q[0] == L] = 0
    c.m[1] = 1.0
    c.m[2] = 0.0
    return c


# ------------------------------------------------------------------------------------------- pseudo labels
PSEUDO_P = [1, 65, 257, 2048 * 256 + 77]           # the last: past one trip of the capped elementwise grid (2048 blocks of 256)
PSEUDO_L = [1, 3, 4, 10]


def pseudo_case(p, L, seed=0):
    """logits [P, 3L+1] drawn from a few integers (many equal maxima), then planted (where P allows): background ties with the last
    class of every head | two foreground classes tie | NaN in one class of head 1 | NaN in the background | -inf everywhere but one
    class | all equal"""
    rs = np.random.RandomState(31 + L + p % 1009)
    c = 3 * L + 1
    z = torch.from_numpy(rs.randint(-3, 4, size=(p, c))).float() + torch.from_numpy(rs.standard_normal((p, 1))).float()
    z[::3] = torch.from_numpy(2 * rs.standard_normal(z[::3].shape)).float()          # a third of the rows without ties
    if p >= 65:
        rows = [p - 1, 0, 7, 13, 21, 34, 55]
        z[rows[0]] = 0.0
        z[rows[0], 0] = 1.0
        for k in range(3):
            z[rows[0], k * L + L] = 1.0
        z[rows[1]] = 0.0
        z[rows[1], 1] = 2.0
        z[rows[1], min(2, L)] = 2.0
        z[rows[1], 1 + L] = 1.0
        z[rows[2], 1 + L + (L - 1)] = float("nan")
        z[rows[3], 0] = float("nan")
        z[rows[4]] = float("-inf")
        z[rows[4], 1 + 2 * L] = -5.0
        z[rows[5]] = 1.25
        z[rows[6]] = float("-inf")
    return z


def pseudo_ref(z):
    """coranet_ref.pseudo on the NCHW view -> (q [P] int64, m [P] fp32)"""
    q, m = CR.pseudo(z.t().reshape(1, z.shape[1], z.shape[0], 1))
    return q.reshape(-1), m.reshape(-1)


# ------------------------------------------------------------------------------------------- EMA
EMA_LENGTHS = [1, 8191, 8192, 8193, 3 * 8192 + 5] + [3] * 300      # one block per 8192-element chunk of one tensor; many entries


def ema_refs(ema, params, alpha):
    """(ref64, bar) per tensor: alpha and 1 - alpha as the fp32 values the kernel is handed; two roundings, or one fused rounding, of
    alpha e + beta p stay within 2^-23 (|alpha e| + |beta p|)"""
    a, b = float(np.float32(alpha)), float(np.float32(1 - alpha))
    out = []
    for e, p in zip(ema, params):
        e64, p64 = e.double().numpy(), p.double().numpy()
        out.append((a * e64 + b * p64, 2.0 ** -23 * (np.abs(a * e64) + np.abs(b * p64))))
    return out


# ------------------------------------------------------------------------------------------- DTC cases
@functools.lru_cache(maxsize=4)
def dtc_case(n, b, c, hw, seed=0):
    """dtc_ref.loss_case as rows: half the t near zero (the live sigmoid at k = 1500), logits 2 * randn, sdf in [-1, 1]"""
    t, z, s = DR.loss_case(n, b, c, hw, 1, 100 * c + 10 * n + b + seed + hw % 991)
    rows = lambda x: x.squeeze(-1).permute(0, 2, 1).contiguous()
    if t.numel() < 256:                  # a handful of elements: the draw alone may leave none near zero; every other one is put there
        t.view(-1)[::2] = torch.from_numpy(np.random.RandomState(seed + hw).uniform(-5e-3, 5e-3, (t.numel() + 1) // 2)).float()
    return types.SimpleNamespace(n=n, b=b, c=c, hw=hw, t=rows(t), z=rows(z), sdf=rows(s))


def live_share(gt64):
    """share of elements with a non-zero fp64 d L_cons / dt (the condition of tests/test_dtc_gpu.py for the (0, 1) combination)"""
    return float((gt64 != 0).double().mean())


PLANTED_T = [0.0, -0.0, 1.0, -1.0, 1e-30, -1e-30, 0.0592, -0.0592]     # |k t| = 88.8 at k = 1500: exp reaches the fp32 denormals


def dtc_planted_t_case(c, hw=1300):
    cs = clone_case(dtc_case(3, 2, c, hw, 3))
    vals = torch.tensor(PLANTED_T)
    flat = cs.t.view(-1)
    idx = torch.arange(flat.numel())
    plant = idx % 3 != 2                                              # two elements in three planted, the rest stay as drawn
    flat[plant] = vals[(idx % c + idx // c) % len(PLANTED_T)][plant]  # (channel + pixel: every value reaches every channel)
    flat[-1] = -0.0592
    return cs


def dtc_saturated_case(c, hw=1300):
    """logits 25 * randn and planted: channel 0 at +80 over -80 | the last channel +80 over a -80 channel 0 | all equal"""
    cs = clone_case(dtc_case(3, 2, c, hw, 4))
    cs.z *= 12.5
    pix = planted_pixels(hw, 3)
    cs.z[:, pix[0], :] = -80.0
    cs.z[:, pix[0], 0] = 80.0
    cs.z[:, pix[1], 0] = -80.0
    cs.z[:, pix[1], c - 1] = 80.0
    cs.z[:, pix[2], :] = 3.0
    return cs
