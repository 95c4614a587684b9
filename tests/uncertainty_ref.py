"""References of ``ops.tta_uncertainty`` (csrc/uncertainty.hip): the fp64 definition, an fp32 numpy emulation of the kernel's stated
arithmetic, the members' own labels, the agreement counts from given maps, the bounds, and the case draw.  Host code only.

The arithmetic the kernel states, per output pixel q, all fp32, member by member in list order: z = member[F_g(q)][0..K-1];
a_t = the first maximum of z (the first maximum wins, a NaN wins); m = max_k z_k; e_k = expf(z_k - m); s = e_0 + e_1 + ... in
channel order; q_k = e_k / s; acc_k += q_k; h_t = -(q_0 logf(q_0 + 1e-6f) + ...) in channel order; hs += h_t.  Then
mean_k = acc_k / (float)T; pred = the first maximum of mean; conf = mean_pred; H = -(mean_0 logf(mean_0 + 1e-6f) + ...);
EH = hs / (float)T; MI = fmaxf(H - EH, 0.f); votes = #{t : a_t == pred}.

counts int64 [K][2 T + 4], row k = {V, ALL, ANY, HSUM, V_0 .. V_{T-1}, I_0 .. I_{T-1}}: V pixels with pred == k; ALL every
a_t == k; ANY some a_t == k; V_t a_t == k; I_t a_t == k and pred == k; HSUM the sum over pixels with pred == k and a finite H of
(int64)rintf(H * 2^20).

Bounds (absolute, against fp64), eps = 2^-24:
  B_H  = uamt_ref.entropy_bound(K, T)                       (derived in tests/uamt_ref.py for exactly this arithmetic)
  B_EH = entropy_bound(K, 1) + eps (T + 1) ln K             (each h_t is a one-member entropy; then T - 1 additions and one division
                                                             of values <= ln K)
  B_MI = B_H + B_EH + eps ln max(K, 2)                      (the subtraction; the clamp at 0 only moves the value towards the true
                                                             one, which is >= 0 because -p log(p + 1e-6) is concave)"""
import math

import numpy as np
import torch

import tta_ref
import uamt_ref

SCALE = 1 << 20
V, ALL, ANY, HSUM, FIXED = 0, 1, 2, 3, 4
D4, FLIPS = tuple(range(8)), (0, 4, 6, 2)
# (T, N, H, W, C, K, transforms, members are views one float into their allocation)
CASES = [
    (8, 2, 20, 20, 5, 5, D4, False),                           # partial tile of both tile sizes
    (4, 1, 37, 50, 5, 5, FLIPS, True),                         # 2 x 2 tiles of 32, non-square, unaligned rows
    (8, 1, 40, 40, 5, 5, D4, True),                            # quarter turns across tiles
    (2, 2, 16, 24, 7, 3, (0, 0), False),                       # K < C
    (4, 1, 33, 35, 4, 4, FLIPS, False),                        # even C
    (8, 1, 20, 20, 12, 12, D4, False),                         # runtime class loop, staged
    (3, 1, 9, 11, 33, 32, (0, 4, 2), False),                   # rows read in place, K = 32
    (16, 1, 20, 20, 5, 5, D4 + D4, False),                     # T at its limit
    (1, 1, 1, 1, 2, 2, (0,), False),                           # one pixel, one member
    (3, 2, 9, 7, 1, 1, (0, 4, 2), False),                      # one class
]
IDS = ["d4-20x20", "flips-37x50-offset", "d4-40x40-offset", "K3-of-7", "flips-evenC", "d4-K12", "C33-K32", "T16", "one-pixel-T1",
       "one-class"]
SEED = 0


def bound_h(k, t):
    return uamt_ref.entropy_bound(k, t)


def bound_eh(k, t):
    return uamt_ref.entropy_bound(k, 1) + uamt_ref.EPS32 * (t + 1) * math.log(k)


def bound_mi(k, t):
    return bound_h(k, t) + bound_eh(k, t) + uamt_ref.EPS32 * math.log(max(k, 2))


def draw(t, n, h, w, c, transforms, rs):
    """T members, NHWC fp32 arrays on their own (transformed) grids, drawn as ``uamt_ref.case`` draws: a shared per-pixel logit
    vector of random sharpness plus unit member noise -- H spreads over [0, ln K] and the members partly agree -- and member t is
    ``F_g`` of its logits."""
    u = 3.0 * rs.standard_normal((1, n, h, w, c)) * rs.uniform(0.0, 1.5, (1, n, h, w, 1)) + rs.standard_normal((t, n, h, w, c))
    u = torch.from_numpy(u.astype(np.float32))
    return [on_member_grid(u[i], g) for i, g in enumerate(transforms)]


def on_member_grid(x, g):
    """[N, H, W, C] on the un-transformed grid (tensor) -> the NHWC array of ``F_g`` of it"""
    return np.ascontiguousarray(tta_ref.fwd(x.permute(0, 3, 1, 2), g).permute(0, 2, 3, 1).numpy())


def draw_cases():
    """The members of every case of ``CASES``, from ONE RandomState(SEED) drawn through the cases in order"""
    rs = np.random.RandomState(SEED)
    return [draw(t, n, h, w, c, tr, rs) for (t, n, h, w, c, k, tr, off) in CASES]


def put_back(z, g):
    """NHWC [N, h, w, C] on the member's grid (tensor) -> [N, H, W, C] on the un-transformed grid"""
    return tta_ref.inv(z.permute(0, 3, 1, 2), g).permute(0, 2, 3, 1)


def reference(members, transforms, classes):
    """fp64 ``(pred int64, conf, H, EH, MI, gap)`` [N, H, W] of T NHWC members on their own grids: per-member softmax put back with
    ``tta_ref.inv``, the mean, its first maximum, the entropies, and the distance between the two largest mean probabilities (inf
    with one class)."""
    pred, conf, mean, gap = tta_ref.merge_ref(members, transforms, classes=classes)
    eh = None
    for z, g in zip(members, transforms):
        p = torch.softmax(torch.as_tensor(np.asarray(z)).double()[..., :classes], dim=-1)
        ht = put_back(-(p * torch.log(p + 1e-6)).sum(-1, keepdim=True), g)[..., 0]
        eh = ht if eh is None else eh + ht
    eh = eh / len(transforms)
    h = -(mean * torch.log(mean + 1e-6)).sum(-1)
    return pred, conf, h, eh, h - eh, gap


def _entropy32(q):
    """-(q_0 log(q_0 + 1e-6f) + ...) along the last axis, fp32, in channel order"""
    term = q * np.log(q + np.float32(1e-6))
    h = term[..., 0].copy()
    for k in range(1, q.shape[-1]):
        h = h + term[..., k]
    assert h.dtype == np.float32
    return -h


def first_max(z):
    """The first maximum along the last axis by the kernels' comparison: the first maximum wins, a NaN wins (the first NaN)"""
    z = np.asarray(z)
    nan = np.isnan(z)
    return np.where(nan.any(-1), np.argmax(nan, -1), np.argmax(np.where(nan, -np.inf, z), -1))


def emulate_fp32(members, transforms, classes):
    """The stated arithmetic in numpy fp32, operation by operation (numpy's exp / log in place of the device's):
    ``(pred, conf, H, EH, MI)`` [N, H, W]"""
    t = len(transforms)
    acc = hs = None
    for z, g in zip(members, transforms):
        z = put_back(torch.as_tensor(np.asarray(z, dtype=np.float32)), g).numpy()[..., :classes]
        e = np.exp(z - z.max(-1, keepdims=True))
        s = e[..., 0].copy()
        for k in range(1, classes):
            s = s + e[..., k]
        q = e / s[..., None]
        acc = q if acc is None else acc + q
        hs = _entropy32(q) if hs is None else hs + _entropy32(q)
    mean = acc / np.float32(t)
    pred = first_max(mean)
    h, eh = _entropy32(mean), hs / np.float32(t)
    mi = np.maximum(h - eh, np.float32(0))
    assert mean.dtype == h.dtype == eh.dtype == mi.dtype == np.float32
    return pred, np.take_along_axis(mean, pred[..., None], -1)[..., 0], h, eh, mi


def member_labels(members, transforms, classes):
    """int64 [T, N, H, W]: every member's own label -- the first maximum of its K leading logits -- on the un-transformed grid"""
    return np.stack([tta_ref.inv(torch.from_numpy(first_max(np.asarray(z)[..., :classes])), g).numpy()
                     for z, g in zip(members, transforms)])


def votes_of(labels, pred):
    return (np.asarray(labels) == np.asarray(pred)[None]).sum(0)


def counts_of(pred, labels, h32, classes):
    """int64 [K, 2 T + 4] from a prediction [N, H, W], member labels [T, N, H, W] and an fp32 entropy map [N, H, W]"""
    pred, labels, h32 = np.asarray(pred), np.asarray(labels), np.asarray(h32)
    assert h32.dtype == np.float32
    t = labels.shape[0]
    finite = np.isfinite(h32)
    units = np.rint(np.where(finite, h32, np.float32(0)) * np.float32(SCALE)).astype(np.int64)   # (exact: a scaling by 2^20)
    out = np.zeros((classes, 2 * t + FIXED), dtype=np.int64)
    for k in range(classes):
        ip, at = pred == k, labels == k
        out[k, V], out[k, ALL], out[k, ANY] = ip.sum(), at.all(0).sum(), at.any(0).sum()
        out[k, HSUM] = units[ip & finite].sum()
        out[k, FIXED:FIXED + t] = at.reshape(t, -1).sum(1)
        out[k, FIXED + t:] = (at & ip[None]).reshape(t, -1).sum(1)
    return out
