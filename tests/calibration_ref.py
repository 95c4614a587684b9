"""fp64 reference, fp32 emulation, error budgets and case draw of the calibration statistics (csrc/calibration.hip; the arithmetic
is stated in include/smsut_hip.h).  Host code only.

Totals vector (``ops.CalibrationLayout``, restated here on its own): ``[3 b + 0..2]`` bin b {pixels, sum of conf, correct};
``[3 B + 4 k + 0..3]`` true class k {pixels, correct, sum of nll, sum of brier}; ``[3 B + 4 K + 0..3]`` {g, h, skipped, nonfinite}.

Error budgets, with eps = 2^-24 (the fp32 rounding unit; expf and logf are charged 2 ulp = 4 eps relative), K classes, and per case
D = the largest |u_k - m|, U = the largest |u_k|, Z = the largest |z_k|.  They are derived, not fitted:

B_p, a probability (hence conf): ``tta_ref.budget(K, 1)`` = eps (2 K + 9) -- one rounding in u - m, expf, K - 1 additions in s, the
  division; |d| e^d <= 1 / e bounds how the error of the exponent's argument propagates -- plus ONE rounding, eps, for the product
  beta z_k when beta != 1.  (To first order that product moves u_k by at most eps |u_k| and p_k by at most
  p_k (1 - p_k) 2 eps U <= eps U / 2: one rounding for U <= 2.)
B_nll: s carries 5 eps per term (argument 1 / e, expf 4) and eps s per addition, so log s is off by at most
  (5 K + (K - 1)) eps <= 6 K eps as s >= 1; logf adds 4 eps ln K; u_y - m one rounding, eps D; the final subtraction eps (ln K + D);
  with beta != 1 the products move nll by sum_k |p_k - [k == y]| eps |u_k| <= 2 eps U.
    B_nll = eps (6 K + 5 ln K + 2 D + 2 U [beta != 1])
B_brier: each p_k - [k == y] is off by B_p + eps and at most 1 in size, its square by 2 (B_p + eps) + eps; K - 1 additions of a
  sum <= 2.   B_brier = 2 K B_p + (5 K - 2) eps
B_g, ez - z_y: sum_k |dp_k| |z_k| <= K B_p Z; the products and additions of ez, a sum with sum_k p_k |z_k| <= Z, (1 + K - 1) eps Z;
  the subtraction 2 eps Z.   B_g = Z (K B_p + (K + 2) eps)
B_h, vz: ezz as ez with one more rounding for z_k^2: Z^2 (K B_p + (K + 1) eps); ez^2: 2 Z d(ez) + eps Z^2 with
  d(ez) = Z (K B_p + K eps); the subtraction eps Z^2; the clamp at 0 moves the value towards the true one, which is >= 0.
    B_h = Z^2 (3 K B_p + (3 K + 3) eps)
A fused multiply-add in brier, ez, ezz or vz drops a rounding and stays inside these.  A sum over n pixels is held to n times its
per-pixel bound: the kernel converts each pixel's value to fp64 and adds in fp64, whose own error, n 2^-53 relative, is some 2^-29
of a per-pixel bound and is neglected.  Counts are exact.
"""
import math

import numpy as np

import tta_ref

EPS = 2.0 ** -24
T_SCALED = 1.7                                  # the second temperature every case runs at
CASES = [(3, 7, 9, 5, 5, 15), (2, 67, 129, 5, 5, 10), (1, 9, 11, 33, 32, 32), (2, 16, 24, 13, 5, 15), (1, 5, 5, 2, 2, 1),
         (1, 1, 1, 3, 1, 4)]                    # (N, H, W, C, K, B)
# More than 65536 pixels and no multiple of 256 * 256: the kernel's grid stops at 256 workgroups of 256-pixel tiles, so every
# workgroup walks its tile loop more than once and the last round is ragged (compile-time K = 5; runtime K = 7); and K = 4, the
# one compile-time class count the cases above leave out.
LOOP_CASES = [(3, 160, 161, 5, 5, 15), (2, 200, 181, 7, 7, 12)]
MORE_CASES = LOOP_CASES + [(2, 19, 23, 4, 4, 15)]


def beta_of(temperature):
    """The fp32 inverse temperature the kernel multiplies by, as a Python float."""
    return float(np.float32(1.0 / float(temperature)))


def size(k, b):
    return 3 * b + 4 * k + 4


def b_p(k, beta):
    return tta_ref.budget(k, 1) + (EPS if beta != 1.0 else 0.0)


def per_pixel_bounds(k, beta, d, u, z):
    """(B_p, B_nll, B_brier, B_g, B_h) of the module docstring."""
    bp = b_p(k, beta)
    return (bp,
            EPS * (6 * k + 5 * math.log(k) + 2 * d + (2 * u if beta != 1.0 else 0.0)),
            2 * k * bp + (5 * k - 2) * EPS,
            z * (k * bp + (k + 2) * EPS),
            z * z * (3 * k * bp + (3 * k + 3) * EPS))


def first_max(p):
    return np.argmax(p == p.max(axis=-1, keepdims=True), axis=-1)


def _pixels(z, y, k, beta, dtype):
    """Per-pixel values of the stated arithmetic in ``dtype`` (fp64: the reference, u = beta z exact; fp32: the emulation, every
    step rounded).  z [P, C] float32, y [P] int64.  Rows whose label lies outside 0 .. K-1 are computed with y = 0 and masked by
    the caller."""
    f = dtype
    zk = z[:, :k].astype(f)
    u = zk if beta == 1.0 else (f(beta) * zk).astype(f)
    m = u.max(axis=1, keepdims=True)
    d = (u - m).astype(f)
    e = np.exp(d).astype(f)
    s = e[:, 0].copy()
    for c in range(1, k):
        s = (s + e[:, c]).astype(f)
    p = (e / s[:, None]).astype(f)
    pred = first_max(p)
    rows = np.arange(z.shape[0])
    conf = p[rows, pred]
    yy = np.where((y >= 0) & (y < k), y, 0)
    nll = (np.log(s).astype(f) - d[rows, yy]).astype(f)
    brier, ez, ezz = np.zeros(z.shape[0], f), np.zeros(z.shape[0], f), np.zeros(z.shape[0], f)
    for c in range(k):
        t = (p[:, c] - (yy == c).astype(f)).astype(f)
        brier = (brier + (t * t).astype(f)).astype(f)
        ez = (ez + (p[:, c] * zk[:, c]).astype(f)).astype(f)
        ezz = (ezz + (p[:, c] * (zk[:, c] * zk[:, c]).astype(f)).astype(f)).astype(f)
    vz = np.maximum((ezz - (ez * ez).astype(f)).astype(f), f(0))
    gz = (ez - zk[rows, yy]).astype(f)
    if k > 1:
        top2 = np.sort(p, axis=1)[:, -2:]
        gap = (top2[:, 1] - top2[:, 0]).astype(np.float64)
    else:
        gap = np.full(z.shape[0], np.inf)
    return dict(conf=conf, pred=pred, nll=nll, brier=brier, gz=gz, vz=vz, gap=gap, absd=np.abs(d).max(axis=1),
                absu=np.abs(u).max(axis=1), absz=np.abs(zk).max(axis=1))


def stats(z, y, k, b, beta=1.0, dtype=np.float64):
    """The totals vector (fp64) of logits z [N, H, W, C] (float32) and labels y [N, H, W] (int64) by the stated arithmetic carried
    out in ``dtype``, and the per-pixel dict it was summed from (with ``counted``, ``bin``)."""
    z = np.asarray(z, dtype=np.float32)
    z2, y1 = z.reshape(-1, z.shape[-1]), np.asarray(y).reshape(-1).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        px = _pixels(z2, y1, k, beta, dtype)
        labelled = (y1 >= 0) & (y1 < k)
        finite = np.isfinite(px["conf"])
        counted = labelled & finite
        px["bin"] = np.minimum(b - 1, (np.where(counted, px["conf"], 0) * dtype(b)).astype(dtype).astype(np.int64))
    px["counted"] = counted
    out = np.zeros(size(k, b))
    ok = counted & (px["pred"] == y1)
    for j in range(b):
        sel = counted & (px["bin"] == j)
        out[3 * j:3 * j + 3] = sel.sum(), px["conf"][sel].astype(np.float64).sum(), (sel & ok).sum()
    for c in range(k):
        sel = counted & (y1 == c)
        out[3 * b + 4 * c:3 * b + 4 * c + 4] = (sel.sum(), (sel & ok).sum(), px["nll"][sel].astype(np.float64).sum(),
                                                px["brier"][sel].astype(np.float64).sum())
    out[3 * b + 4 * k:] = (px["gz"][counted].astype(np.float64).sum(), px["vz"][counted].astype(np.float64).sum(),
                           (~labelled).sum(), (labelled & ~finite).sum())
    return out, px


def bounds(px, y, k, b, beta):
    """The tolerance of every element of the totals vector (0: exact), from the reference's per-pixel dict: the number of pixels
    summed into the element times the per-pixel bound at the case's D, U, Z."""
    y1 = np.asarray(y).reshape(-1)
    c = px["counted"]
    d, u, z = (float(px[q][c].max()) if c.any() else 0.0 for q in ("absd", "absu", "absz"))
    bp, bn, bb, bg, bh = per_pixel_bounds(k, beta, d, u, z)
    tol = np.zeros(size(k, b))
    for j in range(b):
        tol[3 * j + 1] = (c & (px["bin"] == j)).sum() * bp
    for q in range(k):
        n = (c & (y1 == q)).sum()
        tol[3 * b + 4 * q + 2], tol[3 * b + 4 * q + 3] = n * bn, n * bb
    tol[3 * b + 4 * k], tol[3 * b + 4 * k + 1] = c.sum() * bg, c.sum() * bh
    return tol


def unsafe(z, k, b, betas):
    """Rows of z [P, C] whose fp64 confidence lies within 4 B_p of a bin edge j / B, 0 < j < B, or whose two largest probabilities
    are closer than 4 B_p, at any of ``betas``: there a rounding may move the bin or the prediction."""
    bad = np.zeros(z.shape[0], dtype=bool)
    y0 = np.zeros(z.shape[0], dtype=np.int64)
    for beta in betas:
        px = _pixels(z, y0, k, beta, np.float64)
        margin = 4 * b_p(k, beta)
        t = px["conf"].astype(np.float64) * b
        near = np.abs(t - np.round(t)) / b <= margin
        inner = (np.round(t) > 0) & (np.round(t) < b)
        bad |= (near & inner) | (px["gap"] < margin)
    return bad


def draw(case, seed, betas=None):
    """``(z [N, H, W, C] float32, y [N, H, W] int64, rounds)``: logits 3 * standard_normal; every pixel that is ``unsafe`` at one of
    ``betas`` (default: 1 and 1 / 1.7) is drawn again until none is left (``rounds`` redraws); labels uniform in 0 .. K-1 with
    every 11th pixel from the 6th on planted outside (-1, K, 255 in turn)."""
    n, h, w, c, k, b = case
    betas = (1.0, beta_of(T_SCALED)) if betas is None else betas
    rng = np.random.default_rng(seed)
    p = n * h * w
    z = (3.0 * rng.standard_normal((p, c))).astype(np.float32)
    rounds = 0
    while True:
        bad = unsafe(z, k, b, betas)
        if not bad.any():
            break
        z[bad] = (3.0 * rng.standard_normal((int(bad.sum()), c))).astype(np.float32)
        rounds += 1
        assert rounds < 50
    y = rng.integers(0, k, p).astype(np.int64)
    idx = np.arange(5, p, 11)
    y[idx] = np.array([-1, k, 255])[np.arange(idx.size) % 3]
    return z.reshape(n, h, w, c), y.reshape(n, h, w), rounds


def planted(seed, n=4, h=24, w=24, k=5, scale=2.5):
    """The temperature-fit case: z0 = 2 * standard_normal logits, labels sampled from softmax(z0), logits handed over
    ``scale * z0`` -- an over-confident network whose NLL is minimal near T = scale.  Returns ``(z float32 [n, h, w, k], y)``."""
    rng = np.random.default_rng(seed)
    z0 = 2.0 * rng.standard_normal((n * h * w, k))
    p = np.exp(z0 - z0.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    y = (rng.random((n * h * w, 1)) > np.cumsum(p, axis=1)).sum(axis=1).clip(0, k - 1).astype(np.int64)
    return (scale * z0).astype(np.float32).reshape(n, h, w, k), y.reshape(n, h, w)


def newton_step_size(z, y, k, beta):
    """fp64 (|g| / h, g, h) of the summed NLL at ``beta``."""
    out, _ = stats(z, y, k, 1, beta)
    g, h = out[3 + 4 * k], out[3 + 4 * k + 1]
    return abs(g) / h, g, h
