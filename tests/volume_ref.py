"""fp64 NumPy oracle of the volume-preparation kernels (csrc/volume.hip), with an fp32 restatement of every floating-point
function: ``dtype=np.float64`` is the statement, ``dtype=np.float32`` the same expression on the same inputs in fp32 (``ref32``),
whose distance from the statement sets the tests' bars.  No scipy needed; tests/test_volume_ref_cpu.py checks it against scipy.

Arrays are [D, H, W] = [z, y, x].  Index map: x = ((i + start) * num) / den - offset in fp64; inside iff -0.5 <= x < n - 0.5."""
import numpy as np

CHAOS_RANGES = ((55, 70), (110, 135), (175, 200), (240, 255))          # grey range of class 1..4


def mirror(j, n):
    """Whole-sample mirror folding of integer indices onto 0 .. n-1: -1 -> 1, n -> n - 2 (n == 1: everything is 0)."""
    j = np.asarray(j, dtype=np.int64)
    if n == 1:
        return np.zeros_like(j)
    p = 2 * n - 2
    m = np.mod(j, p)
    return np.where(m < n, m, p - m)


def spline_matrix(n, dtype=np.float64):
    """A[i, mirror(i + k)] += (1/6, 4/6, 1/6), k = -1, 0, 1: coefficients c solve A c = v.  n == 1: the identity."""
    a = np.zeros((n, n), dtype=dtype)
    if n == 1:
        a[0, 0] = 1
        return a
    w = (dtype(1) / dtype(6), dtype(4) / dtype(6), dtype(1) / dtype(6))
    for i in range(n):
        for k, wk in zip((-1, 0, 1), w):
            a[i, int(mirror(i + k, n))] += wk
    return a


def coefficients(v, dtype=np.float64):
    """Cubic B-spline interpolation coefficients of v with mirror boundaries: the dense solve, axis after axis (x, y, z)."""
    c = np.asarray(v).astype(dtype)
    for ax in (2, 1, 0):
        n = c.shape[ax]
        if n == 1:
            continue
        m = np.moveaxis(c, ax, 0)
        s = np.linalg.solve(spline_matrix(n, dtype), m.reshape(n, -1)).astype(dtype)
        c = np.moveaxis(s.reshape(m.shape), 0, ax)
    return np.ascontiguousarray(c)


def coords(n_out, start, num, den, offset=0):
    """The continuous source index of every output index of one axis, fp64: an exact integer product, one division."""
    i = np.arange(n_out, dtype=np.int64)
    return ((i + int(start)) * int(num)).astype(np.float64) / np.float64(den) - np.float64(offset)


def inside(x, n):
    return (x >= -0.5) & (x < n - 0.5)


def axis_weights(n_out, n_src, start, num, den, offset=0, dtype=np.float64):
    """[n_out, n_src] matrix of one axis: the four cubic B-spline weights of t = x - floor(x) on the mirror-folded indices
    floor(x) - 1 .. floor(x) + 2; rows of outside points are zero.  Returns (matrix, inside mask)."""
    x = coords(n_out, start, num, den, offset)
    ok = inside(x, n_src)
    f = np.floor(x)
    t = (x - f).astype(dtype)
    u = dtype(1) - t
    six = dtype(6)
    w = [u * u * u / six, (dtype(4) - six * t * t + dtype(3) * t * t * t) / six,
         (dtype(4) - six * u * u + dtype(3) * u * u * u) / six, t * t * t / six]
    m = np.zeros((n_out, n_src), dtype=dtype)
    for j in range(4):
        idx = mirror(f.astype(np.int64) - 1 + j, n_src)
        for i in range(n_out):
            if ok[i]:
                m[i, idx[i]] += w[j][i]
    return m, ok


def resample(coef, out_size, num, den, start, offset=(0, 0, 0), dtype=np.float64):
    """The spline with coefficients coef at the mapped points of the window out_size; 0 outside."""
    c = np.asarray(coef).astype(dtype)
    ms, oks = zip(*(axis_weights(out_size[a], c.shape[a], start[a], num[a], den[a], offset[a], dtype) for a in range(3)))
    r = np.einsum("xc,dhc->dhx", ms[2], c).astype(dtype)
    r = np.einsum("yh,dhx->dyx", ms[1], r).astype(dtype)
    r = np.einsum("zd,dyx->zyx", ms[0], r).astype(dtype)
    ok = oks[0][:, None, None] & oks[1][None, :, None] & oks[2][None, None, :]
    return np.where(ok, r, dtype(0)), ok


def nearest(lab, out_size, num, den, start, offset=(0, 0, 0), lut=None):
    """Nearest neighbour: source index floor(x + 0.5), 0 outside; lut (256 entries) applied to the source value."""
    lab = np.asarray(lab)
    src = lab if lut is None else np.asarray(lut, dtype=np.uint8)[lab]
    idx, oks = [], []
    for a in range(3):
        x = coords(out_size[a], start[a], num[a], den[a], offset[a])
        ok = inside(x, lab.shape[a])
        idx.append(np.where(ok, np.floor(x + 0.5).astype(np.int64), 0))
        oks.append(ok)
    out = src[idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]
    ok = oks[0][:, None, None] & oks[1][None, :, None] & oks[2][None, None, :]
    return np.where(ok, out, 0).astype(np.uint8)


def window(v, lo, hi, dtype=np.float32):
    """(uint8)((min(max(x, lo), hi) - lo) / (hi - lo) * 255) in dtype, truncated; zeros when hi == lo."""
    v, lo, hi = np.asarray(v).astype(dtype), dtype(lo), dtype(hi)
    if hi == lo:
        return np.zeros(v.shape, dtype=np.uint8)
    q = (np.minimum(np.maximum(v, lo), hi) - lo) / (hi - lo) * dtype(255)
    assert q.dtype == dtype
    return q.astype(np.int32).astype(np.uint8)


def chaos_lut():
    lut = np.zeros(256, dtype=np.uint8)
    for cls, (lo, hi) in enumerate(CHAOS_RANGES, start=1):
        lut[lo:hi + 1] = cls
    return lut


def bar(ref32, ref64):
    """16 times the reference's own fp32 rounding over the tensor."""
    return 16.0 * float(np.abs(np.asarray(ref32, dtype=np.float64) - ref64).max())


def volume(shape, seed, bits=12):
    """Seeded data on a scanner's 12-bit range: a smooth field plus noise, fp32.  NOT rounded to integers: on integer data and a
    very short axis the fp32 solve is exact (its results are small dyadic fractions), which would make a bar of zero out of
    ``bar(ref32, ref64)`` although the truncated-FIR form and any recursion still round."""
    rng = np.random.default_rng(seed)
    d, h, w = shape
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    smooth = 0.5 + 0.25 * np.sin(0.7 * z + 0.31 * y) * np.cos(0.23 * x + 0.4 * z)
    v = np.clip(smooth + 0.2 * rng.standard_normal(shape), 0, 1) * (2 ** bits - 1)
    return v.astype(np.float32)


def blocky_labels(shape, seed, block=3, values=(0, 1, 2, 3, 4)):
    rng = np.random.default_rng(seed)
    small = rng.choice(np.asarray(values, dtype=np.uint8), size=tuple(-(-s // block) for s in shape))
    big = small.repeat(block, 0).repeat(block, 1).repeat(block, 2)
    return np.ascontiguousarray(big[:shape[0], :shape[1], :shape[2]])
