"""Cases and fp64 references for the two geometric augmentation kernels of ``csrc/pointwise.hip``: ``k_warp_joint`` (through
``gpu_augment.warp_joint``) and ``k_elastic_nearest`` (through ``gpu_augment.elastic_deform``).  ``test_augment_cases_cpu.py`` proves
without a GPU that the cases and references are sound, ``test_augment_edges_gpu.py`` runs the kernels against them.

The references are written from the kernels' header comments (the DEFINITIONS), in fp64, on the same fp32 parameters the kernels receive:

  ref_warp     source(yo, xo) = A (xo, yo, 1) + D(yo, xo);  D = the P x P control grid, spanning the output, interpolated bilinearly
               (hat-function matrices: D_k = Ay c_k Ax^T);  image = sum over the four neighbours of hat(dy) hat(dx) value, zero outside the
               plane;  label = the pixel at floor(v + 0.5), zero outside.
  ref_elastic  d_k(y, x) = sum_ij B3(gy - i) B3(gx - j) coef_k[mirror(i), mirror(j)] with B3 the cubic B-spline BASIS FUNCTION,
               g = pixel (P - 1) / (size - 1) (0 when size == 1), whole-sample mirror;  image and labels are read at order 0
               (floor(c + 0.5)) at pixel + d, and are the constant 0 where a coordinate is below 0 or above size - 1.

Index planes.  ``index_mask``: value 1 + y W + x names its own position (0 = outside), so an output says which source pixel was read.

Rounding bounds (u = 2^-24, the unit round-off of fp32; first order, every constant rounded up).

(1) k_warp_joint, coordinates without control displacements.  xs = a0 xo + a1 yo + a2 is two products and two sums (xo, yo convert
exactly), each rounded once, each of a partial value whose magnitude is at most S = |a0| xo + |a1| yo + |a2|: |xs32 - xs64| <= 4 u S = dx
(contraction into fma only removes roundings).  dy likewise with a3, a4, a5.

(2) k_warp_joint, image.  wx = xs - floor(xs) is exact.  With |v| <= M and weights in [0, 1]: one row (1 - wx) v0 + wx v1 carries the
rounding of 1 - wx (<= u (1 - wx) M), two products (<= u M together) and a sum (<= u M): <= 3 u M.  The column step repeats it on the two
rows: 3 u M propagated (the weights sum to 1) + u (1 - wy) M + u M + u M <= 6 u M <= 8 u M, the bar.  Bilinear interpolation with zero fill
is continuous and piecewise linear with slopes at most Gx, Gy (the largest differences of adjacent samples of the zero-padded source), so
with inexact coordinates |got - ref| <= dx Gx + dy Gy + 8 u M -- for EVERY pixel.

(3) k_warp_joint, labels.  The kernel rounds once more: floor(fl(xs + 0.5f)), and that rounding (<= u (S + 1/2)) can carry a value just
below an integer onto it.  The coordinate bound 4 u S leaves this rounding out, so the label band uses dx + u (S + 1/2) (and the same
for y), 25 % wider than the coordinate bound alone; the image bound keeps 4 u S.  A pixel is IN THE BAND when a coordinate is within
that distance of a tie k + 1/2; there the kernel may read either neighbour (``candidates``), elsewhere it must read the reference's pixel.

(4) k_elastic_nearest, coordinate along one axis, C = max |coef[n, axis]| (d_axis reads no other coefficient; C = 0 gives d = 0 exactly, so
the band of such a plane is empty).  Counted on the kernel's expressions, no contraction assumed:
  g = y (P - 1) / (H - 1): product exact, one correctly rounded division, |dg| <= u (P - 1).  The kernel evaluates the spline at the rounded
    g exactly as defined (floor and fraction of an fp32 number are exact), and |d spline / dg| <= max |c_j - c_j-1| <= 2 C, so both axes
    together move d by <= 4 (P - 1) u C <= 16 u C for P <= 5.
  weights of one axis, f exact, g1 = fl(1 - f) (u relative): w0 = g1^3 / 6: 7 u relative of <= 1/6;  w3 = f^3 / 6: 4 u of <= 1/6;
    w1 = (4 - 6 f^2 + 3 f^3) / 6: (12 + 4 + 9 + 4) u / 6 + 2 u 2/3 <= 6.2 u;  w2, the same in g1: (24 + 4 + 18 + 4) u / 6 + 2 u 2/3 <= 9.7 u.
    Sum of the four absolute weight errors <= 18 u.
  row sums r = sum wx c: weight errors 18 u C, four products u C together, three roundings of partial sums 3 u C:  <= 22 u C.
  d = sum wy r: 22 u C propagated + 18 u C + u C + 3 u C = 44 u C.
  ys = fl(y + d) <= u (size + C), and the label's fl(ys + 0.5f) <= u (size + C + 1/2).
Total <= u ((44 + 16 + 2) C + 2 size + 1/2): ``elastic_delta`` uses u (64 C + 2 size + 1).  (A quick count -- 16 taps, two roundings each --
suggests 32 C; it misses the division and that a weight carries up to nine roundings, w2, so the derived 64 is used.)
A pixel is in the band when a coordinate is within that of k + 1/2, of 0 or of size - 1 (the last two guard the range test).
"""
import random

import numpy as np

U = 2.0 ** -24
EW_CAP_ITEMS = 2048 * 256          # work items of one trip of a capped elementwise grid (ew_grid, csrc/common.h)


# ---- index planes -------------------------------------------------------------------------------------------------------------------

def index_mask(n, h, w):
    return np.broadcast_to(1 + np.arange(h * w, dtype=np.int64).reshape(h, w), (n, h, w)).copy()


def index_value(y, x, h, w, inside=True):
    """The value an index plane holds at (y, x); 0 where ``inside`` is false or the position is off the plane."""
    ok = inside & (y >= 0) & (y < h) & (x >= 0) & (x < w)
    return np.where(ok, 1 + np.clip(y, 0, h - 1) * w + np.clip(x, 0, w - 1), 0).astype(np.int64)


def decode(v, w):
    """index value -> (inside, y, x)"""
    v = np.asarray(v).astype(np.int64)
    return v > 0, np.where(v > 0, (v - 1) // w, -1), np.where(v > 0, (v - 1) % w, -1)


# ---- references ---------------------------------------------------------------------------------------------------------------------

def _hat(t):
    return np.maximum(0.0, 1.0 - np.abs(t))


def _grid_pos(size, P):
    p = np.arange(size, dtype=np.float64)
    return p * (P - 1) / (size - 1) if size > 1 else np.zeros(size)


def control_field(ctrl, Ho, Wo):
    """[2, P, P] control displacements -> [2, Ho, Wo]: bilinear interpolation, first / last control point on the first / last output pixel."""
    c = np.asarray(ctrl, dtype=np.float64)
    P = c.shape[-1]
    Ay = _hat(_grid_pos(Ho, P)[:, None] - np.arange(P)[None, :])
    Ax = _hat(_grid_pos(Wo, P)[:, None] - np.arange(P)[None, :])
    return np.stack([Ay @ c[k] @ Ax.T for k in range(2)])


def _zero_filled(plane, y, x, fill=0):
    h, w = plane.shape
    ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
    return np.where(ok, plane[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], fill)


def ref_warp(img, msk, aff, ctrl, Ho, Wo, fault=None):
    """-> (image fp64 [N,Ho,Wo], labels int64 [N,Ho,Wo] or None, source coordinates fp64 [N,2,Ho,Wo] as (ys, xs)).
    ``fault`` (for the CPU test's "the bound has teeth" checks): 'swap' = wx and wy swapped, 'clamp' = the +1 taps clamped to the plane
    instead of zero-filled, 'half' = a half-pixel offset."""
    img = np.asarray(img, dtype=np.float64)
    N, H, W = img.shape
    aff = np.asarray(aff, dtype=np.float32).astype(np.float64).reshape(N, 6)
    if ctrl is not None:
        ctrl = np.asarray(ctrl, dtype=np.float32).astype(np.float64)
    yo, xo = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    oimg = np.zeros((N, Ho, Wo))
    omsk = None if msk is None else np.zeros((N, Ho, Wo), np.int64)
    coords = np.zeros((N, 2, Ho, Wo))
    for n in range(N):
        a = aff[n]
        xs = a[0] * xo + a[1] * yo + a[2]
        ys = a[3] * xo + a[4] * yo + a[5]
        if ctrl is not None:
            d = control_field(ctrl[n], Ho, Wo)
            ys, xs = ys + d[0], xs + d[1]
        coords[n, 0], coords[n, 1] = ys, xs
        if fault == "half":
            ys, xs = ys + 0.5, xs + 0.5
        by, bx = np.floor(ys).astype(np.int64), np.floor(xs).astype(np.int64)
        for da in (0, 1):
            for db in (0, 1):
                ty, tx = by + da, bx + db
                wy, wx = _hat(ys - ty), _hat(xs - tx)
                if fault == "swap":
                    wy, wx = _hat(xs - bx - da), _hat(ys - by - db)      # the row taps weighted by x's fraction and vice versa
                if fault == "clamp":
                    ty, tx = (np.minimum(ty, H - 1) if da else ty), (np.minimum(tx, W - 1) if db else tx)
                oimg[n] += wy * wx * _zero_filled(img[n], ty, tx, 0.0)
        if msk is not None:
            ny, nx = np.floor(coords[n, 0] + 0.5).astype(np.int64), np.floor(coords[n, 1] + 0.5).astype(np.int64)
            omsk[n] = _zero_filled(np.asarray(msk[n], dtype=np.int64), ny, nx)
    return oimg, omsk, coords


def _bspline3(t):
    """the cubic B-spline basis function"""
    t = np.abs(t)
    return np.where(t < 1.0, 2.0 / 3.0 - t * t + 0.5 * t ** 3, np.where(t < 2.0, (2.0 - t) ** 3 / 6.0, 0.0))


def _mirror(j, P):
    """whole-sample mirror: ... 2 1 | 0 1 .. P-1 | P-2 P-3 ..."""
    period = 2 * (P - 1)
    j = np.abs(j) % period
    return np.where(j >= P, period - j, j)


def _spline_matrix(size, P):
    """[size, P]: row y holds, per coefficient, the summed basis weights of every (mirrored) integer knot at g(y)."""
    g = _grid_pos(size, P)
    M = np.zeros((size, P))
    for j in range(-3, P + 3):
        M[:, int(_mirror(np.int64(j), P))] += _bspline3(g - j)
    return M


def elastic_field(coef, H, W):
    """[2, P, P] spline coefficients -> displacement field [2, H, W] (dy, dx), fp64"""
    c = np.asarray(coef, dtype=np.float64)
    My, Mx = _spline_matrix(H, c.shape[-1]), _spline_matrix(W, c.shape[-1])
    return np.stack([My @ c[k] @ Mx.T for k in range(2)])


def ref_elastic(img, msk, coef):
    """-> (image [N,H,W] in img's dtype, labels int64 or None, source coordinates fp64 [N,2,H,W] as (ys, xs)); ``coef``: the fp32
    coefficients the kernel receives."""
    img = np.asarray(img)
    N, H, W = img.shape
    coef = np.asarray(coef, dtype=np.float32).astype(np.float64)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    oimg = np.zeros_like(img)
    omsk = None if msk is None else np.zeros((N, H, W), np.int64)
    coords = np.zeros((N, 2, H, W))
    for n in range(N):
        d = elastic_field(coef[n], H, W)
        ys, xs = yy + d[0], xx + d[1]
        coords[n, 0], coords[n, 1] = ys, xs
        inside = (ys >= 0) & (ys <= H - 1) & (xs >= 0) & (xs <= W - 1)
        ny, nx = np.floor(ys + 0.5).astype(np.int64), np.floor(xs + 0.5).astype(np.int64)
        oimg[n] = np.where(inside, _zero_filled(img[n], ny, nx, img.dtype.type(0)), img.dtype.type(0))
        if msk is not None:
            omsk[n] = np.where(inside, _zero_filled(np.asarray(msk[n], dtype=np.int64), ny, nx), 0)
    return oimg, omsk, coords


# ---- bounds and the band rule ---------------------------------------------------------------------------------------------------------

def warp_delta(aff, Ho, Wo):
    """(dy, dx) [N,Ho,Wo] of the docstring's (1): 4 u (|a| xo + |a'| yo + |a''|), and the sums S themselves (for (3))."""
    a = np.abs(np.asarray(aff, dtype=np.float32).astype(np.float64)).reshape(-1, 6)
    yo, xo = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    Sx = a[:, 0, None, None] * xo + a[:, 1, None, None] * yo + a[:, 2, None, None]
    Sy = a[:, 3, None, None] * xo + a[:, 4, None, None] * yo + a[:, 5, None, None]
    return 4 * U * Sy, 4 * U * Sx, Sy, Sx


def warp_label_delta(aff, Ho, Wo):
    """(dy, dx) of the docstring's (3): the coordinate bound plus the rounding of v + 0.5f."""
    dy, dx, Sy, Sx = warp_delta(aff, Ho, Wo)
    return dy + U * (Sy + 0.5), dx + U * (Sx + 0.5)


def source_gradients(img):
    """(Gy, Gx): the largest absolute differences of vertically / horizontally adjacent samples of the zero-padded planes."""
    p = np.pad(np.asarray(img, dtype=np.float64), ((0, 0), (1, 1), (1, 1)))
    return float(np.abs(np.diff(p, axis=1)).max()), float(np.abs(np.diff(p, axis=2)).max())


def warp_image_bound(img, aff, Ho, Wo):
    """the docstring's (2), per pixel"""
    dy, dx, _, _ = warp_delta(aff, Ho, Wo)
    Gy, Gx = source_gradients(img)
    return dx * Gx + dy * Gy + 8 * U * float(np.abs(img).max())


def elastic_delta(coef, H, W):
    """[N, 2] (dy, dx) of the docstring's (4); 0 for a plane whose coefficients along that axis are all zero."""
    c = np.abs(np.asarray(coef, dtype=np.float32).astype(np.float64))
    assert c.shape[-1] <= 5, "the constant 64 covers P <= 5"
    C = c.reshape(c.shape[0], 2, -1).max(-1)
    size = np.array([H, W], dtype=np.float64)[None, :]
    return np.where(C > 0, U * (64 * C + 2 * size + 1), 0.0)


def candidates(c, d, size, closed):
    """The nearest-sample indices the kernel may take for a coordinate known to within d (d << 1/2, so [c - d, c + d] holds at most one
    decision point and its two ends enumerate the outcomes): (lo, hi), -1 = outside.  ``closed``: the elastic kernel's range test
    0 <= c <= size - 1 on the coordinate; otherwise the warp kernel's test 0 <= index < size."""
    out = []
    for v in (c - d, c + d):
        n = np.floor(v + 0.5).astype(np.int64)
        ok = ((v >= 0) & (v <= size - 1)) if closed else ((n >= 0) & (n < size))
        out.append(np.where(ok, n, -1))
    return out


def check_sources(got, coords, dy, dx, H, W, closed):
    """got: index values [N,h,w] read by the kernel; coords [N,2,h,w] fp64; dy, dx broadcastable to [N,h,w].
    -> (ok, band): ok = the value is one of the candidates (outside the band there is exactly one, the reference's); band = the
    pixel has more than one candidate."""
    cy = candidates(coords[:, 0], dy, H, closed)
    cx = candidates(coords[:, 1], dx, W, closed)
    got = np.asarray(got).astype(np.int64)
    ok = np.zeros(got.shape, bool)
    for y in cy:
        for x in cx:
            ok |= got == index_value(y, x, H, W, (y >= 0) & (x >= 0))
    band = (cy[0] != cy[1]) | (cx[0] != cx[1])
    return ok, band


# ---- part 1: exact cases of k_warp_joint --------------------------------------------------------------------------------------------------
# name -> (N, H, W, Ho, Wo, [matrix per sample], P).  Every matrix entry is a multiple of 1/8 of magnitude <= 4 (the 10^6 offset aside, an
# integer), offsets multiples of 1/8, sizes <= 512, image values integers 0..255, control displacements multiples of 1/4 in [-4, 4],
# Ho - 1 = (P - 1) 2^k: every intermediate of the kernel is a dyadic number of far fewer than 24 bits (test_augment_cases_cpu.py proves it).

def _t(dx, dy):
    return [1, 0, dx, 0, 1, dy]


_H, _W = 12, 20                                            # the small non-square plane
HFLIP, VFLIP, TURN = [-1, 0, _W - 1, 0, 1, 0], [1, 0, 0, 0, -1, _H - 1], [-1, 0, _W - 1, 0, -1, _H - 1]
SHEAR = [1, 0.25, 0, -0.125, 1, 0]
TRANSPOSE = [0, 1, 0, 1, 0, 0]
DOWN2, UP2 = [2, 0, 0.5, 0, 2, 0.5], [0.5, 0, -0.25, 0, 0.5, -0.25]
HALF_P, HALF_M = _t(0.5, 0.5), _t(-0.5, -0.5)

EXACT = {
    "shift-x-1": (1, _H, _W, _H, _W, [_t(-1, 0)], 0),
    "shift-y-1": (1, _H, _W, _H, _W, [_t(0, -1)], 0),
    "shift-x+W-1": (1, _H, _W, _H, _W, [_t(_W - 1, 0)], 0),
    "shift-y+H-1": (1, _H, _W, _H, _W, [_t(0, _H - 1)], 0),
    "shift-x+W-allzero": (1, _H, _W, _H, _W, [_t(_W, 0)], 0),
    "shift-x-W-allzero": (1, _H, _W, _H, _W, [_t(-_W, 0)], 0),
    "shift-1e6-allzero": (2, _H, _W, _H, _W, [_t(1e6, 0), _t(-1e6, -1e6)], 0),
    "half+": (1, _H, _W, _H, _W, [HALF_P], 0),
    "half-": (1, _H, _W, _H, _W, [HALF_M], 0),
    "down2": (1, _H, _W, _H // 2, _W // 2, [DOWN2], 0),
    "up2": (1, _H, _W, 2 * _H, 2 * _W, [UP2], 0),
    "transpose": (1, _H, _W, _W, _H, [TRANSPOSE], 0),
    "hflip": (1, _H, _W, _H, _W, [HFLIP], 0),
    "vflip": (1, _H, _W, _H, _W, [VFLIP], 0),
    "turn180": (1, _H, _W, _H, _W, [TURN], 0),
    "shear": (1, _H, _W, _H, _W, [SHEAR], 0),
    "batch6": (6, _H, _W, _H, _W, [_t(-1, 0), HALF_P, HFLIP, VFLIP, TURN, SHEAR], 0),
    "1x1": (2, 1, 1, 1, 1, [_t(0, 0), HALF_P], 0),
    "1x9-to-9x1": (1, 1, 9, 9, 1, [TRANSPOSE], 0),
    "ctrl-P2-17x17": (2, 17, 17, 17, 17, [_t(0, 0), _t(0.5, -0.25)], 2),
    "ctrl-P3-33x65": (2, 33, 65, 33, 65, [_t(0, 0), _t(-1, 2)], 3),
    "ctrl-P5-65x33": (2, 65, 33, 65, 33, [_t(0, 0), _t(0.25, 0)], 5),
    "ctrl-P3-Ho1": (2, 9, 33, 1, 33, [_t(0, 4), _t(0, 3.5)], 3),
    "ctrl-P3-Wo1": (2, 33, 9, 33, 1, [_t(4, 0), _t(4.5, 0)], 3),
    "gridstride-half+": (3, 419, 419, 419, 419, [HALF_P] * 3, 0),
    "gridstride-down2": (9, 484, 490, 242, 245, [DOWN2] * 9, 0),
}
ALL_ZERO = ("shift-x+W-allzero", "shift-x-W-allzero", "shift-1e6-allzero")


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def exact_case(name):
    """-> (img fp32 [N,H,W] of integers 0..255, index mask, aff fp32 [N,6], ctrl fp32 [N,2,P,P] or None, Ho, Wo)"""
    N, H, W, Ho, Wo, mats, P = EXACT[name]
    rs = np.random.RandomState(_seed(name))
    img = rs.randint(0, 256, (N, H, W)).astype(np.float32)
    ctrl = (rs.randint(-16, 17, (N, 2, P, P)) / 4.0).astype(np.float32) if P else None
    return img, index_mask(N, H, W), np.asarray(mats, dtype=np.float32), ctrl, Ho, Wo


# ---- part 2: rotations and crops as the loader draws them -----------------------------------------------------------------------------------
# name -> (N, H, W, Ho, Wo, seed).  The seeds are chosen so that (test_augment_cases_cpu.py asserts both) at most 1 % of the pixels lie in
# the label band and each of the three planted faults breaks the image bound on at least 1 % of the pixels.
DRAWN = {
    "33x47": (2, 33, 47, 33, 47, 2),
    "48x80-to-32x40": (2, 48, 80, 32, 40, 3),
    "64x64-to-96x96": (2, 64, 64, 96, 96, 3),
    "5x7-to-3x2": (2, 5, 7, 3, 2, 1),
    "3x419x419-gridstride": (3, 419, 419, 419, 419, 6),
}


def drawn_case(name):
    """-> (img fp32 in [0, 1], index mask, aff fp32 [N,6], Ho, Wo): angles in +-15 degrees, crops from ``resized_crop_params``"""
    import smsut_amd  # noqa: F401
    from smsut_amd.data_loader import gpu_augment as ga
    N, H, W, Ho, Wo, seed = DRAWN[name]
    state = random.getstate()
    random.seed(seed)
    aff = np.array([ga.affine_for(random.uniform(-15, 15), ga.resized_crop_params(H, W), (H, W), (Ho, Wo)) for _ in range(N)],
                   dtype=np.float32)
    random.setstate(state)
    img = np.random.RandomState(seed).rand(N, H, W).astype(np.float32)
    return img, index_mask(N, H, W), aff, Ho, Wo


# ---- part 3: k_elastic_nearest ----------------------------------------------------------------------------------------------------------------
# name -> (H, W, P, [per sample (sigma_y, sigma_x) or a constant (dy, dx) tagged 'const'], seed).  sigma in the reference's 9..13
# (config.data_aug) unless the plane is too small for such a draw to leave anything inside.
ELASTIC = {
    "P3-64x96": (64, 96, 3, [(9.0, 9.0), (13.0, 13.0)], 1),
    "P4-48x48": (48, 48, 4, [(9.0, 9.0), (11.0, 11.0)], 1),
    "P2-37x53": (37, 53, 2, [(10.0, 10.0), (13.0, 13.0)], 1),
    "P5-40x33": (40, 33, 5, [(9.0, 9.0), (12.0, 12.0)], 1),
    "P3-3x419x419-gridstride": (419, 419, 3, [(9.0, 9.0), (11.0, 11.0), (13.0, 13.0)], 1),
    "2x2": (2, 2, 3, [(11.0, 11.0), (0.4, 0.4), (0.4, 0.4), (0.3, 0.6), (0.6, 0.3), (1.0, 1.0)], 117),
    "1x9": (1, 9, 3, [(0.0, 2.0), (11.0, 11.0), (0.0, 11.0)], 1),
    "9x1": (9, 1, 3, [(2.0, 0.0), (11.0, 11.0), (11.0, 0.0)], 1),
    "zero-samples-0-and-2": (40, 56, 3, [(0.0, 0.0), (11.0, 11.0), (0.0, 0.0)], 1),
    "const+3-2": (208, 304, 3, [("const", 3.0, -2.0)], 1),       # (its band is one row and one column: 512 of 63232 pixels)
}
ELASTIC_NO_MASK = ("P3-64x96", "P5-40x33")                   # the shapes that also run with msk = None


def elastic_case(name):
    """-> (index image fp32 [N,H,W], index mask, control displacements fp32 [N,2,P,P]); the kernel's coefficients are
    ``gpu_augment.spline_prefilter(ctrl)``"""
    H, W, P, samples, seed = ELASTIC[name]
    rs = np.random.RandomState(seed)
    ctrl = np.zeros((len(samples), 2, P, P), np.float32)
    for n, s in enumerate(samples):
        if s[0] == "const":
            ctrl[n, 0], ctrl[n, 1] = s[1], s[2]
        else:
            ctrl[n, 0] = rs.standard_normal((P, P)) * s[0]
            ctrl[n, 1] = rs.standard_normal((P, P)) * s[1]
    msk = index_mask(len(samples), H, W)
    return msk.astype(np.float32), msk, ctrl
