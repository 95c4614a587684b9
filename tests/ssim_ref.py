"""Reference and case table of the translation metrics (csrc/similarity.hip, ``ops.image_similarity``).  Not a test.

The definitions, restated from the formulas in fp64 NumPy:
  window   w[k] = exp(-k^2 / (2 1.5^2)), k = -5 .. 5, normalised to sum 1 in fp64; the 2-D window is w (x) w
  moments  at every centre at least 5 pixels from each edge ((H-10)(W-10) centres): mu_a, mu_b the window-weighted means,
           s_a^2 = E_w[a^2] - mu_a^2, s_b^2 alike, s_ab = E_w[ab] - mu_a mu_b   (population moments)
  SSIM     (2 mu_a mu_b + C1)(2 s_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(s_a^2 + s_b^2 + C2)), C1 = (0.01 L)^2, C2 = (0.03 L)^2;
           a slice's SSIM is the mean over its centres   (Wang et al. 2004)
  SE, AE   sum (a-b)^2 and sum |a-b| over all H W pixels, each value converted to fp64 before the subtraction
and a FLOAT32 restatement of the same SSIM expression that rounds every step to fp32 (``ssim_mean(..., np.float32)``): the
distance between the two is the reference's own rounding, from which tests/test_similarity_gpu.py derives its bar."""
import functools

import numpy as np

# the kernel's tile of window centres: constexpr TH, TW in csrc/similarity.hip (one workgroup per TH x TW centres of one slice)
TH, TW = 32, 64
RADIUS = 5
FAMILIES = ("independent", "perturbed", "blob", "identical", "constant", "grid8")


def window(dt=np.float64):
    k = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    w = np.exp(-k * k / (2 * 1.5 ** 2))
    w /= w.sum()
    return w.astype(dt)


def _filt(a, w, dt):
    """Valid 11 x 11 separable filter: taps left to right, then top to bottom, every step rounded to ``dt``."""
    h, wd = a.shape
    n = 2 * RADIUS
    t = np.zeros((h, wd - n), dt)
    for k in range(n + 1):
        t = (t + w[k] * a[:, k:k + wd - n]).astype(dt)
    o = np.zeros((h - n, wd - n), dt)
    for k in range(n + 1):
        o = (o + w[k] * t[k:k + h - n, :]).astype(dt)
    return o


def ssim_map(x, y, dt=np.float64, data_range=1.0):
    """The SSIM value of every window centre, [(H-10), (W-10)], computed in ``dt``."""
    x, y, w = np.asarray(x).astype(dt), np.asarray(y).astype(dt), window(dt)
    c1, c2 = dt((0.01 * data_range) ** 2), dt((0.03 * data_range) ** 2)
    mx, my = _filt(x, w, dt), _filt(y, w, dt)
    xx, yy, xy = _filt((x * x).astype(dt), w, dt), _filt((y * y).astype(dt), w, dt), _filt((x * y).astype(dt), w, dt)
    sx, sy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
    s = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx + sy + c2))
    assert s.dtype == dt
    return s


def ssim_mean(x, y, dt=np.float64, data_range=1.0):
    """A slice's SSIM: the fp64 mean of ``ssim_map`` computed in ``dt``."""
    return float(ssim_map(x, y, dt, data_range).astype(np.float64).mean())


def ssim_scipy(x, y, data_range=1.0):
    """skimage's form of the same: ``gaussian_filter(sigma=1.5, truncate=3.5, mode='reflect')`` moments, cropped by 5 pixels."""
    from scipy.ndimage import gaussian_filter
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    f = lambda v: gaussian_filter(v, sigma=1.5, truncate=3.5, mode="reflect")
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mx, my = f(x), f(y)
    sx, sy, sxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
    s = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx + sy + c2))
    return float(s[RADIUS:-RADIUS, RADIUS:-RADIUS].mean())


def se_ae(x, y):
    d = np.asarray(x).astype(np.float64) - np.asarray(y).astype(np.float64)
    return float((d * d).sum()), float(np.abs(d).sum())


def psnr_of(se, voxels, data_range=1.0):
    return float("inf") if se == 0 else float(10.0 * np.log10(data_range ** 2 / (se / voxels)))


# ------------------------------------------------------------------------------------------- inputs
def make_pair(family, h, w, seed):
    """One seeded (a, b) pair of fp32 [h, w] images in [0, 1]."""
    rng = np.random.default_rng([seed, h, w, FAMILIES.index(family)])
    x = rng.random((h, w))
    if family == "independent":                      # uniform noise against independent uniform noise
        a, b = x, rng.random((h, w))
    elif family == "perturbed":                      # noise against itself plus N(0, 0.05), clipped
        a, b = x, np.clip(x + 0.05 * rng.standard_normal((h, w)), 0, 1)
    elif family == "blob":                           # smooth blob on an exactly-zero background; noise inside the blob only
        yy, xx = np.mgrid[0:h, 0:w]                  # (the cancellation case: the variances are ~0 next to C2)
        s = 0.5 + 0.5 * np.sin(xx / 7.0) * np.cos(yy / 5.0)
        m = ((xx - w / 2) ** 2 + (yy - h / 2) ** 2) < (min(h, w) / 3) ** 2
        a = s * m
        b = np.clip(a + 0.02 * rng.standard_normal((h, w)) * m, 0, 1)
    elif family == "identical":
        a = x
        b = x.copy()
    elif family == "constant":
        a, b = np.full((h, w), 0.7), np.full((h, w), 0.7)
    elif family == "grid8":                          # values on the 8-bit grid k / 255
        a = np.round(x * 255) / 255
        b = np.round(np.clip(x + 0.1 * rng.standard_normal((h, w)), 0, 1) * 255) / 255
    else:
        raise KeyError(family)
    return a.astype(np.float32), b.astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(family, h, w, seed, scale=1.0):
    """(a, b, ssim64, ssim32, SE, AE) of one slice, computed once and shared (the arrays are read-only).  ``scale``: inputs and
    data_range multiplied by it (255: the 8-bit range)."""
    a, b = make_pair(family, h, w, seed)
    if scale != 1.0:
        a, b = (a * np.float32(scale)).astype(np.float32), (b * np.float32(scale)).astype(np.float32)
    a.setflags(write=False); b.setflags(write=False)
    se, ae = se_ae(a, b)
    return a, b, ssim_mean(a, b, np.float64, scale), ssim_mean(a, b, np.float32, scale), se, ae


def batch(family, h, w, n, scale=1.0):
    """n slices of one family (seeds 0 .. n-1): stacked (a, b) and per-slice reference lists."""
    cs = [case(family, h, w, s, scale) for s in range(n)]
    return (np.stack([c[0] for c in cs]), np.stack([c[1] for c in cs]), [c[2] for c in cs], [c[3] for c in cs],
            [c[4] for c in cs], [c[5] for c in cs])


def ssim_bar(ref32, ref64):
    """|gpu - ref64| may be 16 times the float32 restatement's own distance from fp64, or 16 fp32 ulps of 1, whichever is more."""
    return max(16.0 * abs(ref32 - ref64), 16.0 * 2.0 ** -23)


def shapes():
    """(H, W) of the kernel tests: every tile-edge combination of window-centre counts up to 256 a side, plus the fixed shapes."""
    out = [(ch + 10, cw + 10) for ch in (1, TH - 1, TH, TH + 1, 2 * TH + 3) for cw in (1, TW - 1, TW, TW + 1, 2 * TW + 3)
           if ch + 10 <= 256 and cw + 10 <= 256]
    for s in ((11, 11), (11, 12), (12, 11), (13, 13), (12, 37), (43, 42), (21, 300), (256, 256)):
        if s not in out:
            out.append(s)
    return out


SCALED_SHAPES = ((13, 13), (43, 42), (TH + 11, TW + 11))     # data_range 255 with inputs x 255
