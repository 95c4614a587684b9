"""The photometric augmentation (reference data_loader/baseLoader.py:102-109: ColorJitter on mode-L slices, then
RandomGammaCorrection) restated in plain numpy on 8-bit levels -- the reference of the device pass (csrc/photometric.hip).
``tests/test_photometric_cpu.py`` pins it to Pillow's own outputs through ``tests/golden/photometric_pil.npz``.  Also the shared
description of that fixture's cases, used by the generator, the CPU test and the GPU test.  Test infrastructure only: nothing
here runs on the product path.

    brightness = blend(0, v, b)          ImageEnhance.Brightness: degenerate image = black
    contrast   = blend(m, v, c)          ImageEnhance.Contrast: degenerate image = the constant m = int(mean + 0.5), the mean
                                         (integer sum / count, Python floats) of the image AS IT IS when the step runs
    blend(d, v, a): t = fp32(d) + fp32(a) * fp32(v - d), one fp32 multiply and one fp32 add (no fma); trunc(t) when
                    0 <= a <= 1, else 0 if t <= 0, 255 if t >= 255, else trunc(t)           (PIL's ImagingBlend)
    gamma: the table int((255 + 1 - 1e-3) * (l / 255) ** gamma) in float64 (torchvision's F.adjust_gamma restated), Image.point
"""
import numpy as np

F32 = np.float32


def quantise(x):
    """The 8-bit level of a value on the [0, 1] scale: floor(x * 255 + 0.5) in fp32 steps, clamped to 0..255."""
    x = np.asarray(x, dtype=F32)
    t = np.floor((x * F32(255.0)).astype(F32) + F32(0.5))
    return np.clip(t, 0.0, 255.0).astype(np.uint8)


def blend(d, v, a):
    a = F32(a)
    d = np.asarray(d, dtype=np.int32)
    v = np.asarray(v, dtype=np.int32)
    t = (d.astype(F32) + (a * (v - d).astype(F32)).astype(F32)).astype(F32)
    if F32(0.0) <= a <= F32(1.0):
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def brightness(img8, b):
    return blend(0, img8, b)


def contrast(img8, c):
    img8 = np.asarray(img8)
    m = int(int(img8.astype(np.int64).sum()) / img8.size + 0.5)
    return blend(m, img8, c)


def gamma_table(gamma):
    return np.array([int((255 + 1 - 1e-3) * (l / 255.0) ** float(gamma)) for l in range(256)], dtype=np.uint8)


def apply(img8, jitter=None, gamma=None):
    """One slice through the chain.  jitter: None or (order, b, c), order 0 = brightness first, 1 = contrast first;
    gamma: None (not drawn) or the exponent.  uint8 in, uint8 out."""
    out = np.asarray(img8, dtype=np.uint8)
    if jitter is not None:
        order, b, c = jitter
        out = contrast(brightness(out, b), c) if int(order) == 0 else brightness(contrast(out, c), b)
    if gamma is not None:
        out = gamma_table(gamma)[out]
    return out


# ---- the fixture's cases (tests/golden/make_photometric_golden.py records Pillow's output for each) -----------------------------
FACTORS = (0.6, 0.83, 1.0, 1.17, 1.4)
GAMMAS = (0.7, 1.0, 1.5)
PAIRS = ((0.6, 1.4), (1.4, 0.6), (0.83, 1.17), (1.17, 0.83), (1.0, 1.0))      # (b, c), each in both orders
ALL3 = ((0, 0.83, 1.4, 0.7), (1, 1.17, 0.6, 1.5), (0, 1.4, 1.4, 1.5), (1, 0.6, 0.6, 0.7))


def cases():
    """[(kind, order, b, c, gamma)]: order -1 = no jitter; gamma nan = none.  'brightness' / 'contrast' alone are recorded from the
    one Pillow enhancer and run here (and on the device) with the other factor 1.0, which is the identity: blend(d, v, 1) = v."""
    nan = float("nan")
    cs = [("brightness", 0, f, 1.0, nan) for f in FACTORS]
    cs += [("contrast", 0, 1.0, f, nan) for f in FACTORS]
    cs += [("both", o, b, c, nan) for o in (0, 1) for (b, c) in PAIRS]
    cs += [("gamma", -1, 1.0, 1.0, g) for g in GAMMAS]
    cs += [("all", o, b, c, g) for (o, b, c, g) in ALL3]
    return cs


def case_args(row):
    """A fixture row [order, b, c, gamma] -> (jitter, gamma) as ``apply`` and the device pass take them."""
    order, b, c, g = (float(v) for v in row)
    return (None if order < 0 else (int(order), b, c)), (None if np.isnan(g) else g)


def images():
    """The fixture's 8-bit inputs: full-range random, >= 90 % zeros with a bright blob, constant, low range (0-63, odd size)."""
    rs = np.random.RandomState(20)
    rand = rs.randint(0, 256, (20, 31)).astype(np.uint8)
    sparse = np.zeros((48, 64), np.uint8)
    yy, xx = np.mgrid[0:48, 0:64]
    blob = (yy - 20) ** 2 + (xx - 40) ** 2 < 64
    sparse[blob] = (255 - 3 * np.sqrt((yy - 20) ** 2 + (xx - 40) ** 2)[blob]).astype(np.uint8)
    sparse[5, 7:12] = (3, 90, 91, 200, 254)
    const = np.full((24, 32), 137, np.uint8)
    low = rs.randint(0, 64, (17, 23)).astype(np.uint8)
    assert (sparse == 0).mean() >= 0.9
    return {"rand": rand, "sparse": sparse, "const": const, "low": low}
