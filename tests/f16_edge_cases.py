"""Case tables, restated launch plans and input generators of the fp16-operand convolution edge tests.  ``test_f16_edges_gpu.py`` runs
the kernels on them; ``test_f16_edges_cases_cpu.py`` checks, without a GPU, that the restated plans are self-consistent and that every
exact (tier A) case meets the conditions under which bit equality with fp64 is owed.  No GPU, no library call in here.

Tier A (exact): x, gy in [-4, 4], w in [-2, 2] are small integers, gradient operands those integers times G = 2^-23.  With the
power-of-two scale of ``smsut_absmax_scale`` every fp16 conversion, every product and every fp32 partial sum is exact in any summation
order, so the result must be BIT-EQUAL to the fp64 reference cast to fp32.  Conditions (not tolerances), see ``conditions_a`` /
``wgrad_conditions_a``: every converted value is fp16-representable; per statistics tile sum y^2 < 2^24; per BST tile
sum |gz xhat| < 2^24 in units of its power-of-two grid; weight gradients 16 N H W < 2^24.

Tier B (rounded operands): Gaussian fp32 inputs at real magnitudes (gradients 2e-7); the fp64 reference is computed from the operands
as the kernels are specified to round them -- ``x.half()``, ``w.half()``, ``(gy * s).half() / s`` -- so round-to-nearest-even at the
staging conversion and the placement of the gradient scale are pinned at the fp32 twins' bars."""
import torch
import torch.nn.functional as F

from conv_edge_helpers import (cdiv, conv3_64, dgrad3_64, fp16_exact, gen, rn, sums_exact, tap_conv3_64, tap_dgrad3_64, tile_sums,
                               wgrad3_64)

G = 2.0 ** -23               # the power of two the integer gradient operands are multiplied by (|gy| ~ 1e-7 at 512^2)
SLOPE_A = 0.25               # LeakyReLU slope of the exact cases: a power of two (it is an argument of the entry points)
SLOPE_B = 0.01
TAPS = (0, 4, 7, 8, -1)      # one-hot single taps (a wrong tap pairing shows as a missing tap) and the full 3x3 kernel (-1)


# ================================================================================================ restated plans
def fwd_p_eligible(n, h, w, k, m):
    """fwd_p_eligible (conv_mfma.hip)"""
    return (k in (8, 16, 32, 64) and w % 16 == 0 and h % 8 == 0 and m % 16 == 0 and n * (h // 8) * (w // 16) * (m // 16) >= 1024
            and n * h * w * max(k, m) < 2 ** 31)


def f16_supported(ks, k, m):
    """smsut_conv2d_f16_supported (conv_mfma.hip)"""
    return ks in (1, 3) and k >= 16 and k % 16 == 0 and m >= 1


def select_fwd_p_f16(h, k, m, split=0):
    """select_fwd_p with fp16 operands (conv_mfma.hip; no Winograd form, no 8-channel form): (TH, NTN, NCH)"""
    if k == 16 and h % 16 == 0:
        return (16, 1, 1)
    if k == 32 and m % 32 == 0 and not (split and split % 32 != 0):
        return (8, 2, 2)
    return {16: (8, 1, 1), 32: (8, 1, 2), 64: (8, 1, 4)}[k]


P_INSTANCES = ((16, 1, 1), (8, 1, 1), (8, 2, 2), (8, 1, 2), (8, 1, 4))       # every row of select_fwd_p fp16 operands can reach


def per_tile_row_f16(n, h, w, m, transposed):
    """dispatch_fwd<3> below the persistent kernel with fp16 operands (its launch_fwd rows, conv_mfma.hip; the 8-pixel-wide tile of the
    8x8-plane row asks !f16): (row name, TH, NTN).  The tile is always 16 pixels wide."""
    nt, tx = cdiv(m, 16), cdiv(w, 16)
    wg16 = tx * cdiv(h, 16) * n * ((nt + 1) // 2)
    wg8 = tx * cdiv(h, 8) * n * ((nt + 1) // 2)
    if h <= 4:
        return ("h4", 4, 1)
    if nt == 1:
        return ("nt1", 8, 1)
    if wg16 >= 512:
        return ("wg16", 16, 2)
    if wg8 >= 256 and not transposed:
        return ("wg8", 8, 2)
    return ("fall", 8, 1)


ROWS_FWD = {"h4", "nt1", "wg16", "wg8", "fall"}          # rows of that table a forward fp16 call can reach
ROWS_DGRAD = {"h4", "nt1", "wg16", "fall"}               # ("wg8" is forward-only: its row of dispatch_fwd asks !c.transposed_w)


def ckw_f16(ks, k, cat):
    """channels per LDS pass of the per-tile kernel with fp16 operands (launch_fwd, conv_mfma.hip)"""
    return 32 if (ks == 3 and k % 32 == 0 and k >= 32 and (not cat or (k // 2) % 32 == 0)) else 16


def plan_wgrad_f16(n, h, w, ci, co):
    """plan_wgrad_f16 over plan_wgrad (conv_mfma_wgrad.hip): (cit, cot, splits, tiles_per_split, total tiles).  The
    split plan is the fp32 kernels' (slabs counted with their CIT = Cin > 16), only the slab shape is the fp16 kernel's own."""
    cit0, cot0 = (2 if ci > 16 else 1), (2 if co > 16 else 1)
    total = n * cdiv(w, 16) * cdiv(h, 8)
    slabs = cdiv(ci, 16 * cit0) * cdiv(co, 16 * cot0)
    want = cdiv(768 if cit0 == 1 and cot0 == 1 else 512, slabs)
    want = max(min(want, max((8 << 20) // (ci * co * 9), 1), total), 1)
    tps = cdiv(total, want)
    return (2 if ci % 32 == 0 else 1), (2 if co % 32 == 0 else 1), cdiv(total, tps), tps, total


def wgrad_f16_supported(n, h, w, ci, co):
    """smsut_conv2d_wgrad_f16_supported = wgrad_f16_shape_ok (conv_mfma_wgrad.hip)"""
    return h % 8 == 0 and w % 16 == 0 and ci % 16 == 0 and co % 16 == 0 and n * h * w * max(ci, co) < 2 ** 31


# ================================================================================================ 1. per-tile kernel
# Shapes the persistent kernel declines, one or more per reachable row of per_tile_row_f16.
# Columns: n, h, w, ci, co, (forward row, data-gradient row or None), legs, splits of the data-gradient (over ci), splits of the
# forward (over co), KS == 1 as well.  Legs: fwd / fwd+ (transposed 0 / 2), stats, dgrad / acc (transposed 1 / 3), cat, split.
#   (3,3,19,16->4)      H <= 4 on a plane of 3 rows, W = 16 + 3, Ndim tail 4 (no data-gradient: Kdim 4); KS 1 too
#   (3,4,33,32->48)     H <= 4, W = 32 + 1, Kdim 32 (one 32-channel pass) / data-gradient Kdim 48 (three 16-channel passes); KS 1 too
#   (3,1,37,96->32)     a plane of ONE ROW; Kdim 96 (three 32-channel passes); cat 48 + 48 (16-channel passes); splits 16, 48 of 96
#   (3,13,19,48->16)    nt == 1 forward, ragged 13 x 19, Kdim 48; the data-gradient (16 -> 48) falls through
#   (3,9,35,16->32)     falls through forward; data-gradient (32 -> 16) nt == 1
#   (5,13,1,64->20)     a plane ONE PIXEL WIDE; Kdim 64, Ndim tail 20 = 16 + 4; cat 32 + 32 (32-channel passes); KS 1 too
#   (16,61,50,32->64)   wg16 = 4 * 4 * 16 * 2 = 512 -> <16,.,2> forward, H = 64 - 3, W = 48 + 2; data-gradient (64 -> 32: wg16 256,
#                       transposed) falls through; cat 16 + 16; splits 16 (data-gradient), 16 and 48 (forward)
#   (16,61,50,64->32)   forward wg16 = 256, wg8 = 4 * 8 * 16 = 512 -> <8,.,2>; data-gradient (32 -> 64) wg16 = 512 -> <16,.,2>
#   (16,61,50,16->40)   <16,.,2> with Ndim 40: the second 32-channel slab holds 8 channels
#   (11,30,47,32->40)   forward wg8 = 3 * 4 * 11 * 2 = 264, wg16 = 132 -> <8,.,2> with that tail, W = 48 - 1
BASIC = ("fwd", "fwd+", "stats", "dgrad", "acc")
FWD_ONLY = ("fwd", "fwd+", "stats")
PER_TILE = [
    (3, 3, 19, 16, 4, ("h4", None), FWD_ONLY, (), (), True),
    (3, 4, 33, 32, 48, ("h4", "h4"), BASIC + ("split",), (16,), (16,), True),
    (3, 1, 37, 96, 32, ("h4", "h4"), BASIC + ("cat", "split"), (16, 48), (16,), False),
    (3, 13, 19, 48, 16, ("nt1", "fall"), BASIC + ("split",), (16,), (), False),
    (3, 9, 35, 16, 32, ("fall", "nt1"), BASIC, (), (), False),
    (5, 13, 1, 64, 20, ("fall", None), FWD_ONLY + ("cat",), (), (), True),
    (16, 61, 50, 32, 64, ("wg16", "fall"), BASIC + ("cat", "split"), (16,), (16, 48), False),
    (16, 61, 50, 64, 32, ("wg8", "wg16"), BASIC + ("cat",), (), (), False),
    (16, 61, 50, 16, 40, ("wg16", None), FWD_ONLY, (), (), False),
    (11, 30, 47, 32, 40, ("wg8", None), FWD_ONLY + ("cat",), (), (), False),
]
# the one-hot taps run on the small planes; the four 16-image cases run the full kernel and the lone ninth tap
PER_TILE_TAPS = {c[:5]: (TAPS if c[0] * c[1] * c[2] < 10000 else (8, -1)) for c in PER_TILE}


# ================================================================================================ 2. persistent kernel
# units = N (H / 8) (W / 16) (Ndim / 16) >= 1024 (fwd_p_eligible); every plane has H != W.
# "edge": just over 1024 units, every form the shape has, every tap.  "walk" (every form, the full kernel): more items than the device can hold workgroups whatever the
# occupancy (8 per CU), an item count no candidate walk length divides -- the last workgroup is short and walks cross images.
# Columns: n, h, w, ci, co, kind, expected (TH, NTN, NCH) forward, data-gradient (or None: not persistent).
#   (171,16,48,16->16)  units 1026: <3,16,1,1> both ways; fused-shortcut data-gradient (Kdim 32 -> 16) <3,8,1,2>
#   (114,24,48,16->16)  units 1026: <3,8,1,1> (H % 16 == 8)
#   (57,24,48,32->32)   units 1026: <3,8,2,2>; a split 16 + 16 forces <3,8,1,2>; fused-shortcut data-gradient at 64 channels <3,8,1,4>
#   (115,24,48,32->16)  units 1035: <3,8,1,2> forward; data-gradient (16 -> 32, units 2070) <3,8,1,1>
#   (29,24,48,64->64)   units 1044: <3,8,1,4>
#   (293,56,16,16->16)  walk: items 2051 = 7 * 293      (293,112,16,16->16)  walk on 16-row items, 2051 of them too
#   (293,56,16,32->32)  walk <3,8,2,2>                  (293,56,16,32->16)   walk <3,8,1,2>
#   (79,56,16,64->64)   walk <3,8,1,4>: items 553 = 7 * 79, nz 4
PERSISTENT = [
    (171, 16, 48, 16, 16, "edge", (16, 1, 1), (16, 1, 1)),
    (114, 24, 48, 16, 16, "edge", (8, 1, 1), (8, 1, 1)),
    (57, 24, 48, 32, 32, "edge", (8, 2, 2), (8, 2, 2)),
    (115, 24, 48, 32, 16, "edge", (8, 1, 2), (8, 1, 1)),
    (29, 24, 48, 64, 64, "edge", (8, 1, 4), (8, 1, 4)),
    (293, 56, 16, 16, 16, "walk", (8, 1, 1), (8, 1, 1)),
    (293, 112, 16, 16, 16, "walk", (16, 1, 1), (16, 1, 1)),
    (293, 56, 16, 32, 32, "walk", (8, 2, 2), (8, 2, 2)),
    (293, 56, 16, 32, 16, "walk", (8, 1, 2), (8, 1, 1)),
    (79, 56, 16, 64, 64, "walk", (8, 1, 4), (8, 1, 4)),
]
WG_PER_CU = 8                                # workgroups of 256 threads a CU can hold


def edge_legs(n, h, w, ci, co):
    """every fp16-operand form the persistent kernel has for [ci -> co] on this plane"""
    legs = ["fwd", "stats", "hs", "hsx", "inaffhsx", "sc", "schs"]
    if fwd_p_eligible(n, h, w, co, ci) and co in (16, 32, 64):
        legs += ["dgrad", "acc", "bst", "bsths"]
        if ci >= 32:
            legs.append("split")
    if ci % 32 == 0:
        legs += ["cat", "hscat", "sccat", "schscat"]
    if co in (16, 32) and ci >= 16 and fwd_p_eligible(n, h, w, 2 * co, ci):
        legs.append("dsc")
        if ci >= 32:
            legs.append("dscsplit")
    return tuple(legs)


def persistent_splits(ci):
    """splits of a ci-channel result: at 16 (with ci == 32 that is split % 32 != 0 on a 32-channel-slab shape) and, from 64 on, at 32"""
    return (16,) if ci < 64 else (16, 32)


def walk_lengths(items, nz, cus):
    """launch_fwd_p (conv_mfma.hip): ipw = ceil(items nz / (CUs occ)) for the occupancy of the launched instantiation, which has
    no query: every value 1..8"""
    return {cdiv(items * nz, cus * occ) for occ in range(1, WG_PER_CU + 1)}


# ================================================================================================ 3. weight gradient
# conv_f16_wgrad<CIT, COT, DUAL, SC, XH, INAFF> (launch_wgrad_f16, conv_mfma_wgrad.hip): CIT = 2 iff Cin % 32 == 0, COT alike; DUAL
# = virtual cat, SC = fused shortcut (10 tap rows), XH = fp16 x, INAFF = raw fp16 y1 normalised while staged; grid (splits, Cin / 16 CIT,
# Cout / 16 COT).  Forms: plain, cat, sc, sccat, xh, xhaff.
# Columns: n, h, w, ci, co, forms, ca values of the cat forms, what the plane is.
#   (1,8,16)    ONE tile in total            (3,8,48)   one tile row             (3,24,16)  one tile column
#   (1,200,496,16->16)  25 * 31 = 775 tiles, want 768 -> 2 per split, 388 splits, the last holds ONE tile
#   (7,88,112,16->32) / (32->16)  7 * 11 * 7 = 539 tiles, want 512 -> 2 per split, 270 splits, last one tile
#   (3,72,304,32->32)   3 * 9 * 19 = 513 tiles, want 512 -> 2 per split, 257 splits, last one tile; 171 tiles per image: split 85 holds the
#                       last tile of image 0 and the first of image 1
#   48 -> 16: three slabs in grid y (CIT 1), 32 -> 96: three in grid z (COT 2)
ALL_PLAIN = ("plain", "sc", "xh", "xhaff")
WGRAD = [
    (1, 8, 16, 16, 16, ALL_PLAIN, (), "one tile"),
    (3, 8, 48, 16, 32, ALL_PLAIN, (), "tile row"),
    (3, 24, 16, 32, 16, ALL_PLAIN + ("cat", "sccat"), (16,), "tile column"),
    (3, 24, 16, 32, 32, ALL_PLAIN + ("cat", "sccat"), (16,), "tile column"),
    (3, 8, 48, 48, 16, ALL_PLAIN + ("cat", "sccat"), (16, 32), "tile row"),
    (1, 8, 16, 48, 32, ("plain", "cat", "sccat"), (32,), "one tile"),
    (3, 24, 16, 32, 96, ("plain", "sc"), (), "tile column"),
    (3, 8, 48, 64, 32, ("cat", "sccat"), (32,), "tile row"),
    (1, 200, 496, 16, 16, ("plain", "xhaff"), (), "short last split"),
    (7, 88, 112, 16, 32, ("plain",), (), "short last split"),
    (7, 88, 112, 32, 16, ("sc",), (), "short last split"),
    (3, 72, 304, 32, 32, ("plain", "xh", "cat"), (16,), "short last split"),
]
WGRAD_TIER_B = [(3, 24, 16, 32, 32), (7, 88, 112, 16, 32), (3, 8, 48, 48, 16)]


def wgrad_instance(ci, co, form):
    """(CIT, COT, DUAL, SC, XH, INAFF) of the kernel launch_wgrad_f16 starts for this form"""
    return (2 if ci % 32 == 0 else 1, 2 if co % 32 == 0 else 1, form in ("cat", "sccat"), form in ("sc", "sccat"),
            form in ("xh", "xhaff"), form == "xhaff")


WGRAD_INSTANCES = {(cit, cot) + f for cit in (1, 2) for cot in (1, 2)
                   for f in ((False, False, False, False), (True, False, False, False), (False, True, False, False),
                             (True, True, False, False), (False, False, True, False), (False, False, True, True))}


# ================================================================================================ inputs and references
def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


class Lazy:
    def __init__(self):
        self._c = {}

    def _get(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]


class IntRefs(Lazy):
    """tier A inputs of one shape (CPU, fp32, exactly representable in fp16 after the gradient scale) and their fp64 references.
    ks = 1: the weights are [ci, co] and every reference a matrix product."""

    def __init__(self, n, h, w, ci, co, seed=3, ks=3):
        super().__init__()
        self.shape, self.seed, self.ks = (n, h, w, ci, co), seed, ks

    def cpu(self, name):
        n, h, w, ci, co = self.shape
        mk = {"x": lambda: ints(gen(self.seed), -4, 4, n, h, w, ci),
              "gy": lambda: ints(gen(self.seed + 2), -4, 4, n, h, w, co) * G,
              "base": lambda: ints(gen(self.seed + 3), -4, 4, n, h, w, ci) * G,
              "basey": lambda: ints(gen(self.seed + 8), -4, 4, n, h, w, co),
              "w1": lambda: ints(gen(self.seed + 4), -2, 2, ci, co),
              "gs": lambda: ints(gen(self.seed + 5), -4, 4, n, h, w, co) * G,
              "w1d": lambda: ints(gen(self.seed + 6), -2, 2, ci, co)}
        return self._get(name, mk[name])

    def wt(self, tap=-1):
        """[3, 3, ci, co] integer weights: the full kernel (tap -1) or zero outside one tap; ks = 1: [ci, co]"""
        n, h, w, ci, co = self.shape

        def mk():
            if self.ks == 1:
                return ints(gen(self.seed + 1), -2, 2, ci, co)
            if tap < 0:
                return ints(gen(self.seed + 1), -2, 2, 3, 3, ci, co)
            wt = torch.zeros(3, 3, ci, co)
            wt[tap // 3, tap % 3] = ints(gen(self.seed + 10 + tap), -2, 2, ci, co)
            return wt
        return self._get(("wt", tap), mk)

    def _conv(self, x, tap):
        if self.ks == 1:
            return x.double() @ self.wt().double()
        return conv3_64(x, self.wt(tap)) if tap < 0 else tap_conv3_64(x, self.wt(tap)[tap // 3, tap % 3], tap)

    def _dgrad(self, gy, tap):
        if self.ks == 1:
            return gy.double() @ self.wt().double().t()
        return dgrad3_64(gy, self.wt(tap)) if tap < 0 else tap_dgrad3_64(gy, self.wt(tap)[tap // 3, tap % 3], tap)

    def aff(self):
        """integer mean / beta, power-of-two rstd / gamma and a y1 whose pre-activation (y1 - mean) rstd gamma + beta is one of
        {-8, -4, 1, 2, 3, 4}: never zero (asserted), and LeakyReLU at slope 1/4 gives the integers {-2, -1, 1, 2, 3, 4}.  xhat = (y1 -
        mean) rstd is a multiple of 1/2, y1 a multiple of 1/4 below 32: fp16 numbers."""
        def mk():
            n, h, w, ci, co = self.shape
            g = gen(self.seed + 7)
            mean, beta = ints(g, -2, 2, n, ci), ints(g, -2, 2, ci)
            rstd = 2.0 ** ints(g, -1, 1, n, ci)
            gam = 2.0 ** ints(g, 0, 1, ci)
            pre = torch.tensor([-8., -4., 1., 2., 3., 4.])[torch.randint(0, 6, (n, h, w, ci), generator=g)]
            y1 = (pre - beta) / (gam * rstd[:, None, None]) + mean[:, None, None]
            xhat = ((y1.double() - mean.double()[:, None, None]) * rstd.double()[:, None, None])
            chk = xhat * gam.double() + beta.double()
            assert bool((chk == pre.double()).all()) and float(pre.abs().min()) >= 1, "a pre-activation off its grid or at the kink"
            return {"mean": mean, "rstd": rstd, "gam": gam, "bet": beta, "y1": y1, "pre": pre.double(), "xhat": xhat,
                    "act": F.leaky_relu(pre, SLOPE_A)}
        return self._get("aff", mk)

    def ref(self, name, tap=-1):
        def mk():
            if name == "y":
                return self._conv(self.cpu("x"), tap)
            if name == "y+base":
                return self.ref("y", tap) + self.cpu("basey").double()
            if name == "gx":
                return self._dgrad(self.cpu("gy"), tap)
            if name == "gx+base":
                return self.ref("gx", tap) + self.cpu("base").double()
            if name == "yaff":
                return self._conv(self.aff()["act"], tap)
            if name == "gz":
                pre = self.aff()["pre"]
                return self.ref("gx", tap) * torch.where(pre > 0, 1.0, SLOPE_A).double()
            if name == "ysc":
                return self.cpu("x").double() @ self.cpu("w1").double()
            if name == "gxsc":
                return self.ref("gx", tap) + self.cpu("gs").double() @ self.cpu("w1d").double().t()
            raise AssertionError(name)
        return self._get(("ref", name, tap), mk)


def scale_window(t):
    """the two powers of two smsut_absmax_scale may choose: max |t| s in [2^13, 2^14]"""
    m = float(t.abs().max())
    return [s for s in (2.0 ** k for k in range(-20, 60)) if 2.0 ** 13 <= m * s <= 2.0 ** 14]


def conditions_a(R, legs, th, th_d=None, tap=-1):
    """the conditions under which tier A owes bit equality, asserted on the inputs and the fp64 references alone (th / th_d: rows of the
    statistics tile of the forward / the BST data-gradient launch; tiles are 16 pixels wide)"""
    assert fp16_exact(R.cpu("x")) and fp16_exact(R.wt(tap)), "an fp16 conversion would round"
    legs = set(legs)
    if legs & {"fwd", "stats", "cat", "hs", "hsx", "hscat", "sc", "sccat", "schs", "schscat"}:
        y = R.ref("y", tap)
        assert sums_exact(y, 1.0, th, 16) and sums_exact(y * y, 1.0, th, 16), "sum y^2 over a statistics tile reaches 2^24"
        assert fp16_exact(y), "the half-storage result would round twice"
    if legs & {"fwd+"}:
        assert fp16_exact(R.cpu("basey"))
    if legs & {"sc", "sccat", "schs", "schscat"}:
        assert fp16_exact(R.cpu("w1"))
        s = R.ref("ysc")
        assert sums_exact(s, 1.0, th, 16) and sums_exact(s * s, 1.0, th, 16)
    if legs & {"dgrad", "acc", "split", "bst", "bsths", "dsc", "dscsplit"}:
        gy = R.cpu("gy")
        for s in scale_window(gy):
            assert fp16_exact(gy.double() * s), "the scaled gradient operand is no fp16 number"
        assert float(gy.abs().max()) == 4 * G
        # products of the scaled operands are multiples of the scale's grid and the sum over 9 Kdim of them is far below 2^24 grid units
        assert 9 * R.shape[4] * 8 * 2 < 2 ** 24
    if legs & {"dsc", "dscsplit"}:
        both = torch.cat([R.cpu("gy").reshape(-1), R.cpu("gs").reshape(-1)])
        for s in scale_window(both):
            assert fp16_exact(R.cpu("gs").double() * s)
        assert fp16_exact(R.cpu("w1d"))
    if legs & {"inaffhsx", "bst", "bsths"}:
        a = R.aff()
        assert fp16_exact(a["y1"]) and fp16_exact(a["act"])
    if "inaffhsx" in legs:
        y = R.ref("yaff", tap)
        assert sums_exact(y, 1.0, th, 16) and sums_exact(y * y, 1.0, th, 16) and fp16_exact(y)
    if legs & {"bst", "bsths"}:
        gz = R.ref("gz", tap)
        assert sums_exact(gz, G / 4, th_d, 16), "sum |gz| over a BST tile reaches 2^24 grid units"
        assert sums_exact(gz * R.aff()["xhat"], G / 8, th_d, 16), "sum |gz xhat| over a BST tile reaches 2^24 grid units"


class WgradRefs(Lazy):
    """inputs and fp64 references of one weight-gradient shape; tier "A" (integers) or "B" (Gaussians, rounded as the kernel rounds)"""

    def __init__(self, n, h, w, ci, co, tier, seed=60):
        super().__init__()
        self.shape, self.tier, self.seed = (n, h, w, ci, co), tier, seed

    def cpu(self, name):
        n, h, w, ci, co = self.shape
        if self.tier == "A":
            mk = {"x": lambda: ints(gen(self.seed), -4, 4, n, h, w, ci), "gy": lambda: ints(gen(self.seed + 1), -4, 4, n, h, w, co) * G,
                  "gs": lambda: ints(gen(self.seed + 2), -4, 4, n, h, w, co) * G}
        else:
            mk = {"x": lambda: rn(gen(self.seed), n, h, w, ci), "gy": lambda: rn(gen(self.seed + 1), n, h, w, co, scale=2e-7),
                  "gs": lambda: rn(gen(self.seed + 2), n, h, w, co, scale=6e-7)}
        return self._get(name, mk[name])

    def aff(self):
        """tier A: as IntRefs.aff (slope 1/4).  Tier B: a raw fp16 y1 with Gaussian statistics (slope 0.01); the activated operand is
        computed in the kernel's own fp32 steps -- the subtraction rounds, the fma rounds once (product and sum held exactly in fp64),
        the LeakyReLU product rounds -- and THEN converted to fp16"""
        def mk():
            n, h, w, ci, co = self.shape
            if self.tier == "A":
                a = IntRefs(n, h, w, ci, co, seed=self.seed + 20).aff()
                return dict(a, slope=SLOPE_A)
            g = gen(self.seed + 7)
            mean, rstd = rn(g, n, ci, scale=0.2), 0.5 + torch.rand(n, ci, generator=g)
            gam, bet = 1 + 0.1 * rn(g, ci), 0.1 * rn(g, ci)
            y1 = rn(g, n, h, w, ci).half()
            d = y1.float() - mean[:, None, None]
            rg = rstd[:, None, None] * gam
            pre = (d.double() * rg.double() + bet.double()).float()
            act = torch.where(pre > 0, pre, pre * SLOPE_B)
            return {"mean": mean, "rstd": rstd, "gam": gam, "bet": bet, "y1": y1, "act": act, "slope": SLOPE_B}
        return self._get("aff", mk)

    def scale_ops(self, s, form):
        """(x, gy, gs) as fp64 of the operands the kernel multiplies, given the gradient scale s it was handed"""
        x = self.aff()["act"] if form == "xhaff" else self.cpu("x")
        rd = lambda t: (t.double() * s).float().half().double() / s
        return x.half().double(), rd(self.cpu("gy")), rd(self.cpu("gs"))

    def ref(self, s, form):
        """(gw [3, 3, ci, co], row 9 or None) in fp64"""
        def mk():
            x, gy, gs = self.scale_ops(s, form)
            sc = form in ("sc", "sccat")
            n, h, w, ci, co = self.shape
            return wgrad3_64(x, gy), (x.reshape(-1, ci).t() @ gs.reshape(-1, co)) if sc else None
        return self._get(("ref", s, form in ("sc", "sccat"), form == "xhaff"), mk)


def wgrad_conditions_a(R, forms):
    n, h, w, ci, co = R.shape
    assert 16 * n * h * w < 2 ** 24, "a weight-gradient sum could need a 25th bit"
    assert fp16_exact(R.cpu("x"))
    both = torch.cat([R.cpu("gy").reshape(-1), R.cpu("gs").reshape(-1)])
    for t in (R.cpu("gy"), both):
        assert float(t.abs().max()) == 4 * G
        for s in scale_window(t):
            assert fp16_exact(R.cpu("gy").double() * s) and fp16_exact(R.cpu("gs").double() * s)
    if "xhaff" in forms:
        a = R.aff()
        assert fp16_exact(a["y1"]) and fp16_exact(a["act"]) and float(a["act"].abs().max()) <= 4


class GaussRefs(Lazy):
    """tier B inputs of one forward-family shape: fp32 Gaussians at real magnitudes; references from the operands as the kernels round
    them"""

    def __init__(self, n, h, w, ci, co, seed=80):
        super().__init__()
        self.shape, self.seed = (n, h, w, ci, co), seed

    def cpu(self, name):
        n, h, w, ci, co = self.shape
        mk = {"x": lambda: rn(gen(self.seed), n, h, w, ci), "wt": lambda: rn(gen(self.seed + 1), 3, 3, ci, co, scale=(9 * ci) ** -0.5),
              "gy": lambda: rn(gen(self.seed + 2), n, h, w, co, scale=2e-7), "w1": lambda: rn(gen(self.seed + 4), ci, co, scale=ci ** -0.5),
              "base": lambda: rn(gen(self.seed + 3), n, h, w, ci, scale=2e-7)}
        return self._get(name, mk[name])

    def aff(self):
        def mk():
            n, h, w, ci, co = self.shape
            return WgradRefs(n, h, w, ci, co, "B", seed=self.seed + 30).aff()
        return self._get("aff", mk)

    def ref(self, name, s=1.0):
        def mk():
            xh, wh = self.cpu("x").half().double(), self.cpu("wt").half().double()
            if name == "y":
                return conv3_64(xh, wh)
            if name == "y_unrounded":                 # the 8-channel fused-shortcut half-storage form runs on fp32 operands
                return conv3_64(self.cpu("x"), self.cpu("wt"))
            if name == "gx":
                return dgrad3_64((self.cpu("gy").double() * s).float().half().double() / s, wh)
            if name == "gx+base":
                return self.ref("gx", s) + self.cpu("base").double()
            if name == "yaff":
                return conv3_64(self.aff()["act"].half().double(), wh)
            if name == "ysc":
                return xh @ self.cpu("w1").half().double()
            if name == "ysc_unrounded":
                return self.cpu("x").double() @ self.cpu("w1").double()
            raise AssertionError(name)
        return self._get((name, s), mk)
