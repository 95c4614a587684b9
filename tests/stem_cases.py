"""Case table, restated launch plan, operand families and fp64 references of the 5x5 stem edge tests (``csrc/conv_small.hip``:
``stem_fwd<1 / 5>``, ``stem_dgrad1``, ``stem_wgrad<1 / 5>`` behind ``smsut_conv2d_small_fwd`` / ``_small_dgrad`` /
``smsut_conv2d_flat_wgrad``).  ``test_stem_edges_gpu.py`` runs the kernels on them; ``test_stem_cases_cpu.py`` checks, without a GPU,
that every claim of the table follows from the restated plan and that every exact case meets the conditions under which bit equality
with fp64 is owed.  No GPU, no library call in here; the references run on whatever device their operands live on.

Tensors are NHWC, weights ``[KH][KW][Cin][Cout]``; the stem is Cin 1 / 5 -> 8 channels, 5x5, stride 1, pad 2.

Operand families:
  integer   x in {-2..2}, gy in {-1, 0, 1}, w and bias multiples of 1/8 in [-1, 1].  Every forward sum is a multiple of 1/8 below
            (125 * 2 + 1) * 8 < 2^24 units, every data-gradient sum one below 200 * 8, every weight-gradient sum an integer below
            sum |x| |gy| < 2^24: exact in fp32 in ANY order (and under any fma contraction), so the result must be BIT-EQUAL to the
            fp64 reference cast to fp32.  ``integer_conditions`` asserts this on the operands and references, nothing is assumed.
  one-hot   the dense operand is Gaussian fp32 with all 24 mantissa bits live, the other is 1.0 at one place and 0 elsewhere: the
            result is a shifted, zero-padded copy of the dense operand, bit for bit.  Catches what small integers cannot (an operand
            passed through a narrower type) and names the tap that is wrong.
  float     Gaussian operands at the scales of ``test_stem_5x5_kernels``; compared with the textbook bound of a K-term fp32 dot product,
            |got - ref64| <= (K + 2) 2^-24 A with A the same convolution of the absolute values in fp64."""
import torch
import torch.nn.functional as F

from conv_edge_helpers import cdiv, gen, rn, sums_exact

KS, PAD, CO = 5, 2, 8                      # SKS, SPD, SCO (conv_small.hip:245)
STY, STX = 16, 64                          # the stem kernels' pixel tile (conv_small.hip:245)
FTH, FTW = 8, 16                           # the flattened-M weight gradient's pixel tile (conv_small.hip:121), which sizes the workspace
FLAT_CAP = 2048                            # flat_plan's cap on the number of splits (conv_small.hip:452)
STEM_WGS = 512                             # stem_wgrad_wgs' cap on the number of workgroups (conv_small.hip:435)
CINS = (1, 5)
U = 2.0 ** -24                             # unit roundoff of fp32
ONE_HOT_CO = (1, 6)                        # one output channel in each float4 half of the 8


# ================================================================================================ restated plan
def stem_shape(h, w, ci, co=CO, k=KS, s=1, p=PAD):
    """stem_shape (conv_small.hip:429-432; Ho == H and Wo == W follow from k 5, s 1, p 2)"""
    return k == KS and s == 1 and p == PAD and co == CO and ci in (1, 5) and h % STY == 0 and w % STX == 0


def flat_plan(n, ho, wo):
    """flat_plan (conv_small.hip:447-456): (tiles_x, tiles_y, splits, tiles_per_split)"""
    tx, ty = cdiv(wo, FTW), cdiv(ho, FTH)
    total = n * tx * ty
    want = min(total, FLAT_CAP)
    tps = cdiv(total, want)
    return tx, ty, cdiv(total, tps), tps


def flat_ws(n, ho, wo, ci, co=CO, k=KS):
    """smsut_conv2d_flat_wgrad_ws (conv_small.hip:522-525): the stem kernel's slabs live in the workspace of the general plan"""
    return flat_plan(n, ho, wo)[2] * k * k * ci * co


def stem_wgrad_wgs(n, h, w, max_slabs):
    """stem_wgrad_wgs (conv_small.hip:433-438)"""
    total = n * (h // STY) * (w // STX)
    wgs = min(total, STEM_WGS)
    wgs = min(wgs, max_slabs)
    return max(wgs, 1)


class StemPlan:
    """the stem branch of smsut_conv2d_flat_wgrad (conv_small.hip:533-537): tpw = ceil(total / wgs), nwg = ceil(total / tpw); workgroup
    g accumulates tiles [g tpw, min((g + 1) tpw, total)) in registers (stem_wgrad, conv_small.hip:376-378) and writes slab g"""

    def __init__(self, n, h, w):
        assert h % STY == 0 and w % STX == 0
        self.n, self.h, self.w = n, h, w
        self.tiles_x, self.tiles_y = w // STX, h // STY
        self.per_image = self.tiles_x * self.tiles_y
        self.total = n * self.per_image
        self.slabs = flat_plan(n, h, w)[2]
        self.wgs = stem_wgrad_wgs(n, h, w, self.slabs)
        self.tpw = cdiv(self.total, self.wgs)
        self.nwg = cdiv(self.total, self.tpw)

    def tiles(self, g):
        return list(range(g * self.tpw, min((g + 1) * self.tpw, self.total)))

    def image(self, t):
        return t // self.per_image

    def origin(self, t):
        """(y0, x0) of tile t (stem_fwd / stem_dgrad1 / stem_wgrad: conv_small.hip:270-271, 318-319, 378-379)"""
        rem = t % self.per_image
        return (rem // self.tiles_x) * STY, (rem % self.tiles_x) * STX

    def images(self, g):
        return sorted({self.image(t) for t in self.tiles(g)})


# ================================================================================================ cases
# id: (n, h, w), each for Cin 1 and 5 -- the smallest shapes at which each mechanism exists
#   A (1,16,64)     one tile; every halo side is the image border
#   B (2,32,128)    2 x 2 tiles: interior seams both ways; a second image
#   C (3,48,64)     three tiles stacked: an odd tile count per image; a third image
#   D (1,16,192)    three tiles side by side
#   E (171,48,64)   513 tiles: tpw 2, nwg 257; workgroup 1 holds tiles 2, 3 = images 0 and 1; the last workgroup holds ONE tile
#   F (205,16,320)  1025 tiles: tpw 3, nwg 342; workgroups straddle images (5 tiles each); the last holds two tiles
STEM = {"A": (1, 16, 64), "B": (2, 32, 128), "C": (3, 48, 64), "D": (1, 16, 192), "E": (171, 48, 64), "F": (205, 16, 320)}
# one step outside the predicate: H % 16 == 8, W % 64 == 32 -> small_fwd / small_dgrad / flat_wgrad
NEAR = {"nearH": (2, 24, 64), "nearW": (2, 16, 96)}
ALL = dict(STEM, **NEAR)
ONE_HOT_SHAPES = ("A", "B")
TPW_NWG = {"A": (1, 1), "B": (1, 8), "C": (1, 9), "D": (1, 3), "E": (2, 257), "F": (3, 342)}


def assert_claims(cid):
    """every claim of the table above, from the restated plan: when the plan changes the case fails instead of testing something else"""
    n, h, w = ALL[cid]
    if cid in NEAR:
        assert not stem_shape(h, w, 1) and not stem_shape(h, w, 5)
        assert (h % STY, w % STX) == ((8, 0) if cid == "nearH" else (0, 32))
        assert stem_shape(h + 8 if cid == "nearH" else h, w + 32 if cid == "nearW" else w, 1), "one step from a stem plane"
        tx, ty, splits, tps = flat_plan(n, h, w)
        assert tps == 1 and splits == n * tx * ty
        return
    assert stem_shape(h, w, 1) and stem_shape(h, w, 5)
    p = StemPlan(n, h, w)
    assert (p.tpw, p.nwg) == TPW_NWG[cid]
    assert p.wgs == min(p.total, STEM_WGS) <= p.slabs, "the slab cap of stem_wgrad_wgs binds: the workspace no longer sizes the grid"
    assert p.nwg <= p.slabs, "more slabs than the workspace holds"
    assert (p.nwg - 1) * p.tpw < p.total <= p.nwg * p.tpw, "every workgroup holds a tile, together they hold all"
    if cid == "A":
        assert (p.tiles_x, p.tiles_y, p.total) == (1, 1, 1)
    elif cid == "B":
        assert (p.tiles_x, p.tiles_y, n) == (2, 2, 2)
    elif cid == "C":
        assert (p.tiles_x, p.tiles_y, n) == (1, 3, 3) and p.per_image % 2 == 1
    elif cid == "D":
        assert (p.tiles_x, p.tiles_y, n) == (3, 1, 1)
    elif cid == "E":
        assert p.total == 513 and p.tpw == 2 and p.nwg == 257
        assert p.tiles(1) == [2, 3] and p.images(1) == [0, 1]
        assert p.tiles(p.nwg - 1) == [512]
    elif cid == "F":
        assert p.total == 1025 and p.tpw == 3 and p.nwg == 342
        assert p.per_image == 5 and any(len(p.images(g)) == 2 for g in range(p.nwg))
        assert p.tiles(p.nwg - 1) == [1023, 1024]


def where(cid, idx):
    """a mismatching element (n, y, x, c) of a stem plane with its tile and in-tile coordinates, for a failure message"""
    n, y, x, c = (int(v) for v in idx)
    return f"(n {n}, y {y}, x {x}, c {c}): tile (row {y // STY}, col {x // STX}), in-tile (row {y % STY}, col {x % STX}, quad {x % STX // 4})"


def first_mismatch(got, ref):
    """index of the first element where got != ref (NaN counts), or None"""
    bad = (got != ref) | torch.isnan(got)
    if not bool(bad.any()):
        return None
    return tuple(int(v) for v in bad.nonzero()[0])


# ================================================================================================ operands
def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def integer_operands(cid, ci, seed=7):
    """CPU fp32: x in {-2..2}, gy in {-1, 0, 1}, w and bias multiples of 1/8 in [-1, 1]"""
    n, h, w = ALL[cid]
    g = gen(seed + 16 * ci + sum(map(ord, cid)))
    return {"x": ints(g, -2, 2, n, h, w, ci), "gy": ints(g, -1, 1, n, h, w, CO), "w": ints(g, -8, 8, KS, KS, ci, CO) / 8,
            "b": ints(g, -8, 8, CO) / 8}


def float_operands(cid, ci, seed=21):
    """CPU fp32 Gaussians at the scales of test_stem_5x5_kernels: x, gy, bias ~ N(0, 1), w ~ N(0, 1 / (25 Cin))"""
    n, h, w = ALL[cid]
    g = gen(seed + 16 * ci + sum(map(ord, cid)))
    return {"x": rn(g, n, h, w, ci), "gy": rn(g, n, h, w, CO), "w": rn(g, KS, KS, ci, CO, scale=(KS * KS * ci) ** -0.5), "b": rn(g, CO)}


def one_hot_weight(kh, kw, ci, co, cin):
    wt = torch.zeros(KS, KS, cin, CO)
    wt[kh, kw, ci, co] = 1.0
    return wt


def one_hot_taps(cin):
    """all 25 Cin taps for two output channels"""
    return [(kh, kw, ci, co) for kh in range(KS) for kw in range(KS) for ci in range(cin) for co in ONE_HOT_CO]


def one_hot_pixels(cid):
    """(image, y, x) of the one-hot gradient pixels that lie in the plane: the four corners, the four pixels round the first interior
    tile corner (15, 63) .. (16, 64), columns 60..67 of row 0 (the tile seam from both sides); the image cycles through the batch"""
    n, h, w = ALL[cid]
    px = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (15, 63), (16, 64), (15, 64), (16, 63)] + [(0, c) for c in range(60, 68)]
    px = sorted({(y, x) for y, x in px if y < h and x < w})
    return [(i % n, y, x) for i, (y, x) in enumerate(px)]


def one_hot_gy(cid, n0, y, x, co):
    n, h, w = ALL[cid]
    gy = torch.zeros(n, h, w, CO)
    gy[n0, y, x, co] = 1.0
    return gy


# ================================================================================================ references
def fwd64(x, wt, b=None):
    """fp64 5x5 stride-1 pad-2 conv, tap by tap (25 matrix products on doubles; test_stem_cases_cpu.py holds it to conv_ref): x
    [n,h,w,ci], wt [5,5,ci,co], b [co] or None -> y[y][x][:] = b + sum x[y + kh - 2][x + kw - 2][:] @ wt[kh][kw]"""
    n, h, w, ci = x.shape
    xp, wd = F.pad(x.double(), (0, 0, PAD, PAD, PAD, PAD)), wt.double()
    y = torch.zeros(n, h, w, wt.shape[3], dtype=torch.float64, device=x.device)
    if b is not None:
        y += b.double()
    for kh in range(KS):
        for kw in range(KS):
            y += xp[:, kh:kh + h, kw:kw + w, :] @ wd[kh, kw]
    return y


def dgrad64(gy, wt):
    """fp64 gradient of that conv with respect to its input: gx[y][x][:] = sum gy[y + 2 - kh][x + 2 - kw][:] @ wt[kh][kw]^T"""
    n, h, w, co = gy.shape
    gp, wd = F.pad(gy.double(), (0, 0, PAD, PAD, PAD, PAD)), wt.double()
    gx = torch.zeros(n, h, w, wt.shape[2], dtype=torch.float64, device=gy.device)
    for kh in range(KS):
        for kw in range(KS):
            gx += gp[:, 2 * PAD - kh:2 * PAD - kh + h, 2 * PAD - kw:2 * PAD - kw + w, :] @ wd[kh, kw].t()
    return gx


def wgrad64(x, gy):
    """fp64 gradient with respect to the weights, tap by tap: gw[kh][kw][ci][co] = sum x[y + kh - 2][x + kw - 2][ci] gy[y][x][co] (one
    small matrix product per image row, then the sum over the rows: a single [Cin, pixels] x [pixels, 8] product is one long serial
    reduction on a GPU)"""
    n, h, w, ci = x.shape
    xp = F.pad(x.double(), (0, 0, PAD, PAD, PAD, PAD))
    g3 = gy.double().reshape(n * h, w, gy.shape[3])
    gw = torch.empty(KS, KS, ci, gy.shape[3], dtype=torch.float64, device=x.device)
    for kh in range(KS):
        for kw in range(KS):
            gw[kh, kw] = torch.bmm(xp[:, kh:kh + h, kw:kw + w, :].reshape(n * h, w, ci).transpose(1, 2), g3).sum(0)
    return gw


def refs64(ops, bias=True):
    """{y, gx, gw} in fp64 of one operand set (on the operands' device)"""
    return {"y": fwd64(ops["x"], ops["w"], ops["b"] if bias else None), "gx": dgrad64(ops["gy"], ops["w"]), "gw": wgrad64(ops["x"], ops["gy"])}


def abs_refs64(ops, bias=True):
    """the same three convolutions of the absolute values: the A of the dot-product bounds"""
    return refs64({k: v.abs() for k, v in ops.items()}, bias)


def shifted(t, dy, dx):
    """out[n, y, x, :] = t[n, y + dy, x + dx, :], zero outside the plane (same dtype: a copy, bit for bit)"""
    n, h, w, c = t.shape
    tp = F.pad(t, (0, 0, PAD, PAD, PAD, PAD))
    return tp[:, PAD + dy:PAD + dy + h, PAD + dx:PAD + dx + w, :]


def one_hot_fwd_ref(x, kh, kw, ci, co):
    """forward with the one-hot weight (kh, kw, ci, co), no bias: channel co is x's channel ci shifted by the tap, the rest 0"""
    n, h, w, _ = x.shape
    y = torch.zeros(n, h, w, CO, dtype=x.dtype, device=x.device)
    y[..., co] = shifted(x, kh - PAD, kw - PAD)[..., ci]
    return y


def one_hot_dgrad_ref(gy, kh, kw, ci, co, cin):
    """data-gradient with that weight: channel ci is gy's channel co shifted the other way"""
    n, h, w, _ = gy.shape
    gx = torch.zeros(n, h, w, cin, dtype=gy.dtype, device=gy.device)
    gx[..., ci] = shifted(gy, PAD - kh, PAD - kw)[..., co]
    return gx


def one_hot_wgrad_ref(x, n0, y, xx, co):
    """weight gradient of a gy that is 1.0 at (n0, y, xx, co): column co is the 5x5 window of x round that pixel"""
    ci = x.shape[3]
    xp = F.pad(x[n0], (0, 0, PAD, PAD, PAD, PAD))
    gw = torch.zeros(KS, KS, ci, CO, dtype=x.dtype, device=x.device)
    gw[..., co] = xp[y:y + KS, xx:xx + KS, :]
    return gw


# ================================================================================================ exactness conditions
def integer_conditions(ops, refs, arefs):
    """the conditions under which the integer family owes bit equality, on the operands, the fp64 references (refs) and the references
    of the absolute values (arefs) alone: every term is a multiple of the unit and the sum of the absolute terms of EVERY result stays
    below 2^24 units, so no partial sum in any order needs a 25th bit"""
    x, gy, wt, b = (ops[k].double() for k in ("x", "gy", "w", "b"))
    for t, unit in ((x, 1.0), (gy, 1.0), (wt, 0.125), (b, 0.125)):
        assert bool((t / unit == (t / unit).round()).all()), "an operand off its grid"
    assert float(x.abs().max()) <= 2 and float(gy.abs().max()) <= 1 and float(wt.abs().max()) <= 1 and float(b.abs().max()) <= 1
    # forward / data-gradient: one sum per output element (1 x 1 tiles)
    for name in ("y", "gx"):
        assert sums_exact(refs[name], 0.125, 1, 1) and sums_exact(arefs[name], 0.125, 1, 1), f"{name}: a sum reaches 2^24 units"
    # weight gradient: one sum over all pixels per tap; |x[shifted] gy| <= (max of |x| over the 5x5 window and the channels) max_co |gy|
    # pixel by pixel, so the sum of that plane bounds the absolute sum of every tap
    n, h, w, ci = x.shape
    xm = F.max_pool2d(x.abs().amax(3)[:, None], KS, stride=1, padding=PAD)[:, 0]
    assert sums_exact((xm * gy.abs().amax(3))[..., None], 1.0), "sum |x gy| reaches 2^24"
    assert float(arefs["gw"].max()) < 2.0 ** 24 and bool((refs["gw"] == refs["gw"].round()).all())
    for v in refs.values():
        assert bool((v.float().double() == v).all()), "a reference is no fp32 number"


def asymmetric(wt):
    """no flip or transposition of the 5x5 window maps the weights to themselves (a mirrored tap index would go unseen)"""
    return not any(torch.equal(wt, v) for v in (wt.flip(0), wt.flip(1), wt.flip(0, 1), wt.transpose(0, 1), wt.transpose(0, 1).flip(0, 1)))
