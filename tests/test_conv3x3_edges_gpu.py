"""The 3x3 stride-1 MFMA convolution kernels -- the Winograd / persistent families and the LDS weight gradients that
``test_conv_families_gpu.py`` leaves out -- against fp64 on the CPU, each through its own C-ABI entry point, at the shapes where its
launch plan, its tile walk or its staging changes:

  1. the resident-weight Winograd kernel ``conv_mfma_fwd_p<3, 16, 1, NCH, .., WINO>`` (Kdim 16 / 32; csrc/conv_mfma.hip),
  2. the streamed-weight Winograd kernel ``conv_wino_l<NTN, ..>`` (Kdim >= 64; csrc/conv_wino.hip) with one and two slabs per wave,
  3. the direct persistent forms ``conv_mfma_fwd_p<3, TH, NTN, NCH, K8, N8>`` (8-row items, 8-channel reduction / result, Kdim 64,
     the fused-shortcut data-gradient at 64 reduction channels) and every instantiation ``select_fwd_p`` can choose through
     ``smsut_conv2d_fwd_mfma_cfg``,
  4. the per-tile kernel ``conv_mfma_fwd<3, TH, 4, 1, NTN, false, MW>`` on ragged planes and channel tails,
  5. the LDS weight-gradient kernels ``conv_mfma_wgrad<3, CIT, COT, ..>``, ``plane_wgrad`` and the three ``sum_splits`` widths.

Conventions (as in ``test_conv_families_gpu.py``): tensors are NHWC, weights ``[KH][KW][Cin][Cout]``; every reference is fp64
(``F.conv2d`` / ``F.conv_transpose2d`` / ``torch.nn.grad.conv2d_weight`` on doubles, computed once per shape on the CPU and shared by
the on-the-fly and the prepared run); outputs are NaN inside and carry a sentinel guard behind them in the same allocation; statistics
buffers and workspaces are exactly their query's size with the same guard; every ``*_supported`` predicate is asserted before a
launch.  Every case asserts the kernel family it claims through the library's queries (``smsut_conv2d_mfma_form`` /
``_persistent`` / ``_tiles``); what has no query (NTN, ntn, the weight-gradient kernel) is restated from the cited source lines.
The items-per-workgroup count has no query: walk cases are sized from the hardware bound (a CU holds at most 8 workgroups of 256
threads; ``conv_wino_l`` runs one per CU) against the CU count of the device.

Bars, on max |got - ref| / max |ref|: 2e-6 forward / data-gradient, 5e-6 the input-side-InstanceNorm and BST forms, 3e-6 weight
gradients over <= ~1e5 pixels and 5e-5 beyond; statistics partials as the existing tests (rtol 1e-5, atol 1e-3).  Each leg prints its
figure."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conv_edge_helpers import based_buf, cdiv, conv3_64, dgrad3_64, gen, out_buf, poisoned, rn, untouched, wgrad3_64

pytestmark = pytest.mark.gpu

FWD_BAR = 2e-6
AFF_BAR = 5e-6
WGRAD_BAR = 3e-6
WGRAD_BAR_BIG = 5e-5
SLOPE = 0.01
WG_PER_CU = 8                # workgroups of 256 threads a CU can hold: the bound on the persistent kernels' occupancy

BASIC = ("fwd", "stats", "dgrad", "acc")


@pytest.fixture(scope="module")
def H():
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return _hip


@pytest.fixture(scope="module")
def cus(H):
    return torch.cuda.get_device_properties(0).multi_processor_count


def check(tag, got, ref, bar):
    """max |got - ref| / max |ref| against an fp64 reference that already lives on the device"""
    e = float((got.double() - ref).abs().max() / ref.abs().max())
    print(f"{tag}: rel_err {e:.3g} bar {bar:.3g}")
    assert e < bar, tag              # (a NaN left in `got` gives e = nan, and nan < bar is False)


def check_partials(tag, part, n, tiles, c, col0, col1, rtol=1e-5, atol0=1e-3, atol1=1e-3):
    """statistics partials [n][tiles][c][2] summed over tiles against the two per-image, per-channel sums (fp64 of the kernel's output)"""
    p = part[:n * tiles * c * 2].view(n, tiles, c, 2).double().sum(1)
    d0, d1 = float((p[..., 0] - col0).abs().max()), float((p[..., 1] - col1).abs().max())
    print(f"{tag}: partial sums off by {d0:.3g} / {d1:.3g} (atol {atol0:.3g} / {atol1:.3g}, rtol {rtol:.3g})")
    assert torch.allclose(p[..., 0], col0, rtol=rtol, atol=atol0), tag
    assert torch.allclose(p[..., 1], col1, rtol=rtol, atol=atol1), tag


class Prepared:
    """smsut_wino_prepare for one weight tensor, both forms (0: forward image of [ci -> co], 1: data-gradient image); the images are
    passed to the `_pre` entry points by ``call``"""

    def __init__(self, H, w, ci, co):
        forms = [(0, ci, co), (1, co, ci)]
        self.u, self.g = zip(*[poisoned(H.call("smsut_wino_image_floats", k, m)) for _, k, m in forms])
        PA, IA = ctypes.c_void_p * 2, ctypes.c_int * 2
        self.arr = (PA(w.data_ptr(), w.data_ptr()), PA(*[u.data_ptr() for u in self.u]), IA(ci, co), IA(co, ci), IA(0, 1))
        H.call("smsut_wino_prepare", *[ctypes.addressof(a) for a in self.arr], 2, H.stream_ptr())


def call(H, keep, name, tr, *args):
    """the entry point, or -- with prepared images -- its `_pre` form with the image of this form (tr: 0 forward, 1 data-gradient)
    in front of the stream"""
    if keep is None:
        return H.call(name, *args)
    return H.call(name + "_pre", *args[:-1], keep.u[tr & 1], args[-1])


class Refs:
    """inputs of one shape and their fp64 references, each computed on first use on the CPU and kept on the device"""

    def __init__(self, n, h, w, ci, co, seed):
        self.shape = (n, h, w, ci, co)
        self.seed = seed
        self._c = {}

    def _get(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    def cpu(self, name):
        n, h, w, ci, co = self.shape
        mk = {"x": lambda: rn(gen(self.seed), n, h, w, ci), "wt": lambda: rn(gen(self.seed + 1), 3, 3, ci, co, scale=(9 * ci) ** -0.5),
              "gy": lambda: rn(gen(self.seed + 2), n, h, w, co), "base": lambda: rn(gen(self.seed + 3), n, h, w, ci),
              "w1": lambda: rn(gen(self.seed + 4), ci, co, scale=ci ** -0.5), "gs": lambda: rn(gen(self.seed + 5), n, h, w, co),
              "w1d": lambda: rn(gen(self.seed + 6), ci, co, scale=co ** -0.5)}
        return self._get("cpu_" + name, mk[name])

    def dev(self, name):
        return self._get("dev_" + name, lambda: self.cpu(name).cuda())

    def aff(self):
        """mean / rstd [n, ci], gamma / beta [ci] handed to the kernels as they are, and a y1 [n, h, w, ci] built so that NO fp64
        pre-activation (y1 - mean) rstd gamma + beta lies within 1e-4 max|pre| of zero: the LeakyReLU mask of the BST form cannot
        flip under fp32 rounding (asserted here, on the CPU)"""
        def mk():
            n, h, w, ci, co = self.shape
            g = gen(self.seed + 7)
            mean, rstd = rn(g, n, ci, scale=0.2), 0.5 + torch.rand(n, ci, generator=g)
            gam, bet = 1 + 0.1 * rn(g, ci), 0.1 * rn(g, ci)
            t = rn(g, n, h, w, ci).double()
            t = torch.sign(t) * (0.05 + t.abs())
            y1 = (((t - bet.double()) / gam.double()) / rstd.double()[:, None, None] + mean.double()[:, None, None]).float()
            xhat = (y1.double() - mean.double()[:, None, None]) * rstd.double()[:, None, None]
            pre = xhat * gam.double() + bet.double()
            assert float(pre.abs().min()) > 1e-4 * float(pre.abs().max()), "a pre-activation sits at the LeakyReLU kink"
            return {"mean": mean.cuda(), "rstd": rstd.cuda(), "gam": gam.cuda(), "bet": bet.cuda(), "y1": y1.cuda(), "pre": pre,
                    "xhat": xhat.cuda()}
        return self._get("aff", mk)

    def ref(self, name):
        def mk():
            x, wt = self.cpu("x"), self.cpu("wt")
            if name == "y":
                r = conv3_64(x, wt)
            elif name == "gx":
                r = dgrad3_64(self.cpu("gy"), wt)
            elif name == "gx+base":
                r = self.ref("gx").cpu() + self.cpu("base").double()
            elif name == "yaff":
                r = conv3_64(F.leaky_relu(self.aff()["pre"], SLOPE), wt)
            elif name == "gz":
                pre = self.aff()["pre"]
                r = self.ref("gx").cpu() * torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, SLOPE))
            elif name == "ysc":
                r = x.double() @ self.cpu("w1").double()
            elif name == "gxsc":
                r = self.ref("gx").cpu() + self.cpu("gs").double() @ self.cpu("w1d").double().t()
            return r.contiguous().cuda()
        return self._get("ref_" + name, mk)


_REFS = {}


def refs_for(n, h, w, ci, co, seed=3):
    """one shape at a time: the on-the-fly and the prepared run of a case are neighbours and share the references"""
    key = (n, h, w, ci, co, seed)
    if key not in _REFS:
        _REFS.clear()
        _REFS[key] = Refs(n, h, w, ci, co, seed)
    return _REFS[key]


def img_sums(t):
    d = t.double()
    return d.sum((1, 2)), (d * d).sum((1, 2))


def run_forms(H, n, h, w, ci, co, legs, prepared=False, splits=None, seed=3):
    """every listed form of the 3x3 conv [ci -> co] on n x h x w against fp64.  Forward-side legs reduce over ci (Kdim = ci, Ndim =
    co), data-gradient-side legs over co (Kdim = co, Ndim = ci); the fused-shortcut data-gradient reduces over 2 co."""
    st = H.stream_ptr()
    R = refs_for(n, h, w, ci, co, seed)
    keep = Prepared(H, R.dev("wt"), ci, co) if prepared else None
    guards = list(keep.g) if keep else []
    tag = f"{n}x{h}x{w} {ci}->{co}{' prepared' if prepared else ''}"
    assert H.call("smsut_conv2d_mfma_supported", 3, 1, 1, ci, co) == 1
    if set(legs) & {"dgrad", "acc", "split", "bst"}:
        assert H.call("smsut_conv2d_mfma_supported", 3, 1, 1, co, ci) == 1
    splits = splits if splits is not None else (16 * (ci // 32),)
    wd = R.dev("wt")
    y_plain = None
    tiles = H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 0)

    def new_stats(c=co, t=None):
        buf, g = poisoned(n * (t or tiles) * c * 2)
        guards.append(g)
        return buf

    def new_out(c):
        t, g = out_buf(n, h, w, c)
        guards.append(g)
        return t

    for leg in legs:
        if leg == "fwd":
            y_plain = new_out(co)
            call(H, keep, "smsut_conv2d_fwd_mfma", 0, R.dev("x"), wd, y_plain, n, h, w, ci, co, 3, 0, st)
            check(f"{tag} fwd", y_plain, R.ref("y"), FWD_BAR)
        elif leg == "stats":
            ys, part = new_out(co), new_stats()
            call(H, keep, "smsut_conv2d_fwd_mfma_stats", 0, R.dev("x"), wd, ys, part, n, h, w, ci, co, 3, st)
            assert torch.equal(ys, y_plain), "the statistics epilogue must not change y"
            check_partials(f"{tag} stats", part, n, tiles, co, *img_sums(ys))
        elif leg == "dgrad":
            gx = new_out(ci)
            call(H, keep, "smsut_conv2d_fwd_mfma", 1, R.dev("gy"), wd, gx, n, h, w, co, ci, 3, 1, st)
            check(f"{tag} dgrad", gx, R.ref("gx"), FWD_BAR)
        elif leg == "acc":
            acc, g = based_buf(R.cpu("base"))
            guards.append(g)
            call(H, keep, "smsut_conv2d_fwd_mfma", 1, R.dev("gy"), wd, acc, n, h, w, co, ci, 3, 3, st)
            check(f"{tag} accumulate", acc, R.ref("gx+base"), FWD_BAR)
        elif leg == "inaff":
            assert H.call("smsut_conv2d_mfma_persistent", n, h, w, ci, co, 3, 0) == 1
            a = R.aff()
            y2, part = new_out(co), new_stats()
            call(H, keep, "smsut_conv2d_fwd_mfma_stats_inaff", 0, a["y1"], wd, y2, part, a["mean"], a["rstd"], a["gam"], a["bet"], SLOPE,
                 n, h, w, ci, co, st)
            check(f"{tag} input-side IN", y2, R.ref("yaff"), AFF_BAR)
            check_partials(f"{tag} input-side IN stats", part, n, tiles, co, *img_sums(y2))
        elif leg == "bst":
            assert H.call("smsut_conv2d_mfma_persistent", n, h, w, co, ci, 3, 0) == 1
            a = R.aff()
            tb = H.call("smsut_conv2d_mfma_tiles", n, h, w, co, ci, 3, 0)
            gz, pb = new_out(ci), new_stats(ci, tb)
            call(H, keep, "smsut_conv2d_dgrad_mfma_bwdstats", 1, R.dev("gy"), wd, gz, pb, a["y1"], a["mean"], a["rstd"], a["gam"], a["bet"],
                 SLOPE, n, h, w, co, ci, st)
            check(f"{tag} BST (no mask flip allowed)", gz, R.ref("gz"), AFF_BAR)
            check_partials(f"{tag} BST stats", pb, n, tb, ci, gz.double().sum((1, 2)), (gz.double() * a["xhat"]).sum((1, 2)),
                           rtol=1e-4, atol0=1e-3, atol1=2e-3)
        elif leg == "cat":
            assert H.call("smsut_conv2d_mfma_cat_supported", n, h, w, ci, co) == 1
            xa, xb = R.dev("x")[..., :ci // 2].contiguous(), R.dev("x")[..., ci // 2:].contiguous()
            y, part = new_out(co), new_stats()
            call(H, keep, "smsut_conv2d_fwd_mfma_stats_cat", 0, xa, xb, wd, y, part, n, h, w, ci, co, st)
            check(f"{tag} virtual cat", y, R.ref("y"), FWD_BAR)
            check_partials(f"{tag} virtual cat stats", part, n, tiles, co, *img_sums(y))
        elif leg == "split":
            for tr in (1, 3):
                for sp in splits:
                    assert H.call("smsut_conv2d_mfma_split_supported", n, h, w, co, ci, sp) == 1
                    if tr == 3:
                        (ga, g1), (gb, g2) = based_buf(R.cpu("base")[..., :sp].contiguous()), based_buf(R.cpu("base")[..., sp:].contiguous())
                        guards.extend([g1, g2])
                    else:
                        ga, gb = new_out(sp), new_out(ci - sp)
                    call(H, keep, "smsut_conv2d_fwd_mfma_split", 1, R.dev("gy"), wd, ga, gb, sp, n, h, w, co, ci, tr, st)
                    check(f"{tag} split {sp}+{ci - sp} transposed {tr}", torch.cat([ga, gb], 3), R.ref("gx+base" if tr == 3 else "gx"), FWD_BAR)
        elif leg in ("sc", "sccat"):
            cat = leg == "sccat"
            assert H.call("smsut_conv2d_fwd_sc_supported", n, h, w, ci, co, int(cat)) == 1
            xa = R.dev("x")[..., :ci // 2].contiguous() if cat else R.dev("x")
            xb = R.dev("x")[..., ci // 2:].contiguous() if cat else None
            y2, s2, p2, q2 = new_out(co), new_out(co), new_stats(), new_stats()
            call(H, keep, "smsut_conv2d_fwd_mfma_stats_sc", 0, xa, xb, wd, R.dev("w1"), y2, s2, p2, q2, n, h, w, ci, co, st)
            assert torch.equal(y2, y_plain), "the fused shortcut must not change y"
            check(f"{tag} fused shortcut{' (cat)' if cat else ''} ysc", s2, R.ref("ysc"), FWD_BAR)
            check_partials(f"{tag} fused shortcut y stats", p2, n, tiles, co, *img_sums(y2))
            check_partials(f"{tag} fused shortcut ysc stats", q2, n, tiles, co, *img_sums(s2))
        elif leg in ("dsc", "dscsplit"):
            sps = splits if leg == "dscsplit" else (0,)
            for sp in sps:
                assert H.call("smsut_conv2d_dgrad_sc_supported", n, h, w, co, ci, sp) == 1
                ga, gb = (new_out(sp), new_out(ci - sp)) if sp else (new_out(ci), None)
                H.call("smsut_conv2d_dgrad_mfma_sc", R.dev("gy"), R.dev("gs"), wd, R.dev("w1d"), ga, gb, sp, n, h, w, co, ci, st)
                check(f"{tag} fused shortcut dgrad{f' split {sp}' if sp else ''} (form {H.call('smsut_conv2d_mfma_form', n, h, w, 2 * co, ci, 1)})",
                      torch.cat([ga, gb], 3) if sp else ga, R.ref("gxsc"), FWD_BAR)
        else:
            raise AssertionError(leg)
    torch.cuda.synchronize()
    assert untouched(*guards), f"{tag}: a guard behind an output, a statistics buffer or a prepared image was written"


def full_legs(ci, co):
    """every form the persistent kernels have for [ci -> co]: virtual cat needs two halves of whole 16-channel chunks (ci % 32 == 0),
    a split two parts of whole 16-channel tiles (ci >= 32), the fused-shortcut data-gradient co in {16, 32}
    (smsut_conv2d_dgrad_sc_supported, conv_mfma.hip), the BST form a reduction width (co) the persistent kernels take"""
    legs = list(BASIC) + ["inaff"]
    if co in (16, 32, 64) or (co >= 64 and co % 16 == 0):
        legs.append("bst")
    if ci % 32 == 0:
        legs += ["cat", "split"]
    legs.append("sc")
    if ci % 32 == 0:
        legs.append("sccat")
    if co in (16, 32):
        legs.append("dsc")
        if ci % 32 == 0:
            legs.append("dscsplit")
    return tuple(legs)


def ipw_candidates(items, nz, cus):
    """launch_fwd_p (conv_mfma.hip): ipw = ceil(items nz / (CUs occ)) for the occupancy occ of the launched instantiation,
    which has no query: every value 1..8 a CU can hold"""
    return {cdiv(items * nz, cus * occ) for occ in range(1, WG_PER_CU + 1)}


def assert_walk(items, nz, cus, tail):
    """a persistent launch whose workgroups walk more than one item whatever the occupancy; tail: the last workgroup is short"""
    assert items * nz > WG_PER_CU * cus, "not a walk on this device"
    cands = ipw_candidates(items, nz, cus)
    assert min(cands) >= 2
    if tail:
        assert all(items % ipw for ipw in cands), (items, sorted(cands))


def is_prime(v):
    return v > 1 and all(v % d for d in range(2, int(v ** 0.5) + 1))


# ================================================================================================ 1. resident Winograd
# dispatch_fwd<3> (conv_mfma.hip) sends a shape to select_fwd_p when fwd_p_eligible (Kdim in {8, 16, 32, 64},
# W % 16 == 0, H % 8 == 0, Ndim % 16 == 0, N (H / 8) (W / 16) (Ndim / 16) >= 1024); select_fwd_p (its winograd_on() row) takes the Winograd
# instantiation launch_fwd_p<3, 16, 1, NCH, false, false, true> for Kdim = 16 NCH in {16, 32} on H % 16 == 0: 16 x 16 items, NTN = 1
# (nz = Ndim / 16).  units = N (H / 8) (W / 16) (Ndim / 16); items = N (H / 16) (W / 16).
#   (2053,16,16,16->16)  items 2053 (prime), nz 1: a walk by 5 items over 8 CUs' worth; data-gradient the same kernel.  FULL.
#   (1031,32,16,32->32)  items 2062 = 2 * 1031, two per image, nz 2: ipw in {3, 4, 5, 6, 9, 17} for occupancy 8..1, none divides
#                        2062: a ragged last workgroup and walks across image boundaries.  FULL (NCH = 2: cat, split, both shortcuts).
#   (347,32,48,16->32)   items 2082, six per image, nz 2 forward (NCH 1) / nz 1 data-gradient (Kdim 32: NCH 2).
#   (512,16,16,16->16)   units = 1024 exactly: the smallest eligible 16 x 16 plane count, no walk.
#   (511,16,16,16->16)   units = 1022: one image below -- form 0, the per-tile kernel <8,4,1,1> (nt = 1) on full tiles.
#   (171,16,48,32->48)   one tile row of three, Ndim 48 (nz 3), units 3078; the data-gradient (Kdim 48) is the per-tile kernel's.
#   (86,32,16,16->48)    one tile column of two, Ndim 48, units 1032; data-gradient per-tile.
# Columns: n, h, w, ci, co, legs ("full" / "basic"), walk (None / "walk" / "tail"), expected (forward, data-gradient) form.
RESIDENT = [(2053, 16, 16, 16, 16, "full", "tail", (1, 1)), (1031, 32, 16, 32, 32, "full", "tail", (1, 1)),
            (347, 32, 48, 16, 32, "basic", "walk", (1, 1)), (512, 16, 16, 16, 16, "basic", None, (1, 1)),
            (511, 16, 16, 16, 16, "basic", None, (0, 0)), (171, 16, 48, 32, 48, "basic", None, (1, 0)),
            (86, 32, 16, 16, 48, "basic", None, (1, 0))]


def units(n, h, w, ndim):
    return n * (h // 8) * (w // 16) * (ndim // 16)


def _id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}-{c[5]}" + (f"-{c[6]}" if c[6] else "")


@pytest.mark.parametrize("case", RESIDENT, ids=[_id(c) for c in RESIDENT])
def test_resident_winograd(H, cus, case):
    n, h, w, ci, co, legs, walk, (ff, fd) = case
    assert H.call("smsut_conv2d_mfma_form", n, h, w, ci, co, 0) == ff
    assert H.call("smsut_conv2d_mfma_form", n, h, w, co, ci, 0) == fd
    assert H.call("smsut_conv2d_mfma_persistent", n, h, w, ci, co, 3, 0) == ff
    if ff == 1:
        assert units(n, h, w, co) >= 1024 and ci in (16, 32) and h % 16 == 0 and w % 16 == 0
        assert H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 0) == (h // 16) * (w // 16)       # 16-row items
    else:
        assert units(n, h, w, co) == 1022 and units(n + 1, h, w, co) == 1024
        assert H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 0) == cdiv(h, 8) * cdiv(w, 16)    # the per-tile kernel's 8-row tiles
    if case[:5] == (512, 16, 16, 16, 16):
        assert units(n, h, w, co) == 1024
    items = n * (h // 16) * (w // 16)
    if walk:
        assert_walk(items, co // 16, cus, walk == "tail")
        if fd == 1:
            assert_walk(items, ci // 16, cus, walk == "tail")
        if walk == "tail":
            assert is_prime(n)
    else:
        assert items * (co // 16) <= WG_PER_CU * cus
    run_forms(H, n, h, w, ci, co, full_legs(ci, co) if legs == "full" else BASIC)


# ================================================================================================ 2. streamed Winograd
# select_fwd_p (conv_mfma.hip) hands every fp32 form of a wino_l_shape (Kdim >= 64 and smsut_wino_l_eligible,
# conv_wino.hip:853-856: H % 16 == W % 16 == 0, Kdim % 16 == Ndim % 16 == 0) to smsut_wino_l_launch (conv_wino.hip:858-873):
#   ntn = 2 when Ndim % 32 == 0 && !(y2 && split % 32 != 0) && items (Ndim / 32) >= CUs, else 1       (conv_wino.hip:867)
#   nz = Ndim / (16 ntn), ipw = ceil(items nz / CUs), grid.x = ceil(items / ipw)                         (conv_wino.hip:786-792)
# with items = N (H / 16) (W / 16).  Per case, for 256 CUs (the test recomputes all of it from the device's count):
#   (257,16,16,64->32)   items 257 (prime).  fwd ntn 2, nz 1, ipw 2: 129 workgroups, the last with one item.  FULL.  Its data-gradient
#                        (Kdim 32) is the resident kernel's, its fused-shortcut data-gradient (Kdim 64) the direct one (sc2_64, part 3).
#   (257,16,16,64->48)   Ndim % 32 != 0 -> ntn 1, nz 3, ipw 4 (257 % 4 = 1).  FULL without BST / dsc (co = 48 is no persistent reduction).
#   (131,32,16,128->64)  items 262, two per image (one tile column).  fwd ntn 2, nz 2, ipw 3 (262 % 3 = 1: ragged, crosses images);
#                        data-gradient Kdim 64 -> Ndim 128: ntn 2, nz 4, ipw 5; split 16 + 112: ntn 1 BECAUSE OF THE SPLIT, nz 8, ipw 9;
#                        split 64 + 64 keeps ntn 2.  BST on the streamed kernel.
#   (64,16,32,96->64)    items 128 < CUs, one tile row of two: ntn 2 (128 * 2 = 256 >= CUs), nz 2, ipw 1.
#   (5,32,16,96->48)     items 10, one tile column: ntn 1 (Ndim 48), nz 3.  Data-gradient (Kdim 48) per-tile.
#   (33,16,32,128->64)   items 66 < CUs: fwd ntn 1 (66 * 2 < CUs); data-gradient Ndim 128: 66 * 4 >= 256 -> ntn 2; split 48 + 80 -> ntn 1
#                        because of the split.
# Columns: n, h, w, ci, co, legs, splits, walk ("tail" or None), (forward, data-gradient) form, (ntn forward, ntn data-gradient or None)
STREAMED = [(257, 16, 16, 64, 32, "full", (32,), "tail", (2, 1), (2, None)),
            (257, 16, 16, 64, 48, "full", (32,), "tail", (2, 0), (1, None)),
            (131, 32, 16, 128, 64, BASIC + ("split", "bst"), (16, 64), "tail", (2, 2), (2, 2)),
            (64, 16, 32, 96, 64, BASIC, (), None, (2, 2), (2, 2)),
            (5, 32, 16, 96, 48, BASIC, (), None, (2, 0), (1, None)),
            (33, 16, 32, 128, 64, BASIC + ("split",), (48,), None, (2, 2), (1, 2))]


def ntn_of(items, ndim, cus, split=0):
    """conv_wino.hip:867"""
    return 2 if (ndim % 32 == 0 and not (split and split % 32 != 0) and items * (ndim // 32) >= cus) else 1


def _sid(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}-{'full' if c[5] == 'full' else 'basic'}" + (f"-{c[7]}" if c[7] else "")


@pytest.mark.parametrize("prepared", [False, True], ids=["on-the-fly", "prepared"])
@pytest.mark.parametrize("case", STREAMED, ids=[_sid(c) for c in STREAMED])
def test_streamed_winograd(H, cus, case, prepared):
    n, h, w, ci, co, legs, splits, walk, (ff, fd), (nf, nd) = case
    assert ff == 2 and ci >= 64
    assert H.call("smsut_conv2d_mfma_form", n, h, w, ci, co, 0) == ff
    assert H.call("smsut_conv2d_mfma_form", n, h, w, co, ci, 0) == fd
    assert H.call("smsut_conv2d_mfma_persistent", n, h, w, ci, co, 3, 0) == 1
    assert H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 0) == (h // 16) * (w // 16)
    items = n * (h // 16) * (w // 16)
    assert ntn_of(items, co, cus) == nf
    ipw = cdiv(items * (co // (16 * nf)), cus)
    if walk:
        assert items * (co // (16 * nf)) > cus and ipw >= 2 and items % ipw != 0 and is_prime(n)
    else:
        assert items < cus
    if fd == 2:
        assert ntn_of(items, ci, cus) == nd
        for sp in splits:
            want = 1 if sp % 32 else nd
            assert ntn_of(items, ci, cus, sp) == want
            ipw_s = cdiv(items * (ci // (16 * want)), cus)
            if walk:
                assert ipw_s >= 2 and items % ipw_s != 0
        if splits:
            assert any(sp % 32 for sp in splits) and nd == 2, "a case whose split alone forces one slab"
    if legs == "full":
        legs = full_legs(ci, co)
    run_forms(H, n, h, w, ci, co, legs, prepared=prepared, splits=splits)


# ================================================================================================ 3. direct persistent forms
# select_fwd_p (conv_mfma.hip) for the shapes the Winograd forms leave (H % 16 == 8, Kdim 8, Ndim 8, Kdim 64 off 16-row planes):
#   Ndim 8 (data-gradient forms; dispatch_fwd<3> with fwd_p_n8_eligible: Kdim in {16, 32}, N (H / 8) (W / 16) >= 1024):
#            Kdim 16 -> <3,16,1,1,N8> on H % 16 == 0 else <3,8,1,1,N8>; Kdim 32 -> <3,8,1,2,N8>
#   Kdim 8  -> <3,16,1,1,K8> on H % 16 == 0 else <3,8,1,1,K8>
#   Kdim 32, Ndim % 32 == 0, no split off 32 -> <3,8,2,2>;  Kdim 16 -> <3,8,1,1>;  Kdim 32 -> <3,8,1,2>;  Kdim 64 -> <3,8,1,4>
# TH = 8 items: tiles = (H / 8) (W / 16).
#   (127,24,48,16->16)  units 1143: <3,8,1,1> both ways            (59,24,48,32->32)  units 1062: <3,8,2,2> both ways; split 16 + 16 -> <3,8,1,2>
#   (115,24,48,32->16)  units 1035: <3,8,1,2>; data-gradient (Kdim 16, Ndim 32, units 2070) <3,8,1,1>
#   (29,24,48,64->64)   units 1044: <3,8,1,4>, Winograd declines H % 16 == 8
#   (1031,8,16,16->16)  units 1031: planes of ONE 8-row item
#   (293,56,16,16->16)  the walk: items 2051 = 7 * 293 (293 prime), seven per image, nz 1, ipw in {2, 3, 5, 9} for occupancy 8..1, none
#                       divides 2051: a ragged last workgroup and walks across image boundaries.  FULL.
DIRECT = [(127, 24, 48, 16, 16, "full", None), (59, 24, 48, 32, 32, "full", None), (115, 24, 48, 32, 16, "full", None),
          (29, 24, 48, 64, 64, "full", None), (1031, 8, 16, 16, 16, "basic", None), (293, 56, 16, 16, 16, "full", "tail")]


@pytest.mark.parametrize("case", DIRECT, ids=[_id(c) for c in DIRECT])
def test_direct_persistent_8row_items(H, cus, case):
    n, h, w, ci, co, legs, walk = case
    assert h % 16 == 8
    for k, m in ((ci, co), (co, ci)):
        assert H.call("smsut_conv2d_mfma_form", n, h, w, k, m, 0) == 0
        assert H.call("smsut_conv2d_mfma_persistent", n, h, w, k, m, 3, 0) == 1
        assert H.call("smsut_conv2d_mfma_tiles", n, h, w, k, m, 3, 0) == (h // 8) * (w // 16)
    items = n * (h // 8) * (w // 16)
    if walk:
        assert_walk(items, co // 16, cus, walk == "tail")
        assert is_prime(n) and h // 8 > 1
    run_forms(H, n, h, w, ci, co, full_legs(ci, co) if legs == "full" else BASIC, splits=(16,) if ci == 32 else None)


# Kdim 8 (forward, statistics, fused shortcut: K8) and Ndim 8 (data-gradient plain, accumulate, fused shortcut: N8); the fused-shortcut
# data-gradient of [8 -> 16] reduces over 2 * 16 = 32 channels: <3,8,1,2,N8> with the shortcut's second half (launch_fwd_p, F_SC2 | F_N8)
#   (260,16,32,8->16)  units 1040; K8 on 16-row items, N8 <3,16,1,1,N8>      (130,24,48,8->16)  units 1170; 8-row items both ways
#   (260,16,32,8->32)  data-gradient Kdim 32 -> <3,8,1,2,N8>; no fused-shortcut data-gradient (co must be 16 for an 8-channel result)
K8N8 = [(260, 16, 32, 8, 16, ("fwd", "stats", "sc", "dgrad", "acc", "dsc")), (130, 24, 48, 8, 16, ("fwd", "stats", "sc", "dgrad", "acc", "dsc")),
        (260, 16, 32, 8, 32, ("fwd", "stats", "sc", "dgrad", "acc"))]


@pytest.mark.parametrize("case", K8N8, ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}" for c in K8N8])
def test_direct_persistent_8_channels(H, case):
    n, h, w, ci, co, legs = case
    assert ci == 8
    assert H.call("smsut_conv2d_mfma_form", n, h, w, ci, co, 0) == 0 and H.call("smsut_conv2d_mfma_persistent", n, h, w, ci, co, 3, 0) == 1
    th = 16 if h % 16 == 0 else 8                                                      # select_fwd_p: 16-row items when H % 16 == 0
    assert H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 0) == (h // th) * (w // 16)
    # the 8-channel result has no query (smsut_conv2d_mfma_persistent asks Ndim % 16 == 0): fwd_p_n8_eligible restated
    assert co in (16, 32) and w % 16 == 0 and h % 8 == 0 and n * (h // 8) * (w // 16) >= 1024
    assert H.call("smsut_conv2d_mfma_form", n, h, w, co, ci, 0) == 0 and H.call("smsut_conv2d_mfma_form", n, h, w, 2 * co, ci, 1) == 0
    run_forms(H, n, h, w, ci, co, legs)


def test_fused_shortcut_dgrad_at_64_channels_stays_direct(H):
    """sc2_64 (select_fwd_p, conv_mfma.hip): on a shape whose every other form is a Winograd kernel, the fused-shortcut data-gradient with
    2 Cout = 64 reduction channels runs the direct <3,8,1,4> form -- both against fp64"""
    n, h, w, ci, co = 257, 16, 16, 64, 32
    assert H.call("smsut_conv2d_mfma_form", n, h, w, 2 * co, ci, 1) == 0            # the fused-shortcut data-gradient: direct
    assert H.call("smsut_conv2d_mfma_form", n, h, w, 2 * co, ci, 0) == 2            # any other form of that (Kdim, Ndim): streamed Winograd
    assert H.call("smsut_conv2d_mfma_form", n, h, w, ci, co, 0) == 2 and H.call("smsut_conv2d_mfma_form", n, h, w, co, ci, 0) == 1
    assert units(n, h, w, ci) >= 1024                                              # fwd_p_eligible(.., 64, Cin): what sc2_64 asks
    run_forms(H, n, h, w, ci, co, ("fwd", "dgrad", "dsc", "dscsplit"), splits=(32, 16))


# smsut_conv2d_fwd_mfma_cfg (dispatch_fwd_cfg, conv_mfma.hip): the instantiations select_fwd_p can choose, at tiny shapes no 1024-unit rule
# guards -- 22 / 23 are the 16-row direct forms only SMSUT_WINOGRAD=0 selects.  cfg -> (TH, NTN, NCH); Kdim = 16 NCH, Ndim % (16 NTN) == 0.
CFGS = {20: (8, 1, 1), 21: (8, 1, 2), 22: (16, 1, 1), 23: (16, 1, 2), 25: (8, 2, 2), 28: (8, 1, 4), 30: (16, 1, 1), 31: (16, 1, 2)}


@pytest.mark.parametrize("cfg", list(CFGS), ids=[f"cfg{c}-th{v[0]}-ntn{v[1]}-nch{v[2]}" for c, v in CFGS.items()])
def test_forced_persistent_instantiations(H, cfg):
    th, ntn, nch = CFGS[cfg]
    n, h, w, c = 3, 3 * th, 32, 16 * nch                   # 3 x 2 items per image, non-square; [c -> c] so that both readings fit
    st = H.stream_ptr()
    for co in ((c,) if ntn == 2 else (c, 48)):             # (48: three 16-channel slabs, NTN = 1 only; forward only unless c == 48)
        R = refs_for(n, h, w, c, co, seed=40 + cfg)
        y, g1 = out_buf(n, h, w, co)
        H.call("smsut_conv2d_fwd_mfma_cfg", R.dev("x"), R.dev("wt"), y, n, h, w, c, co, 3, 0, cfg, st)
        check(f"cfg {cfg} fwd {c}->{co}", y, R.ref("y"), FWD_BAR)
        assert untouched(g1)
        if co != c:
            continue
        gx, g2 = out_buf(n, h, w, c)
        H.call("smsut_conv2d_fwd_mfma_cfg", R.dev("gy"), R.dev("wt"), gx, n, h, w, c, c, 3, 1, cfg, st)
        check(f"cfg {cfg} dgrad", gx, R.ref("gx"), FWD_BAR)
        acc, g3 = based_buf(R.cpu("base"))
        H.call("smsut_conv2d_fwd_mfma_cfg", R.dev("gy"), R.dev("wt"), acc, n, h, w, c, c, 3, 3, cfg, st)
        check(f"cfg {cfg} accumulate", acc, R.ref("gx+base"), FWD_BAR)
        assert untouched(g2, g3)


# ================================================================================================ 4. the per-tile kernel
def tile_branch(N, Hh, W, ndim, transposed):
    """dispatch_fwd<3> below the persistent kernels (its launch_fwd rows, conv_mfma.hip; isc = osc = G = ntap_out = 1, fp32): (TH, NTN, MW).  A
    restatement -- only TH and MW show in smsut_conv2d_mfma_tiles; edit together with those rows."""
    nt, tx = cdiv(ndim, 16), cdiv(W, 16)
    wg16 = tx * cdiv(Hh, 16) * N * ((nt + 1) // 2)
    wg8 = tx * cdiv(Hh, 8) * N * ((nt + 1) // 2)
    if Hh <= 8 and W <= 8 and Hh > 4:
        return (8, 1, 8)
    if Hh <= 4:
        return (4, 1, 16)
    if nt == 1:
        return (8, 1, 16)
    if wg16 >= 512:
        return (16, 2, 16)
    if wg8 >= 256 and not transposed:
        return (8, 2, 16)
    return (8, 1, 16)


# Columns: n, h, w, ci, co, legs, splits, (forward branch, data-gradient branch or None).  Kdim 4 / 12 / 20 / 40: a partial chunk, a
# partial second / third chunk; Ndim 1 / 5 (forward only: a data-gradient needs Kdim % 4 == 0) / 20 / 48: ragged 16-channel tiles.
#   (3,3,17,4->1)      4-row tile, H < 4, W = 16 + 1                     (3,4,33,12->20)   4-row tile, W = 32 + 1, both ways
#   (5,7,7,20->48)     the 8-pixel-wide tile on a ragged 7 x 7 plane       (3,8,8,64->32)    ... on the full 8 x 8 plane: cat, split 16 + 48
#   (3,13,31,40->5)    <8,.,1> by nt = 1, W = 32 - 1, H = 8 + 5            (3,13,15,12->16)  W < 16
#   (11,30,47,40->40)  forward wg8 = 3 * 4 * 11 * 2 = 264 >= 256, wg16 = 132 -> <8,.,2>; the data-gradient stays on <8,.,1>; split 16 + 24
#   (59,33,47,20->20)  wg16 = 3 * 3 * 59 * 1 = 531 -> <16,.,2> both ways, H = 32 + 1, W = 48 - 1
#   (29,33,47,12->48)  wg16 = 3 * 3 * 29 * 2 = 522 -> <16,.,2> with a ragged second 32-channel slab; data-gradient nt = 1
#   (3,13,31,64->20)   Kdim 64 (four chunks) on a ragged plane: cat 32 + 32; data-gradient Ndim 64 split 16 + 48
PER_TILE = [(3, 3, 17, 4, 1, ("fwd", "stats"), (), ((4, 1, 16), None)),
            (3, 4, 33, 12, 20, BASIC, (), ((4, 1, 16), (4, 1, 16))),
            (5, 7, 7, 20, 48, BASIC, (), ((8, 1, 8), (8, 1, 8))),
            (3, 8, 8, 64, 32, BASIC + ("cat", "split"), (16,), ((8, 1, 8), (8, 1, 8))),
            (3, 13, 31, 40, 5, ("fwd", "stats"), (), ((8, 1, 16), None)),
            (3, 13, 15, 12, 16, BASIC, (), ((8, 1, 16), (8, 1, 16))),
            (11, 30, 47, 40, 40, BASIC + ("split",), (16,), ((8, 2, 16), (8, 1, 16))),
            (59, 33, 47, 20, 20, BASIC, (), ((16, 2, 16), (16, 2, 16))),
            (29, 33, 47, 12, 48, BASIC, (), ((16, 2, 16), (8, 1, 16))),
            (3, 13, 31, 64, 20, BASIC + ("cat", "split"), (16,), ((8, 1, 16), (8, 1, 16)))]


def _pid(c):
    fb = c[7][0]
    return f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}-th{fb[0]}-ntn{fb[1]}-mw{fb[2]}"


@pytest.mark.parametrize("case", PER_TILE, ids=[_pid(c) for c in PER_TILE])
def test_per_tile_kernel(H, case):
    n, h, w, ci, co, legs, splits, (fb, db) = case
    assert n % 2 == 1
    assert tile_branch(n, h, w, co, False) == fb
    assert H.call("smsut_conv2d_mfma_persistent", n, h, w, ci, co, 3, 0) == 0 and H.call("smsut_conv2d_mfma_form", n, h, w, ci, co, 0) == 0
    assert H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, 0) == cdiv(h, fb[0]) * cdiv(w, fb[2])
    if db:
        assert tile_branch(n, h, w, ci, True) == db
        assert H.call("smsut_conv2d_mfma_persistent", n, h, w, co, ci, 3, 0) == 0
    else:
        assert not set(legs) & {"dgrad", "acc", "split"}
    run_forms(H, n, h, w, ci, co, legs, splits=splits)


def test_per_tile_table_is_covered():
    fwd, dgr = {c[7][0] for c in PER_TILE}, {c[7][1] for c in PER_TILE if c[7][1]}
    assert fwd == {(4, 1, 16), (8, 1, 8), (8, 1, 16), (8, 2, 16), (16, 2, 16)}
    assert dgr == {(4, 1, 16), (8, 1, 8), (8, 1, 16), (16, 2, 16)}                       # (<8,.,2> is forward-only: !c.transposed_w)
    assert {c[3] for c in PER_TILE} >= {4, 12, 20, 40, 64} and {c[4] for c in PER_TILE} >= {1, 5, 20, 48}
    assert {c[2] % 16 for c in PER_TILE} >= {1, 15} and any(c[2] < 16 for c in PER_TILE)


# ================================================================================================ 5. LDS weight gradients
def plan_wgrad(N, Hh, W, ci, co, rows=9):
    """plan_wgrad (conv_mfma_wgrad.hip): (cit, cot, splits, tiles_per_split, total tiles) on 8 x 16 pixel tiles"""
    cit, cot = (2 if ci > 16 else 1), (2 if co > 16 else 1)
    total = N * cdiv(W, 16) * cdiv(Hh, 8)
    slabs = cdiv(ci, 16 * cit) * cdiv(co, 16 * cot)
    want = cdiv(768 if cit == 1 and cot == 1 else 512, slabs)
    want = max(min(want, max((8 << 20) // (ci * co * 9), 1), total), 1)
    tps = cdiv(total, want)
    return cit, cot, cdiv(total, tps), tps, total


def wgrad_kernel(N, Hh, W, ci, co, aff):
    """wgrad_select once the register-row kernel has declined (below_rr; conv_mfma_wgrad.hip)"""
    if Hh * W <= 64 and W % 4 == 0 and ci % 32 == 0 and co % 32 == 0 and N * Hh * W <= 4096 and not aff:     # plane_wgrad_applies
        return "plane"
    cit, cot = (2 if ci > 16 else 1), (2 if co > 16 else 1)
    if cit == 2 and cot == 2 and Hh % 8 == 0 and W % 16 == 0 and ci % 32 == 0 and co % 32 == 0:
        return "ts"
    return f"lds{cit}x{cot}"


def sum_cols(wsize):
    """launch_sum_splits (conv_mfma_wgrad.hip)"""
    return 64 if wsize >= 32768 else (32 if wsize >= 8192 else 16)


def run_wgrad(H, n, h, w, ci, co, form="plain", ca=0, seed=50):
    """one 3x3 weight gradient through the LDS kernels against fp64; returns (kernel, cit, cot, splits, tiles_per_split, total)"""
    st = H.stream_ptr()
    cat, aff, sc = form == "cat", form == "inaff", form == "sc"
    assert H.call("smsut_conv2d_wgrad_mfma_supported", 3, 1, 1, ci, co) == 1
    # the register-row kernel's own predicate (plan_rr, conv_wgrad_rr.hip:372-387, does not look at N beyond N > 0)
    assert H.call("smsut_conv2d_wgrad_pair_supported", 1, 1, h, w, ci, co, int(cat), int(aff), int(sc)) == 0
    kern = wgrad_kernel(n, h, w, ci, co, aff)
    assert kern != "ts"
    rows = 10 if sc else 9
    cit, cot, splits, tps, total = plan_wgrad(n, h, w, ci, co)
    ws_n = H.call("smsut_conv2d_wgrad_sc_ws", n, h, w, ci, co) if sc else H.call("smsut_conv2d_wgrad_mfma_ws", n, h, w, ci, co, 3)
    assert ws_n == splits * rows * ci * co, "the workspace query must describe the plan this test derived"
    g = gen(seed)
    x, gy = rn(g, n, h, w, ci), rn(g, n, h, w, co)
    gw, gg = out_buf(rows, ci, co)
    ws, wg = poisoned(ws_n)
    xe = x
    if aff:
        mean, rstd = rn(g, n, ci, scale=0.2), 0.5 + torch.rand(n, ci, generator=g)
        gam, bet = 1 + 0.1 * rn(g, ci), 0.1 * rn(g, ci)
        xe = F.leaky_relu((x.double() - mean.double()[:, None, None]) * rstd.double()[:, None, None] * gam.double() + bet.double(), SLOPE)
        H.call("smsut_conv2d_wgrad_mfma_inaff", x.cuda(), gy.cuda(), gw, ws, mean.cuda(), rstd.cuda(), gam.cuda(), bet.cuda(), SLOPE,
               n, h, w, ci, co, st)
    elif cat:
        H.call("smsut_conv2d_wgrad_mfma_cat", x[..., :ca].contiguous().cuda(), x[..., ca:].contiguous().cuda(), ca, gy.cuda(), gw, ws,
               n, h, w, ci, co, 3, st)
    elif sc:
        assert H.call("smsut_conv2d_wgrad_sc_supported", n, h, w, ci, co) == 1
        gs = rn(g, n, h, w, co)
        H.call("smsut_conv2d_wgrad_mfma_sc", x.cuda(), None, 0, gy.cuda(), gs.cuda(), gw, ws, n, h, w, ci, co, st)
    else:
        H.call("smsut_conv2d_wgrad_mfma", x.cuda(), gy.cuda(), gw, ws, n, h, w, ci, co, 3, st)
    bar = WGRAD_BAR if n * h * w <= 100000 else WGRAD_BAR_BIG
    tag = f"wgrad {form} {n}x{h}x{w} {ci}->{co} {kern} splits {splits} x {tps} tiles (last {total - (splits - 1) * tps}) cols{sum_cols(rows * ci * co)}"
    check(tag, gw[:9].reshape(3, 3, ci, co), wgrad3_64(xe, gy).cuda(), bar)
    if sc:
        check(tag + " shortcut row", gw[9], (x.double().reshape(-1, ci).t() @ gs.double().reshape(-1, co)).cuda(), bar)
    if kern == "plane":
        assert bool(torch.isnan(ws[:ws_n]).all()), "plane_wgrad writes the final values: no split slabs"
    else:
        assert bool(torch.isfinite(ws[:ws_n]).all()), "every slab element of every split is written"
    assert untouched(gg, wg)
    return kern, cit, cot, splits, tps, total


# every (Cin, Cout) of {4, 12, 20, 40, 48} x {4, 20, 48} on a plane ragged both ways (H = 8 + 5, W = 32 - 1): all four (CIT, COT) slab
# shapes, partial first / second 16-channel tiles on either side; 12 tiles -> <= 12 one-tile splits
@pytest.mark.parametrize("co", [4, 20, 48])
@pytest.mark.parametrize("ci", [4, 12, 20, 40, 48])
def test_lds_wgrad_channel_tails(H, ci, co):
    kern, cit, cot, splits, tps, total = run_wgrad(H, 3, 13, 31, ci, co)
    assert kern == f"lds{1 + (ci > 16)}x{1 + (co > 16)}" and total == 12 and tps == 1


# more than one tile per split with a SHORT last split, per slab shape (plan arithmetic in plan_wgrad above):
#   (1,241,385,4->4)    1x1: 25 x 31 = 775 tiles, want 768 -> 2 per split, 388 splits, the last holds one tile; 92785 pixels
#   (7,81,100,4->20)    1x2 / (7,81,100,20->4) 2x1: 7 * 7 * 11 = 539 tiles, want 512 -> 2 per split, 270 splits, last one tile
#   (5,37,100,40->48)   2x2: 4 slabs -> want 128; 5 * 7 * 5 = 175 tiles -> 2 per split, 88 splits, last one tile
#   (5,37,100,48->76)   2x2, 6 slabs -> want 86 -> 3 per split, 59 splits, last one tile; 9 * 48 * 76 >= 32768: the 64-column sum
SHORT_LAST = [(1, 241, 385, 4, 4, (1, 1, 388, 2)), (7, 81, 100, 4, 20, (1, 2, 270, 2)), (7, 81, 100, 20, 4, (2, 1, 270, 2)),
              (5, 37, 100, 40, 48, (2, 2, 88, 2)), (5, 37, 100, 48, 76, (2, 2, 59, 3))]


@pytest.mark.parametrize("case", SHORT_LAST, ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}-cit{c[5][0]}cot{c[5][1]}-splits{c[5][2]}" for c in SHORT_LAST])
def test_lds_wgrad_short_last_split(H, case):
    n, h, w, ci, co, plan = case
    kern, cit, cot, splits, tps, total = run_wgrad(H, n, h, w, ci, co, seed=51)
    assert (cit, cot, splits, tps) == plan and kern == f"lds{cit}x{cot}"
    assert tps > 1 and total - (splits - 1) * tps == 1, "the last split must be short"


# sum_splits<16 | 32 | 64> by wsize = 9 Cin Cout on each side of 8192 and 32768 (launch_sum_splits, conv_mfma_wgrad.hip): 20x40 -> 7200 | 48x20 ->
# 8640 | 48x72 -> 31104 | 48x76 -> 32832; on 3x13x31 (<= 12 splits: the single-accumulator tail loop alone) and on 5x37x100 (175
# tiles: 175 / 175 / 59 / 59 splits, past 3 * 256 / COLS: the four-accumulator loop and its tail)
@pytest.mark.parametrize("plane", [(3, 13, 31), (5, 37, 100)], ids=["tail-loop", "4acc-loop"])
@pytest.mark.parametrize("ci,co,cols", [(20, 40, 16), (48, 20, 32), (48, 72, 32), (48, 76, 64)])
def test_lds_wgrad_sum_splits_widths(H, ci, co, cols, plane):
    assert sum_cols(9 * ci * co) == cols
    kern, cit, cot, splits, tps, total = run_wgrad(H, *plane, ci, co, seed=52)
    lanes = 256 // cols
    assert (splits > 3 * lanes) == (plane[0] == 5), "which loops of sum_splits a lane runs (c + 3 LANES < splits)"


# Cin == 8: the tap-pair form (C8) and with the fused shortcut (SC8), one and two 16-channel output tiles, ragged and full tiles
@pytest.mark.parametrize("form", ["plain", "sc"])
@pytest.mark.parametrize("n,h,w,co", [(3, 13, 31, 16), (5, 16, 32, 32), (3, 13, 31, 20)])
def test_lds_wgrad_8_input_channels(H, n, h, w, co, form):
    kern, *_ = run_wgrad(H, n, h, w, 8, co, form=form, seed=53)
    assert kern == f"lds1x{1 + (co > 16)}"


# virtual cat (ca % 16 == 0, (Cin - ca) % 4 == 0): 16 + 4 (CIT 2: the second tile is xb's one quad), 16 + 32, 32 + 16 on a ragged plane,
# and 32 + 32 on a plane the register-row kernel declines for H % 4 != 0 alone; input-side IN: 1x1, 2x2 ragged, and 2x2 on that plane
@pytest.mark.parametrize("n,h,w,ci,co,form,ca", [(3, 13, 31, 20, 20, "cat", 16), (3, 13, 31, 48, 48, "cat", 16), (3, 13, 31, 48, 12, "cat", 32),
                                                (3, 14, 32, 64, 32, "cat", 32), (3, 13, 31, 16, 16, "inaff", 0),
                                                (3, 13, 31, 20, 40, "inaff", 0), (3, 14, 32, 32, 32, "inaff", 0)])
def test_lds_wgrad_cat_and_input_side_instnorm(H, n, h, w, ci, co, form, ca):
    kern, cit, cot, *_ = run_wgrad(H, n, h, w, ci, co, form=form, ca=ca, seed=54)
    assert kern == f"lds{cit}x{cot}"


# plane_wgrad (plane_wgrad_applies, conv_mfma_wgrad.hip): H W <= 64, W % 4 == 0, channels % 32 == 0, N H W <= 4096.  Planes 1x4, 2x4,
# 4x8, 8x8 with odd N, plain and cat; N H W = 4096 exactly (64 x 8 x 8) and just past it (65 x 8 x 8 -> the 2x2 LDS kernel)
@pytest.mark.parametrize("form", ["plain", "cat"])
@pytest.mark.parametrize("n,h,w,ci,co,kernel", [(5, 1, 4, 32, 32, "plane"), (5, 2, 4, 64, 32, "plane"), (5, 4, 8, 32, 64, "plane"),
                                               (5, 8, 8, 32, 32, "plane"), (64, 8, 8, 32, 32, "plane"), (65, 8, 8, 32, 32, "lds2x2")])
def test_plane_wgrad(H, n, h, w, ci, co, kernel, form):
    if n >= 64:
        assert (n * h * w == 4096) == (kernel == "plane") and n * h * w <= 4096 + h * w
    kern, *_ = run_wgrad(H, n, h, w, ci, co, form=form, ca=16, seed=55)
    assert kern == kernel
