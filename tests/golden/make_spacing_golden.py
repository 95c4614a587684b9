"""Writes tests/golden/spacing.npz: expected surface statistics, Hausdorff / HD95 ingredients and test-phase matrices under an
anisotropic voxel spacing (smsut_surface_stats_sp / smsut_surface_hd_sp of csrc/metrics.hip), computed with NumPy + scipy only.

medpy is not installed here; its surface distances with ``voxelspacing=sp`` are restated as in make_metrics_golden.py:
``distance_transform_edt(~border(reference), sampling=sp)[border(result)]``.

Volumes of metrics.npz / hausdorff.npz are used by name and not stored again; only the designed ones of ``designed()`` are
(p_c, g_c).  ``runs`` lists the (case, spacing) pairs as rows "case s" with s an index into ``spacings`` ([k, 3]; a 2-D case
takes the last two entries).  Per pair, with the key suffix ``_{case}_s{s}`` and labels 1..4:
  st    [4, 7]  the surface_stats row: |P&G|, |P|, |G|, border(P), sum d(P -> G), border(G), sum d(G -> P) (NaN sums when the other
                mask is empty)
  hd6   [4, 6]  n_pg, n_gp, the two directed maxima, and the pooled order statistics at ranks lo = floor((n - 1) * 0.95) (fp64)
                and hi = min(lo + 1, n - 1) -- all four as DISTANCES from scipy; -1 when either mask is empty
  hd2r  [4, 4]  the same four as SQUARED distances from ``restated``: the device's expression, evaluated in NumPy (-1 likewise)
  hd    [4]     max of all distances;  hd95 [4]  numpy.percentile(pooled distances, 95) (NaN when either mask is empty)

``restated`` is the kernels' arithmetic: w = s * s per axis once, then fl(fl(fl(wx * dx^2) + fl(wy * dy^2)) + fl(wz * dz^2))
minimised over the other border.  Rounding is monotone, so the minimum of the separable passes is the minimum of that expression
over all border voxels: the device's squared distances equal these bit for bit, and the designed select cases are asserted on
them.  ``build`` also asserts that scipy's distances and the square roots of the restated ones differ by less than 1e-15
relative, the ground of the 1e-14 / 1e-13 bars of tests/test_surface_spacing_gpu.py.

spm_*: get_all_matrix / get_hd_matrix over make_metrics_golden.matrix_sets() under the mapping spm_keys -> spm_vals (a
modality name or a volume's own key, which wins).

    python tests/golden/make_spacing_golden.py        # rewrites tests/golden/spacing.npz
"""
import importlib.util
import os

import numpy as np
from scipy import ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "spacing.npz")
Q = 0.95

_spec = importlib.util.spec_from_file_location("make_metrics_golden", os.path.join(HERE, "make_metrics_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)
N_MODAL, N_LABEL = mg.N_MODAL, mg.N_LABEL

SPACINGS = [(1.0, 1.0, 1.0), (5.0, 1.25, 0.7), (0.7, 1.25, 5.0),                       # 0..2: the axis-order case
            (2.5, 0.78125, 0.78125), (1e-3, 3e-3, 7e-4), (1234.5, 999.9, 1000.0),      # 1, 3..5: parity
            (3.0, 0.9, 1.1),                                                           # 6: the select cases
            (2.0, 0.5, 1.5)]                                                           # 7: long lines
PARITY = ("blobs_a", "blobs_b", "odd_5x37x53", "z_column", "empty", "one_sided")
SELECT = ("sel_same", "sel_next", "straddle", "far_pair", "sel_zero")
LONG = ("long_2x600", "long_5x37x300")
RUNS = ([("axis_order", s) for s in (0, 1, 2)] + [(c, s) for c in PARITY for s in (1, 3, 4, 5)] + [(c, 6) for c in SELECT] +
        [(c, 7) for c in LONG])
MATRIX_SPACINGS = {"ct": (2.5, 0.8, 0.8), "ct_001": (3.0, 0.7, 0.7), "t1in": (5.0, 1.25, 1.25), "t1out": (5.5, 1.3, 1.3),
                   "t2": (7.7, 1.4, 1.4)}


def spacing_of(s, ndim):
    return SPACINGS[s][3 - ndim:]


def surface_distances(a, b, sp):
    return ndi.distance_transform_edt(~mg.border(b), sampling=sp)[mg.border(a)]


def restated(a, b, sp):
    """The device's squared distances from border(a) to border(b), in the order of ``surface_distances``."""
    pa, pb = np.argwhere(mg.border(a)).astype(np.float64), np.argwhere(mg.border(b)).astype(np.float64)
    w = [np.float64(s) * np.float64(s) for s in sp]
    pa, pb = np.ascontiguousarray(pa.T), np.ascontiguousarray(pb.T)
    out = np.empty(pa.shape[1], np.float64)
    for i0 in range(0, len(out), 256):
        acc = None
        for ax in range(a.ndim - 1, -1, -1):                      # x, then y, then z: the order of the passes
            term = w[ax] * np.square(pa[ax, i0:i0 + 256, None] - pb[ax, None, :])
            acc = term if acc is None else acc + term
        out[i0:i0 + 256] = acc.min(axis=1)
    return out


def ranks(n, q=Q):
    lo = int(np.floor(np.float64(n - 1) * np.float64(q)))
    return lo, min(lo + 1, n - 1)


def rows(p, g, sp, n_cls=N_LABEL):
    st, hd6, hd2r, hd, hd95 = [], [], [], [], []
    for lab in range(1, n_cls + 1):
        P, G = p == lab, g == lab
        n_pg, n_gp = int(np.count_nonzero(mg.border(P))), int(np.count_nonzero(mg.border(G)))
        row = [np.count_nonzero(P & G), np.count_nonzero(P), np.count_nonzero(G)]
        if not P.any() or not G.any():
            st.append(row + [n_pg, np.nan, n_gp, np.nan])
            hd6.append([n_pg, n_gp, -1, -1, -1, -1])
            hd2r.append([-1, -1, -1, -1])
            hd.append(np.nan)
            hd95.append(np.nan)
            continue
        d_pg, d_gp = surface_distances(P, G, sp), surface_distances(G, P, sp)
        r_pg, r_gp = restated(P, G, sp), restated(G, P, sp)
        for d, r in ((d_pg, r_pg), (d_gp, r_gp)):
            assert len(d) == len(r) and np.all(np.abs(np.sqrt(r) - d) <= 1e-15 * d), "scipy and the restated passes disagree"
        st.append(row + [n_pg, float(d_pg.sum()), n_gp, float(d_gp.sum())])
        pool, pool_r = np.sort(np.hstack((d_pg, d_gp))), np.sort(np.hstack((r_pg, r_gp)))
        lo, hi = ranks(len(pool))
        hd6.append([n_pg, n_gp, d_pg.max(), d_gp.max(), pool[lo], pool[hi]])
        hd2r.append([r_pg.max(), r_gp.max(), pool_r[lo], pool_r[hi]])
        hd.append(max(d_pg.max(), d_gp.max()))
        hd95.append(np.percentile(np.hstack((d_pg, d_gp)), 100.0 * Q))
    return tuple(np.array(v, dtype=np.float64) for v in (st, hd6, hd2r, hd, hd95))


def designed():
    """name -> (prediction, ground truth), label 1 unless said otherwise; the 2-D ones are planar images."""
    c = {}
    # P = one voxel, G = one voxel two slices up and one six columns along: which is nearer depends on the axes' weights
    p, g = np.zeros((3, 2, 8), np.uint8), np.zeros((3, 2, 8), np.uint8)
    p[0, 0, 0] = 1
    g[2, 0, 0] = 1
    g[0, 0, 6] = 1
    c["axis_order"] = (p, g)
    # two rows of 20 three lines apart and one shared voxel far off: the pool is {0, 0} and 40 equal values; ranks lo and hi lie
    # in the middle of those 40
    p, g = np.zeros((8, 70), np.uint8), np.zeros((8, 70), np.uint8)
    p[2, 0:20] = 1
    g[5, 0:20] = 1
    p[4, 65] = 1
    g[4, 65] = 1
    c["sel_same"] = (p, g)
    # one voxel against two, 11 rows down and 9 columns along: at (sy, sx) = (0.9, 1.1) both lie 9.9 away on paper, 0.81 * 121
    # = 1.21 * 81; in fp64 the two products differ in their last bits.  The pool is {v, v, v'}: rank lo is the last v, rank hi the
    # next value up
    p, g = np.zeros((2, 14, 12), np.uint8), np.zeros((2, 14, 12), np.uint8)
    p[0, 1, 1] = 1
    g[0, 12, 1] = 1
    g[0, 1, 10] = 1
    c["sel_next"] = (p, g)
    # identical masks: every distance is 0, every key is 0
    v = np.zeros((4, 12, 12), np.uint8)
    v[1:3, 2:9, 3:10] = 1
    v[0, 0:3, 0:2] = 2
    c["sel_zero"] = (v, v.copy())
    # lines longer than a block: 600 and 300 entries (300 is no multiple of 64), few border voxels
    p, g = np.zeros((2, 600), np.uint8), np.zeros((2, 600), np.uint8)
    p[0, 3] = p[1, 590] = p[1, 310] = 1
    g[1, 20] = g[0, 300] = g[0, 599] = 1
    c["long_2x600"] = (p, g)
    rng = np.random.default_rng(5)
    p, g = np.zeros((5, 37, 300), np.uint8), np.zeros((5, 37, 300), np.uint8)
    for vol in (p, g):
        for lab in (1, 2, 3):
            idx = rng.integers(0, vol.size, size=25)
            vol.reshape(-1)[idx] = lab
    c["long_5x37x300"] = (p, g)
    return c


def volumes():
    """name -> (p, g) for every case of RUNS; the second value: the names of the designed ones."""
    own = designed()
    mx = np.load(os.path.join(HERE, "metrics.npz"), allow_pickle=False)
    hx = np.load(os.path.join(HERE, "hausdorff.npz"), allow_pickle=False)
    hx_own = {str(n) for n in hx["own"]}
    vols = dict(own)
    for name in sorted({c for c, _ in RUNS} - set(own)):
        src = hx if name in hx_own else mx
        vols[name] = (src[f"p_{name}"], src[f"g_{name}"])
    return vols, sorted(own)


def assert_designed(out):
    """The designed cases say what they were built to say, on the restated (device) values."""
    ax = [out[f"hd6_axis_order_s{s}"][0] for s in (0, 1, 2)]
    assert ax[0][2] == 2.0 and abs(ax[1][2] - 4.2) < 1e-14 and abs(ax[2][2] - 1.4) < 1e-14
    r = out["hd2r_sel_same_s6"][0]
    n = int(out["hd6_sel_same_s6"][0, :2].sum())
    lo, hi = ranks(n)
    assert n == 42 and 2 < lo < hi < n - 1 and r[2] == r[3] == r[0] == r[1] == np.float64(0.9) * np.float64(0.9) * 9.0
    r = out["hd2r_sel_next_s6"][0]
    assert out["hd6_sel_next_s6"][0, :2].tolist() == [1, 2] and ranks(3) == (1, 2)
    assert r[0] == r[2] < r[3] == r[1] and (r[3] - r[2]) < 1e-14 * r[2]          # neighbours in the last mantissa bits
    assert r[2].view(np.int64) >> 12 == r[3].view(np.int64) >> 12                # apart only in the select's last level
    r = out["hd2r_straddle_s6"][0]
    assert r[2] == 0.0 and r[3] > 1e4 and out["hd6_straddle_s6"][0, :2].tolist() == [1, 2]
    assert out["hd6_far_pair_s6"][0, :2].tolist() == [1, 1] and len(set(out["hd2r_far_pair_s6"][0].tolist())) == 1
    z = out["hd2r_sel_zero_s6"]
    assert (z[:2] == 0.0).all() and (z[2:] == -1).all() and (out["hd6_sel_zero_s6"][:2, :2] > 0).all()
    for c in LONG:
        assert (out[f"hd6_{c}_s7"][0, 2:] > 0).all()


def matrices(prd, gt, spacings):
    """get_all_matrix's ASSD matrix and get_hd_matrix's two under a per-volume spacing."""
    asm, hdm, h95m = (np.zeros((N_MODAL, N_LABEL)) for _ in range(3))
    n = np.zeros((N_MODAL, 1))
    for k in gt:
        modality = k.split("_")[0]
        sp = spacings[k] if k in spacings else spacings[modality]
        m = mg.MODALITIES.index(modality)
        p1 = mg.cc_slices_ref(mg.cc_ref(prd[k]))
        mx = [0, 0, 0]
        for i in range(N_LABEL):
            P, G = p1 == i + 1, gt[k] == i + 1
            if not P.any():
                v = list(mx)
            else:
                d_pg, d_gp = surface_distances(P, G, sp), surface_distances(G, P, sp)
                pool = np.hstack((d_pg, d_gp))
                v = [0.5 * (d_pg.mean() + d_gp.mean()), pool.max(), np.percentile(pool, 100.0 * Q)]
            mx = [a if a > b else b for a, b in zip(mx, v)]
            asm[m][i] += v[0]
            hdm[m][i] += v[1]
            h95m[m][i] += v[2]
        n[m] += 1
    return mg.full_matrix(asm, n), mg.full_matrix(hdm, n), mg.full_matrix(h95m, n)


def build():
    out = {}
    vols, own = volumes()
    out["own"] = np.array(own)
    out["spacings"] = np.array(SPACINGS, dtype=np.float64)
    out["runs"] = np.array([f"{c} {s}" for c, s in RUNS])
    for name in own:
        out[f"p_{name}"], out[f"g_{name}"] = vols[name]
    for c, s in RUNS:
        p, g = vols[c]
        for kind, v in zip(("st", "hd6", "hd2r", "hd", "hd95"), rows(p, g, spacing_of(s, p.ndim))):
            out[f"{kind}_{c}_s{s}"] = v
    assert_designed(out)
    prd, gt = mg.matrix_sets()
    out["spm_keys"] = np.array(list(MATRIX_SPACINGS))
    out["spm_vals"] = np.array(list(MATRIX_SPACINGS.values()), dtype=np.float64)
    out["spm_assd"], out["spm_hd"], out["spm_hd95"] = matrices(prd, gt, MATRIX_SPACINGS)
    return out


if __name__ == "__main__":
    data = build()
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes,", len(data), "arrays")
