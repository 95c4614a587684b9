"""Writes tests/golden/hausdorff.npz: expected Hausdorff / HD95 ingredients for every volume of metrics.npz and for designed
cases that aim at the radix select of csrc/metrics.hip (smsut_surface_hd), computed with NumPy + scipy only.

medpy is not installed here; its surface distances are restated as in make_metrics_golden.py:
``distance_transform_edt(~border(reference))[border(result)]``.  The squared distances are integers, stored as ``rint(d * d)``
(``sqrt(float64(rint(d * d)))`` gives scipy's value back bit for bit on every case here; ``build`` asserts it).

Per case ``c`` (labels 1..4):
  hd6_c   [4, 6]  n_pg, n_gp, max2_pg, max2_gp, lo2, hi2 with lo = floor((n - 1) * 0.95) in float64, hi = min(lo + 1, n - 1);
                  the four distance entries are -1 when either mask is empty
  hd_c    [4]     max of all distances (NaN when either mask is empty)
  hd95_c  [4]     numpy.percentile(pooled distances, 95) (NaN likewise)
The designed cases also carry their volumes (p_c, g_c); the others' are in metrics.npz.  hdm_hd / hdm_hd95 are the two
matrices of get_hd_matrix over make_metrics_golden.matrix_sets().

    python tests/golden/make_hausdorff_golden.py        # rewrites tests/golden/hausdorff.npz
"""
import importlib.util
import os

import numpy as np
from scipy import ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "hausdorff.npz")
Q = 0.95

_spec = importlib.util.spec_from_file_location("make_metrics_golden", os.path.join(HERE, "make_metrics_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)
N_MODAL, N_LABEL = mg.N_MODAL, mg.N_LABEL


def surface_distances(a, b):
    return ndi.distance_transform_edt(~mg.border(b))[mg.border(a)]


def squared(d):
    d2 = np.rint(d * d).astype(np.int64)
    assert np.array_equal(np.sqrt(d2.astype(np.float64)), d), "the integer restatement must lose nothing"
    return d2


def hd_row(P, G, q=Q):
    """(six integers, hd, percentile) of one pair of masks."""
    n_pg, n_gp = int(np.count_nonzero(mg.border(P))), int(np.count_nonzero(mg.border(G)))
    if not P.any() or not G.any():
        return [n_pg, n_gp, -1, -1, -1, -1], np.nan, np.nan
    d_pg, d_gp = surface_distances(P, G), surface_distances(G, P)
    s_pg, s_gp = squared(d_pg), squared(d_gp)
    assert len(s_pg) == n_pg and len(s_gp) == n_gp
    pool = np.sort(np.hstack((s_pg, s_gp)))
    n = len(pool)
    lo = int(np.floor(np.float64(n - 1) * np.float64(q)))
    hi = min(lo + 1, n - 1)
    six = [n_pg, n_gp, int(s_pg.max()), int(s_gp.max()), int(pool[lo]), int(pool[hi])]
    return six, float(max(d_pg.max(), d_gp.max())), float(np.percentile(np.hstack((d_pg, d_gp)), 100.0 * q))


def hd_case(p, g, n_cls=N_LABEL):
    rows = [hd_row(p == lab, g == lab) for lab in range(1, n_cls + 1)]
    return (np.array([r[0] for r in rows], dtype=np.float64), np.array([r[1] for r in rows], dtype=np.float64),
            np.array([r[2] for r in rows], dtype=np.float64))


def designed():
    """name -> (prediction, ground truth); label 1 unless said otherwise.  The 2-D ones are planar images (D = 1 with the
    4-neighbour border: no z neighbours at all), as ``hd`` / ``hd95`` get them from 2-D masks."""
    c = {}
    # d^2 = 1 + 160^2 = 25601 >= 2^13: the value lies above the first bucket of the first level
    p, g = np.zeros((8, 200), np.uint8), np.zeros((8, 200), np.uint8)
    p[3, 10] = 1
    g[4, 170] = 1
    c["far_pair"] = (p, g)
    # pool {0, 0, 16389}: rank lo in bucket 0, rank hi in bucket 2
    p, g = np.zeros((3, 4, 140), np.uint8), np.zeros((3, 4, 140), np.uint8)
    p[1, 1, 2] = 1
    g[1, 1, 2] = 1
    g[0, 3, 130] = 1
    c["straddle"] = (p, g)
    # every d^2 in 8192..16383 with distinct low bits: second-level selection inside a high bucket
    p, g = np.zeros((20, 120), np.uint8), np.zeros((20, 120), np.uint8)
    p[:, 0] = 1
    for y in range(20):
        g[y, 95 + y] = 1
    c["slant"] = (p, g)
    # d^2 = 4095^2: the top of the per-axis range
    p, g = np.zeros((2, 4096), np.uint8), np.zeros((2, 4096), np.uint8)
    p[0, 0] = 1
    g[0, 4095] = 1
    c["long_line"] = (p, g)
    # the directed maxima differ: 25 from the centre to the square's border, 50 from its corners to the centre
    p, g = np.zeros((15, 15), np.uint8), np.zeros((15, 15), np.uint8)
    g[2:13, 2:13] = 1
    p[7, 7] = 1
    c["nested"] = (p, g)
    # label 2 only in the prediction, label 3 only in the ground truth, label 1 in both
    p, g = np.zeros((2, 10, 12), np.uint8), np.zeros((2, 10, 12), np.uint8)
    p[:, 1:4, 1:5] = 1
    g[:, 2:5, 2:6] = 1
    p[0, 6:9, 7:10] = 2
    g[1, 6:9, 1:4] = 3
    c["one_sided"] = (p, g)
    return c


def get_hd_matrix_ref(prd, gt):
    hdm, h95m = np.zeros((N_MODAL, N_LABEL)), np.zeros((N_MODAL, N_LABEL))
    n = np.zeros((N_MODAL, 1))
    for k in gt:
        m = mg.MODALITIES.index(k.split("_")[0])
        p1 = mg.cc_slices_ref(mg.cc_ref(prd[k]))
        g = gt[k]
        maxhd, maxhd95 = 0, 0
        for i in range(N_LABEL):
            P, G = p1 == i + 1, g == i + 1
            if not P.any():
                h, h95 = maxhd, maxhd95
            elif not G.any():
                raise RuntimeError("empty ground truth")
            else:
                _, h, h95 = hd_row(P, G)
            maxhd = maxhd if maxhd > h else h
            maxhd95 = maxhd95 if maxhd95 > h95 else h95
            hdm[m][i] += h
            h95m[m][i] += h95
        n[m] += 1
    return mg.full_matrix(hdm, n), mg.full_matrix(h95m, n)


def build():
    out = {}
    base = np.load(os.path.join(HERE, "metrics.npz"), allow_pickle=False)
    vols = {str(nm): (base[f"p_{nm}"], base[f"g_{nm}"]) for nm in base["names"]}
    own = designed()
    out["names"] = np.array(sorted(vols) + sorted(own))
    out["own"] = np.array(sorted(own))
    for name, (p, g) in own.items():
        out[f"p_{name}"], out[f"g_{name}"] = p, g
    for name, (p, g) in {**vols, **own}.items():
        out[f"hd6_{name}"], out[f"hd_{name}"], out[f"hd95_{name}"] = hd_case(p, g)
    prd, gt = mg.matrix_sets()
    out["hdm_hd"], out["hdm_hd95"] = get_hd_matrix_ref(prd, gt)
    return out


if __name__ == "__main__":
    data = build()
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes,", len(data), "arrays")
