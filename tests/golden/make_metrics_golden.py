"""Writes tests/golden/metrics.npz: designed volumes for the test-phase metrics (connected-component cleanup, surface statistics,
ASSD, get_all_matrix) with their expected results, computed with NumPy + scipy only.

The reference (misc/utils.py:18-36, :206-283) uses skimage and medpy, which are not installed here.  This generator restates
them on two equivalences, so parity with those libraries is restated, not pinned (like ``binary_dc``):
  * ``skimage.measure.label(x, connectivity=2)`` labels the same components as ``scipy.ndimage.label`` with
    ``generate_binary_structure(x.ndim, 2)`` (18 neighbours in 3-D, 8 in 2-D);
  * medpy's surface distances with default arguments are ``distance_transform_edt(~border(reference))`` read at
    ``border(result)``, where ``border(m) = m ^ binary_erosion(m, generate_binary_structure(m.ndim, 1))`` (border value 0).

    python tests/golden/make_metrics_golden.py        # rewrites tests/golden/metrics.npz
"""
import os

import numpy as np
from scipy import ndimage as ndi

N_MODAL = 4          # config.py: n_modal (the cleanup's class bound) and n_label (the scored organs)
N_LABEL = 4
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics.npz")


def cc_ref(pred):
    """connected_components: keep components of class c = 1..N_MODAL larger than 0.1 * (voxels of class c)."""
    pred = np.asarray(pred)
    out = np.zeros(pred.shape, np.uint8)
    st = ndi.generate_binary_structure(pred.ndim, 2)
    for c in range(1, N_MODAL + 1):
        lab, nl = ndi.label(pred == c, structure=st)
        if nl == 0:
            continue
        sizes = np.bincount(lab.ravel())
        keep = sizes > 0.1 * float(np.count_nonzero(lab))
        keep[0] = False
        out[keep[lab]] = c
    return out


def cc_slices_ref(pred):
    return np.stack([cc_ref(s) for s in pred])


def border(m):
    return m ^ ndi.binary_erosion(m, structure=ndi.generate_binary_structure(m.ndim, 1), iterations=1)


def surface_distances(a, b):
    return ndi.distance_transform_edt(~border(b))[border(a)]


def stats_ref(p, g, n_cls=N_LABEL):
    """[n_cls, 7]: |P&G|, |P|, |G|, border(P), sum d(border P -> border G), border(G), sum d(border G -> border P);
    a distance sum is NaN when the other mask is empty."""
    rows = []
    for lab in range(1, n_cls + 1):
        P, G = p == lab, g == lab
        row = [np.count_nonzero(P & G), np.count_nonzero(P), np.count_nonzero(G)]
        for a, b in ((P, G), (G, P)):
            nb = np.count_nonzero(border(a))
            row += [nb, float(surface_distances(a, b).sum()) if a.any() and b.any() else np.nan]
        rows.append(row)
    return np.array(rows, dtype=np.float64)


def assd_ref(a, b):
    a, b = np.asarray(a).astype(bool), np.asarray(b).astype(bool)
    if not a.any() or not b.any():
        raise RuntimeError("empty mask")
    return 0.5 * (surface_distances(a, b).mean() + surface_distances(b, a).mean())


def dc_ref(a, b):
    den = np.count_nonzero(a) + np.count_nonzero(b)
    return 2.0 * np.count_nonzero(a & b) / float(den) if den else 0.0


def full_matrix(matrix, n):
    n = n.copy()
    n[n == 0] += 1e-8
    matrix = matrix / n
    full = np.zeros((N_MODAL + 1, N_LABEL + 1))
    full[:N_MODAL, :N_LABEL] = matrix
    full[-1, :] = np.mean(full[0:N_MODAL], axis=0)
    full[:, -1] = np.mean(full[:, 0:N_LABEL], axis=1)
    return full


MODALITIES = ("ct", "t1in", "t1out", "t2")


def get_all_matrix_ref(prd, gt):
    dcm, asm = np.zeros((N_MODAL, N_LABEL)), np.zeros((N_MODAL, N_LABEL))
    n = np.zeros((N_MODAL, 1))
    for k in gt:
        m = MODALITIES.index(k.split("_")[0])
        p1 = cc_slices_ref(cc_ref(prd[k]))
        g = gt[k]
        maxassd = 0
        for i in range(N_LABEL):
            P, G = p1 == i + 1, g == i + 1
            s = dc_ref(P, G)
            r = maxassd if not P.any() else assd_ref(P, G)
            maxassd = maxassd if maxassd > r else r
            dcm[m][i] += s
            asm[m][i] += r
        n[m] += 1
    return full_matrix(dcm, n), full_matrix(dcm, n), full_matrix(asm, n)


def blobs(seed, shape, n_cls=N_LABEL, sigma=3.0):
    """Smooth random label volume: the argmax of blurred noise fields, background where all are low."""
    rng = np.random.default_rng(seed)
    f = np.stack([ndi.gaussian_filter(rng.standard_normal(shape), sigma) for _ in range(n_cls + 1)])
    lab = np.argmax(f, axis=0).astype(np.uint8)
    return lab


def cases():
    c = {}
    # 90-voxel block + 12 voxels that touch each other and the block only at 3-D corners: the chain is 12 components of 1
    v = np.zeros((14, 18, 22), np.uint8)
    v[0:2, 0:5, 0:9] = 1
    for k in range(1, 13):
        v[1 + k, 4 + k, 8 + k] = 1
    c["corner_chain"] = v
    # the same chain stepping along edges (dz, dy): one 102-voxel component
    v = np.zeros((14, 18, 22), np.uint8)
    v[0:2, 0:5, 0:9] = 1
    for k in range(1, 13):
        v[1 + k, 4 + k, 8] = 1
    c["edge_chain"] = v
    # an in-plane diagonal chain off a 90-voxel block, on both slices: 8-connected per slice
    v = np.zeros((2, 24, 24), np.uint8)
    v[:, 0:9, 0:10] = 2
    for k in range(1, 13):
        v[:, 8 + k, 9 + k] = 2
    c["diagonal_chain"] = v
    # a column along z off a block on slice 0: one 3-D component of 12 (kept), per slice 12 separate voxels
    v = np.zeros((12, 16, 16), np.uint8)
    v[0, 0:9, 0:10] = 3
    v[:, 2, 14] = 3
    c["z_column"] = v
    # class 1: 90 + 10 voxels (F = 100, the 10 dropped); class 2: 89 + 11 (the 11 kept)
    v = np.zeros((3, 30, 30), np.uint8)
    v[0, 0:9, 0:10] = 1
    v[2, 20:22, 20:25] = 1
    v[0, 15:24, 0:10] = 2
    v[0, 15, 0] = 0
    v[2, 0, 19:30] = 2
    c["tenth"] = v
    # class 1: 90-voxel block + a 5-voxel piece, both touching a class-2 bridge: classes never merge, the piece is dropped
    v = np.zeros((1, 20, 30), np.uint8)
    v[0, 0:9, 0:10] = 1
    v[0, 0:4, 10:14] = 2
    v[0, 0:5, 14] = 1
    c["touching_classes"] = v
    # values above n_modal become 0
    v = np.zeros((2, 12, 12), np.uint8)
    v[0, 0:6, 0:6] = 5
    v[1, 2:8, 2:8] = 255
    v[0, 8:12, 8:12] = 4
    v[1, 0:2, 9:12] = 7
    c["above_n_modal"] = v
    c["empty"] = np.zeros((3, 9, 11), np.uint8)
    c["all_foreground"] = np.ones((4, 7, 9), np.uint8)
    v = np.zeros((1, 20, 20), np.uint8)
    v[0, 2:9, 3:15] = 1
    v[0, 12:18, 1:5] = 2
    v[0, 0, 19] = 2
    c["d1"] = v
    c["odd_5x37x53"] = blobs(11, (5, 37, 53))
    v = np.zeros((1, 5, 8), np.uint8)
    v[0, 2, 2] = 1
    c["pair3"] = v
    c["blobs_a"] = blobs(1, (8, 48, 48))
    c["blobs_b"] = blobs(2, (6, 40, 56), sigma=2.0)
    return c


def gt_for(name, p):
    """Ground truth paired with a case: the blob cases against another seed, pair3 against a voxel 3 away, the rest against a
    shifted copy (np.roll along y) so that the distances are non-trivial."""
    if name == "pair3":
        g = np.zeros_like(p)
        g[0, 2, 5] = 1
        return g
    if name.startswith("blobs") or name.startswith("odd"):
        return blobs(100 + sum(map(ord, name)), p.shape)
    return np.roll(p, 1, axis=1)


def matrix_sets():
    """get_all_matrix inputs: volumes of all four modalities (two of ct), one of them covering the maxassd rule."""
    prd, gt = {}, {}
    shapes = {"ct_000": (6, 40, 40), "ct_001": (5, 32, 48), "t1in_002": (4, 40, 40), "t1out_003": (6, 36, 36), "t2_004": (3, 40, 44)}
    for i, (k, shp) in enumerate(shapes.items()):
        g = blobs(200 + i, shp)
        p = g.copy()
        p[:, ::7, :] = blobs(300 + i, shp)[:, ::7, :]          # a perturbed prediction with small stray pieces
        prd[k], gt[k] = p, g
    # maxassd: label 1 absent from the prediction (r = 0), label 3 absent too (r = max of labels 1..2)
    g = blobs(400, (4, 40, 40))
    p = g.copy()
    p[p == 1] = 0
    p[p == 3] = 0
    prd["t1in_005"], gt["t1in_005"] = p, g
    return prd, gt


def build():
    out = {}
    cs = cases()
    out["names"] = np.array(sorted(cs))
    for name, p in cs.items():
        g = gt_for(name, p)
        out[f"p_{name}"] = p
        out[f"g_{name}"] = g
        out[f"cc3_{name}"] = cc_ref(p)
        out[f"ccs_{name}"] = cc_slices_ref(p)
        out[f"st_{name}"] = stats_ref(p, g)
    prd, gt = matrix_sets()
    out["gam_keys"] = np.array(list(gt))
    for k in gt:
        out[f"gam_p_{k}"] = prd[k]
        out[f"gam_g_{k}"] = gt[k]
    dcm, hdm, asm = get_all_matrix_ref(prd, gt)
    out["gam_dc"], out["gam_hd"], out["gam_assd"] = dcm, hdm, asm
    out["pair3_assd"] = np.float64(assd_ref(cs["pair3"], gt_for("pair3", cs["pair3"])))
    return out


if __name__ == "__main__":
    data = build()
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes,", len(data), "arrays")
