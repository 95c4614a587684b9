"""References of the dual-task-consistency path (csrc/dtc.hip, network/dtc.py, trainer/dtcTrainer.py): an exact integer Euclidean
distance transform in numpy (separable, plus brute force for tiny shapes), the fp64 signed distance map with the project's rules, an
fp64 torch restatement of the two loss terms, the case builders of the GPU tests, and the shared description of the scenarios of
tests/golden/dtc.npz (used by the generator, the CPU test and the GPU test).  Test infrastructure only.

Definitions.  For a class c of a label slice, P = (label == c).  ``d2`` of a pixel = the exact squared Euclidean distance to the nearest
pixel whose membership in P differs from its own (members: scipy's ``distance_transform_edt(P) ** 2``; non-members:
``distance_transform_edt(~P) ** 2``); outside the image is nothing; 0 everywhere where P is empty or full.  ``sdf`` =
+sqrt(d2) / sqrt(max d2 over non-members) on non-members, -sqrt(d2) / sqrt(max d2 over members) on members, exactly 0 on the inner
boundary (members with d2 == 1), exactly +1 where P is empty and -1 where P is full."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import recipe

BIG = 1 << 28


# ------------------------------------------------------------------------------------------- distance transform
def _row_dist(src):
    """src bool [..., W] -> int64 [..., W]: distance along the last axis to the nearest True, BIG where the row has none."""
    w = src.shape[-1]
    idx = np.arange(w)
    left = np.where(src, idx, -BIG)
    left = np.maximum.accumulate(left, axis=-1)                       # nearest True at or before x
    right = np.where(src, idx, BIG)
    right = np.minimum.accumulate(right[..., ::-1], axis=-1)[..., ::-1]
    return np.minimum(np.minimum(idx - left, right - idx), BIG)


def _dist_sq_to(src):
    """src bool [..., H, W] -> int64: squared Euclidean distance to the nearest True pixel (>= BIG where there is none): row distances,
    then the lower envelope min over y' of g(y')^2 + (y - y')^2 by brute force over y'."""
    g = _row_dist(src).astype(np.int64)
    g2 = np.minimum(g * g, BIG)
    h = src.shape[-2]
    out = np.full(src.shape, 4 * BIG, dtype=np.int64)
    for dy in range(-(h - 1), h):                                     # out[y] = min over y' = y + dy
        lo, hi = max(0, -dy), min(h, h - dy)
        if lo >= hi:
            continue
        cand = g2[..., lo + dy:hi + dy, :] + dy * dy
        out[..., lo:hi, :] = np.minimum(out[..., lo:hi, :], cand)
    return out


def edt_sq_masks(p):
    """p bool [..., H, W] -> int32 d2 of the definition above (one transform per sign, separable)."""
    p = np.asarray(p, dtype=bool)
    to_non, to_mem = _dist_sq_to(~p), _dist_sq_to(p)
    d2 = np.where(p, to_non, to_mem)
    d2[d2 >= BIG] = 0
    return d2.astype(np.int32)


def edt_sq_brute(p):
    """The same by brute force over all pixel pairs of one small image [H, W]."""
    p = np.asarray(p, dtype=bool)
    h, w = p.shape
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((h, w), dtype=np.int32)
    for y in range(h):
        for x in range(w):
            other = p != p[y, x]
            if other.any():
                out[y, x] = ((yy[other] - y) ** 2 + (xx[other] - x) ** 2).min()
    return out


def class_masks(labels, n_classes):
    labels = np.asarray(labels)
    return np.stack([labels == c for c in range(n_classes)], axis=1)             # [B, C, H, W]


def edt_sq(labels, n_classes):
    """int labels [B, H, W] -> int32 [B, C, H, W]"""
    return edt_sq_masks(class_masks(labels, n_classes))


def sdf_from(d2, p):
    """fp64 signed distance map from d2 and the membership p (same shape, [..., H, W])."""
    d2 = np.asarray(d2, dtype=np.float64)
    p = np.asarray(p, dtype=bool)
    mx_mem = np.where(p, d2, 0).max(axis=(-2, -1), keepdims=True)
    mx_non = np.where(~p, d2, 0).max(axis=(-2, -1), keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        neg = -np.sqrt(d2) / np.sqrt(mx_mem)
        pos = np.sqrt(d2) / np.sqrt(mx_non)
    out = np.where(p, neg, pos)
    out[p & (d2 == 1)] = 0.0                                          # the inner boundary
    flat = d2.max(axis=(-2, -1), keepdims=True) == 0                  # P empty or full
    out = np.where(flat, np.where(p, -1.0, 1.0), out)
    return out


def sdf(labels, n_classes):
    """(d2 int32, sdf fp64), both [B, C, H, W]"""
    p = class_masks(labels, n_classes)
    d2 = edt_sq_masks(p)
    return d2, sdf_from(d2, p)


def inner_boundary_morph(p):
    """Members whose 4-neighbourhood (reflecting edges) holds a non-member: dilation != erosion restricted to the members, the restatement
    of skimage's find_boundaries(mode='inner') with its default connectivity."""
    p = np.asarray(p, dtype=bool)
    q = np.pad(p, 1, mode="edge")
    er = q[1:-1, 1:-1] & q[:-2, 1:-1] & q[2:, 1:-1] & q[1:-1, :-2] & q[1:-1, 2:]
    di = q[1:-1, 1:-1] | q[:-2, 1:-1] | q[2:, 1:-1] | q[1:-1, :-2] | q[1:-1, 2:]
    return (di != er) & p


# ------------------------------------------------------------------------------------------- loss
def dtc_loss(t, z, sdf_t, k):
    """[mean((t[:B] - sdf)^2), mean((sigmoid(-k t) - softmax(z, 1))^2)] in the dtype of the inputs."""
    b = sdf_t.shape[0]
    l_sdf = ((t[:b] - sdf_t) ** 2).mean()
    l_cons = ((torch.sigmoid(-k * t) - torch.softmax(z, dim=1)) ** 2).mean()
    return torch.stack([l_sdf, l_cons])


# ------------------------------------------------------------------------------------------- case builders
EDT_SHAPES = [(2, 3, 1, 1), (1, 2, 1, 37), (1, 2, 37, 1), (3, 5, 17, 19), (2, 5, 64, 64), (1, 3, 65, 130), (1, 2, 256, 256),
              (1, 2, 512, 300)]                                        # (B, C, H, W)
LOSS_SHAPES = [(2, 1, 2, 24, 40), (4, 2, 5, 17, 19), (16, 8, 5, 64, 64), (3, 3, 1, 8, 8), (2, 1, 5, 256, 256)]     # (N, B, C, H, W)
PATTERNS = ("blobs", "checker", "corner", "half", "edges", "absent")


def label_pattern(name, b, c, h, w, seed=0):
    """int64 labels [b, h, w] with values in [0, c)."""
    rs = np.random.RandomState(seed + 17 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "blobs":                                               # random blobs: thresholded coarse noise, upsampled
        bh, bw = max(h // 6, 1), max(w // 6, 1)
        small = rs.randint(0, c, size=(b, bh, bw))
        lab = small[:, (yy * bh // h), (xx * bw // w)]
        flip = rs.uniform(size=(b, h, w)) < 0.03                      # and a few isolated pixels
        lab = np.where(flip, rs.randint(0, c, size=(b, h, w)), lab)
    elif name == "checker":                                           # every d2 = 1 (classes 0 and 1)
        lab = np.broadcast_to((yy + xx) % min(c, 2), (b, h, w)).copy()
    elif name == "corner":                                            # one member pixel in a corner: the search spans the column
        lab = np.zeros((b, h, w), dtype=np.int64)
        lab[:, h - 1, w - 1] = c - 1
        if b > 1:
            lab[1:] = 0
            lab[1:, 0, 0] = c - 1
    elif name == "half":                                              # a half plane: ties
        lab = np.broadcast_to(np.where(xx >= w // 2, c - 1, 0), (b, h, w)).copy()
    elif name == "edges":                                             # one class touches all four edges (a frame), another inside
        lab = np.zeros((b, h, w), dtype=np.int64)
        inner = (yy > 0) & (yy < h - 1) & (xx > 0) & (xx < w - 1)
        lab[:, inner] = c - 1
        lab[:, h // 2, w // 2] = 0
    elif name == "absent":                                            # class 1 absent; the last slice all background
        small = rs.randint(0, c, size=(b, max(h // 5, 1), max(w // 5, 1)))
        lab = small[:, (yy * small.shape[1] // h), (xx * small.shape[2] // w)]
        lab[lab == 1] = 0
        lab[-1] = 0
    else:
        raise KeyError(name)
    return np.ascontiguousarray(lab).astype(np.int64)


def loss_case(n, b, c, h, w, seed):
    """(t, z, sdf) fp32 CPU tensors: half the pixels have |t| <= 5e-3 (|k t| <= 7.5 at k = 1500: the unsaturated sigmoid), the rest span
    [-1, 1]; logits 2 * randn; sdf in [-1, 1]."""
    rs = np.random.RandomState(seed)
    shape = (n, c, h, w)
    small = rs.uniform(-5e-3, 5e-3, shape)
    wide = rs.uniform(-1.0, 1.0, shape)
    t = np.where(rs.uniform(size=shape) < 0.5, small, wide)
    z = 2.0 * rs.standard_normal(shape)
    s = np.clip(rs.uniform(-1.2, 1.2, (b, c, h, w)), -1.0, 1.0)
    return torch.from_numpy(t).float(), torch.from_numpy(z).float(), torch.from_numpy(s).float()


# ------------------------------------------------------------------------------------------- the scenarios of tests/golden/dtc.npz
C, WIDTH, SIZE, BS, EPOCH, IT0 = 5, 8, 32, 2, 20, 300
SEED_NET, STEP_SEEDS, FWD_SEED = 401, (410, 420), 430
LR, MOMENTUM, WD, MAX_IT = 1e-2, 0.9, 1e-3, 200 * 150
BETA, K, CONSISTENCY, RAMPUP = 0.3, 1500.0, 1.0, 40
SDF_FIXTURE = (("blobs", 2, 3, 40, 56), ("absent", 2, 3, 48, 48), ("absent", 2, 3, 256, 256))      # (pattern, B, C, H, W)
SDF_STRIDE = 5                 # the fixture keeps the 256 x 256 map's d2 and sdf at every 5th pixel of both axes


def shapes(in_ch=1, out_ch=C, w=WIDTH):
    """state_dict keys / shapes of the reference's network.dtc.UNet: the stock U-Net's with the two heads in place of decoder.fc."""
    t = OrderedDict()
    for k, v in recipe.unet_shapes(in_ch, out_ch, w).items():
        if k == "decoder.fc.weight":
            t["decoder.fc1.0.weight"] = v
            t["decoder.fc2.weight"] = v
        else:
            t[k] = v
    return t


def rampup(cur, length):
    ph = 1.0 - np.clip(cur, 0.0, length) / length
    return float(np.exp(-5.0 * ph * ph))


def step_inputs(seed):
    """([labelled | unlabelled] images [2 BS, 1, S, S], labels [BS, S, S]) of one step"""
    return (recipe.synth_images((2 * BS, 1, SIZE, SIZE), seed), recipe.synth_labels(BS, SIZE, SIZE, C, seed + 1, block=8))


def fwd_input():
    return recipe.synth_images((2, 1, SIZE, SIZE), FWD_SEED)
