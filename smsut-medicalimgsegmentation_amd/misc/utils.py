"""The pieces of the reference's ``misc/utils.py`` that the hot-path trainers touch: ``Meter`` (:58-160) and
``maybe_mkdir``; plus the Dice matrix of ``get_mo_matrix`` (:180-203) with medpy's ``dc`` restated from its
formula (medpy is a third-party dependency that is not installed here; SURVEY.md 8c: parity unpinned), and the test
table of ``get_all_matrix`` (:206-283) with ``connected_components`` (:18-36) and medpy's ``assd`` restated on the GPU
(csrc/metrics.hip; skimage and medpy are not installed here either, the same unpinned parity); and medpy's ``hd`` / ``hd95`` /
``asd`` with ``get_hd_matrix``, the Hausdorff table the reference imported ``hd`` for and then left out; and, with no counterpart
upstream, the translator's metrics: ``ssim`` / ``psnr`` / ``mae``, ``TranslationMeter`` and ``translation_tables``
(csrc/similarity.hip)."""
import os
from collections import OrderedDict
from copy import deepcopy
from typing import NamedTuple

import numpy as np

from .. import config as cfg


def maybe_mkdir(*paths):
    for p in paths:
        os.makedirs(p, exist_ok=True)


def binary_dc(result, reference):
    """medpy.metric.binary.dc: 2|A&B| / (|A|+|B|); 0.0 when both are empty."""
    a = np.asarray(result).astype(bool)
    b = np.asarray(reference).astype(bool)
    den = np.count_nonzero(a) + np.count_nonzero(b)
    return 2.0 * np.count_nonzero(a & b) / float(den) if den else 0.0


def get_mo_matrix(prd_npys, gt_npys):
    """Modality x organ Dice matrix, per 3-D volume then averaged (utils.py:180-203)."""
    matrix = np.zeros((cfg.n_modal, cfg.n_label))
    n = np.zeros((cfg.n_modal, 1))
    for k in gt_npys.keys():
        m = cfg.Modality[k.split("_")[0]].value
        p, g = prd_npys[k], gt_npys[k]
        for i in range(cfg.n_label):
            matrix[m][i] += binary_dc(p == i + 1, g == i + 1)
        n[m] += 1
    n[n == 0] += 1e-8
    matrix /= n
    full = np.zeros((cfg.n_modal + 1, cfg.n_label + 1))
    full[:cfg.n_modal, :cfg.n_label] = matrix
    full[-1, :] = np.mean(full[0:cfg.n_modal], axis=0)
    full[:, -1] = np.mean(full[:, 0:cfg.n_label], axis=1)
    return full


def _full_matrix(matrix, n):
    """Per-modality average with the reference's zero guard, then the mean row and column (utils.py:196-203, :255-280)."""
    n = n.copy()
    n[n == 0] += 1e-8
    matrix = matrix / n
    full = np.zeros((cfg.n_modal + 1, cfg.n_label + 1))
    full[:cfg.n_modal, :cfg.n_label] = matrix
    full[-1, :] = np.mean(full[0:cfg.n_modal], axis=0)
    full[:, -1] = np.mean(full[:, 0:cfg.n_label], axis=1)
    return full


def dice_matrix_from_counts(keys, counts):
    """``get_mo_matrix`` from overlap counts instead of volumes.  ``keys``: the volume keys 'm_pid' in slot order; ``counts``:
    an integer array [len(keys), K, 3] = {|P & G|, |P|, |G|} per (volume, class), class 0 the background (what
    ``ops.eval_overlap`` accumulates; organ i is class i + 1, a class K does not reach scores 0.0 as it does there).  The
    result is ``get_mo_matrix``'s bit for bit when the counts are those of the volumes it is given, in the same key order:
    the same fp64 expression on equal integers, accumulated per modality in the same order, the same 1e-8 guard and means."""
    counts = np.asarray(counts)
    keys = list(keys)
    if counts.dtype == np.bool_ or not np.issubdtype(counts.dtype, np.integer):
        raise TypeError(f"dice_matrix_from_counts: expected integer counts, got {counts.dtype}")
    if counts.ndim != 3 or counts.shape[0] != len(keys) or counts.shape[2] != 3:
        raise ValueError(f"dice_matrix_from_counts: expected counts of shape [{len(keys)}, K, 3], got {counts.shape}")
    matrix = np.zeros((cfg.n_modal, cfg.n_label))
    n = np.zeros((cfg.n_modal, 1))
    for slot, k in enumerate(keys):
        m = cfg.Modality[k.split("_")[0]].value
        for i in range(cfg.n_label):
            inter, n_p, n_g = (int(v) for v in counts[slot, i + 1]) if i + 1 < counts.shape[1] else (0, 0, 0)
            matrix[m][i] += 2.0 * inter / float(n_p + n_g) if n_p + n_g else 0.0
        n[m] += 1
    return _full_matrix(matrix, n)


class DiceCounter:
    """The Dice overlap counts of one validation pass, kept on the device.  A volume key 'm_pid' gets a slot in order of first
    appearance (``keys``); ``update`` adds a batch's counts into int64 ``counts`` [slots, K, 3] with one ``ops.eval_overlap``
    launch; ``matrix`` makes the one device-to-host copy.  The tensor is allocated at the first update (K = its class count),
    zero-initialised, and doubled on the device when the slots run out: nothing waits for the device before ``matrix``."""

    def __init__(self, slots=16):
        self._slots = max(int(slots), 1)
        self.keys = []
        self.counts = None
        self.classes = None
        self._slot_of = {}
        self._seen = set()

    def update(self, logits, labels, names, classes=None, want_pred=False):
        """Count one batch: ``names`` 'm_pid_z', one per slice of ``logits`` / ``labels`` (``ops.eval_overlap``'s arguments).
        A name seen before raises ``ValueError``: the host path overwrites a repeated slice, counts would add it twice.
        Returns the uint8 prediction with ``want_pred``, else None."""
        import torch
        from .. import ops
        names = list(names)
        fresh, keys = set(), []
        for nm in names:
            m, pid, _ = nm.split("_")
            cfg.Modality[m]                                  # (KeyError now, not in matrix())
            if nm in self._seen or nm in fresh:
                raise ValueError(f"DiceCounter: slice {nm!r} was counted before")
            fresh.add(nm)
            keys.append(f"{m}_{pid}")
        k = int(logits.shape[1] if classes is None else classes)
        if self.classes is not None and k != self.classes:
            raise ValueError(f"DiceCounter: {k} classes after {self.classes}")
        n_new = len(set(keys) - set(self._slot_of))
        if self.counts is None or len(self.keys) + n_new > self.counts.shape[0]:
            size = self._slots if self.counts is None else self.counts.shape[0]
            while size < len(self.keys) + n_new:
                size *= 2
            grown = torch.zeros(size, k, 3, dtype=torch.int64, device=logits.device)
            if self.counts is not None:
                grown[:self.counts.shape[0]] = self.counts
            slot_of, key_list = dict(self._slot_of), list(self.keys)
        else:
            grown, slot_of, key_list = self.counts, dict(self._slot_of), list(self.keys)
        for key in keys:
            if key not in slot_of:
                slot_of[key] = len(key_list)
                key_list.append(key)
        pred = ops.eval_overlap(logits, labels, [slot_of[key] for key in keys], grown, classes=k, want_pred=want_pred)
        self.counts, self.classes, self._slot_of, self.keys = grown, k, slot_of, key_list     # (only once the launch is out)
        self._seen |= fresh
        return pred

    def matrix(self):
        """The modality x organ Dice matrix of everything counted so far (``dice_matrix_from_counts``)."""
        if self.counts is None:
            return dice_matrix_from_counts([], np.zeros((0, cfg.n_label + 1, 3), dtype=np.int64))
        return dice_matrix_from_counts(self.keys, self.counts[:len(self.keys)].cpu().numpy())


def _device_u8(a, what):
    """An integer (or bool) NumPy array with values in 0..255 as a uint8 tensor on the current HIP device.  A tensor is taken
    as it is when it already is that -- uint8, on the current HIP device (volumes assembled there by
    ``validate_epoch_device``) -- and any other tensor raises ``TypeError``: nothing is converted or moved silently."""
    import torch
    from .._hip import SmsutHipError
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.uint8 or not a.is_cuda or a.device.index != torch.cuda.current_device():
            raise TypeError(f"{what}: a tensor must be uint8 on the current HIP device, got {a.dtype} on {a.device}")
        return a
    a = np.asarray(a)
    if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{what}: expected an integer array, got {a.dtype}")
    if a.size and (a.min() < 0 or a.max() > 255):
        raise ValueError(f"{what}: values must lie in 0..255 (got {a.min()}..{a.max()})")
    if not torch.cuda.is_available():
        raise SmsutHipError("the test-phase metrics run on an MI355X (no HIP device visible; there is no CPU fallback)")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(torch.device("cuda", torch.cuda.current_device()))


def connected_components(pred):
    """utils.py:18-36 on the GPU: for each class c = 1 .. cfg.n_modal (the reference's bound, ``range(cfg.n_modal)``, not
    n_label; both are 4 in config.py) label the components of ``pred == c`` with skimage's connectivity=2 (18-neighbour in
    3-D, 8-neighbour in 2-D) and keep those of more than 0.1 * (voxels of class c) voxels (fp64 comparison; a component of
    exactly a tenth is dropped).  Kept voxels hold c, all others 0 (values above n_modal too).  2-D or 3-D integer array in
    0..255 -> uint8 array of the same shape."""
    from .. import ops
    t = _device_u8(pred, "connected_components")
    if t.dim() not in (2, 3):
        raise ValueError(f"connected_components: expected a 2-D or 3-D array, got shape {tuple(t.shape)}")
    return ops.cc_filter(t, cfg.n_modal, per_slice=False).cpu().numpy()


def _masks(result, reference, what):
    a = _device_u8(np.asarray(result).astype(bool), what)
    b = _device_u8(np.asarray(reference).astype(bool), what)
    if a.shape != b.shape or a.dim() not in (2, 3):
        raise ValueError(f"{what}: expected two 2-D or 3-D masks of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    return a, b


def _raise_if_empty(n_result, n_reference):
    if n_result == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if n_reference == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")


def _voxelspacing(voxelspacing, ndim):
    """medpy's ``voxelspacing`` for an ``ndim``-axis array: None stays None (unit spacing, the integer kernels), a scalar is
    broadcast to every axis, a sequence needs one entry per axis (``RuntimeError`` otherwise, as scipy's
    ``_normalize_sequence`` raises through medpy); entries that are not finite and positive raise ``ValueError``.  Pure host
    code: nothing touches the device."""
    from .. import ops
    if voxelspacing is None:
        return None
    if np.ndim(voxelspacing) == 0:
        voxelspacing = (voxelspacing,) * ndim
    return ops.check_spacing(voxelspacing, ndim)


def _spacings_for(spacings, keys):
    """{volume key: (sz, sy, sx) or None} for ``get_all_matrix`` / ``get_hd_matrix``.  ``spacings``: None, one (sz, sy, sx)
    for every volume, or a mapping in which a volume 'ct_001' is looked up by its own key first and then by its modality name
    'ct'; a volume found under neither raises ``KeyError`` naming it.  Pure host code, run before any volume is uploaded."""
    from collections.abc import Mapping
    keys = list(keys)
    if spacings is None:
        return {k: None for k in keys}
    if not isinstance(spacings, Mapping):
        sp = _voxelspacing(spacings, 3)
        return {k: sp for k in keys}
    out = {}
    for k in keys:
        modality = k.split("_")[0]
        if k in spacings:
            out[k] = _voxelspacing(spacings[k], 3)
        elif modality in spacings:
            out[k] = _voxelspacing(spacings[modality], 3)
        else:
            raise KeyError(f"no voxel spacing for volume {k!r} (neither under {k!r} nor under its modality {modality!r})")
    return out


def assd(result, reference, voxelspacing=None):
    """medpy.metric.binary.assd (erosion connectivity 1) on the GPU: the mean of the two average surface distances, each the
    mean over one mask's border voxels (mask XOR its erosion by the 6-neighbour cross, array faces outside) of the exact
    Euclidean distance to the other mask's border.  2-D or 3-D masks (nonzero = in); ``RuntimeError`` when either is empty,
    as medpy raises.  ``voxelspacing``: None (distances in voxels), a scalar, or one value per array axis, medpy's meaning."""
    from .. import ops
    sp = _voxelspacing(voxelspacing, np.ndim(result))
    a, b = _masks(result, reference, "assd")
    st = ops.surface_stats(a, b, 1, spacing=sp)[0]
    _raise_if_empty(st[1], st[2])
    return 0.5 * (st[4] / st[3] + st[6] / st[5])


def _hd_of(row):
    """Hausdorff distance from one row of ``ops.surface_hd``: the square root of the larger directed maximum."""
    return float(np.sqrt(max(row[2], row[3])))


def _percentile_of(row, quantile):
    """numpy.percentile (linear interpolation) of the pooled distances from one row of ``ops.surface_hd`` taken at
    ``quantile``: the two neighbouring order statistics are exact square roots, the weight is the rank's fraction."""
    n = row[0] + row[1]
    pos = (n - 1) * quantile
    a, b = np.sqrt(row[4]), np.sqrt(row[5])
    return float(a + (b - a) * (pos - np.floor(pos)))


def hd(result, reference, voxelspacing=None):
    """medpy.metric.binary.hd (erosion connectivity 1) on the GPU: the largest distance from a border voxel of either mask
    to the other mask's border -- the square root of an exact maximum of squared distances (integers without
    ``voxelspacing``).  2-D or 3-D masks; ``RuntimeError`` when either is empty, as medpy raises.  ``voxelspacing`` as in
    ``assd``."""
    from .. import ops
    sp = _voxelspacing(voxelspacing, np.ndim(result))
    a, b = _masks(result, reference, "hd")
    row = ops.surface_hd(a, b, 1, spacing=sp)[0]
    _raise_if_empty(row[0], row[1])
    return _hd_of(row)


def hd95(result, reference, voxelspacing=None):
    """medpy.metric.binary.hd95 on the GPU: ``numpy.percentile(numpy.hstack((d_pg, d_gp)), 95)`` of the two directed sets of
    surface distances.  The device selects the two order statistics around rank (n - 1) * 0.95 exactly; the host
    interpolates between their square roots.  ``RuntimeError`` when either mask is empty.  ``voxelspacing`` as in ``assd``."""
    from .. import ops
    sp = _voxelspacing(voxelspacing, np.ndim(result))
    a, b = _masks(result, reference, "hd95")
    row = ops.surface_hd(a, b, 1, q=95.0, spacing=sp)[0]
    _raise_if_empty(row[0], row[1])
    return _percentile_of(row, 0.95)


def asd(result, reference, voxelspacing=None):
    """medpy.metric.binary.asd on the GPU: the mean over ``result``'s border voxels of the distance to ``reference``'s border
    (directed; ``assd`` averages both directions).  ``RuntimeError`` when either mask is empty.  ``voxelspacing`` as in
    ``assd``."""
    from .. import ops
    sp = _voxelspacing(voxelspacing, np.ndim(result))
    a, b = _masks(result, reference, "asd")
    st = ops.surface_stats(a, b, 1, spacing=sp)[0]
    _raise_if_empty(st[1], st[2])
    return st[4] / st[3]


def get_hd_matrix(prd_npys, gt_npys, spacings=None):
    """(Hausdorff, HD95) modality x organ matrices, each (n_modal + 1) x (n_label + 1) with the mean row and column: what the
    reference's commented-out ``hd(predx, gx)`` (utils.py:245) and ``{modality}_hd_matrix.csv`` would have held, plus the
    95th percentile.  Input checks, the two-stage cleanup and the per-modality averaging are ``get_all_matrix``'s; an organ
    the cleaned prediction lacks takes, per metric, the running maximum of this volume's earlier organs (0 for the first);
    an empty ground truth under a non-empty prediction raises RuntimeError.  ``spacings`` as in ``get_all_matrix``: both
    matrices are then in the spacing's unit."""
    from .. import ops
    spacing_of = _spacings_for(spacings, gt_npys.keys())
    hd_matrix = np.zeros((cfg.n_modal, cfg.n_label))
    hd95_matrix = np.zeros((cfg.n_modal, cfg.n_label))
    n = np.zeros((cfg.n_modal, 1))
    for k in gt_npys.keys():
        m = cfg.Modality[k.split("_")[0]].value
        p = _device_u8(prd_npys[k], f"prediction {k}")
        g = _device_u8(gt_npys[k], f"ground truth {k}")
        if p.dim() != 3 or p.shape != g.shape:
            raise ValueError(f"{k}: expected two [D, H, W] volumes of one shape, got {tuple(p.shape)} and {tuple(g.shape)}")
        p1 = ops.cc_filter(p, cfg.n_modal, per_slice=False)
        p1 = ops.cc_filter(p1, cfg.n_modal, per_slice=True)
        rows = ops.surface_hd(p1, g, cfg.n_label, q=95.0, spacing=spacing_of[k])
        maxhd, maxhd95 = 0, 0
        for i in range(cfg.n_label):
            if rows[i][0] == 0:
                h, h95 = maxhd, maxhd95
            elif rows[i][1] == 0:
                raise RuntimeError("The second supplied array does not contain any binary object.")
            else:
                h, h95 = _hd_of(rows[i]), _percentile_of(rows[i], 0.95)
            maxhd = maxhd if maxhd > h else h
            maxhd95 = maxhd95 if maxhd95 > h95 else h95
            hd_matrix[m][i] += h
            hd95_matrix[m][i] += h95
        n[m] += 1
    return _full_matrix(hd_matrix, n), _full_matrix(hd95_matrix, n)


def get_all_matrix(prd_npys, gt_npys, spacings=None):
    """utils.py:206-283: (Dice, "Hausdorff", ASSD) modality x organ matrices, each (n_modal + 1) x (n_label + 1) with the
    mean row and column.  Per volume: connected_components in 3-D, then on every z slice alone (its own class totals);
    per organ j the Dice of the cleaned prediction and, if the prediction holds j, its ASSD to the ground truth -- else the
    running maximum of the ASSDs of this volume's earlier organs (0 for the first).  An empty ground truth under a
    non-empty prediction raises RuntimeError, as in the reference.  The second matrix is the reference's placeholder
    (``t = s``, its hd call commented out): a copy of the Dice values; ``get_hd_matrix`` computes the real Hausdorff and HD95
    matrices.  Each volume is uploaded once; cleanup and surface
    statistics run on the device.  ``spacings``: None (ASSD in voxels), one ``(sz, sy, sx)`` for every volume, or a mapping
    from a volume's key ('ct_001') or, failing that, its modality name ('ct') to its spacing (``KeyError`` naming the volume
    that has neither); the ASSD matrix is then in the spacing's unit.  Dice, the cleanup and the running-maximum rule do not
    depend on it."""
    from .. import ops
    spacing_of = _spacings_for(spacings, gt_npys.keys())
    matrix = np.zeros((cfg.n_modal, cfg.n_label))
    hd_matrix = np.zeros((cfg.n_modal, cfg.n_label))
    assd_matrix = np.zeros((cfg.n_modal, cfg.n_label))
    n = np.zeros((cfg.n_modal, 1))
    for k in gt_npys.keys():
        m = cfg.Modality[k.split("_")[0]].value
        p = _device_u8(prd_npys[k], f"prediction {k}")
        g = _device_u8(gt_npys[k], f"ground truth {k}")
        if p.dim() != 3 or p.shape != g.shape:
            raise ValueError(f"{k}: expected two [D, H, W] volumes of one shape, got {tuple(p.shape)} and {tuple(g.shape)}")
        p1 = ops.cc_filter(p, cfg.n_modal, per_slice=False)
        p1 = ops.cc_filter(p1, cfg.n_modal, per_slice=True)
        st = ops.surface_stats(p1, g, cfg.n_label, spacing=spacing_of[k])
        maxassd = 0
        for i in range(cfg.n_label):
            inter, n_p, n_g, b_p, s_p, b_g, s_g = st[i]
            den = n_p + n_g
            s = 2.0 * inter / float(den) if den else 0.0
            if n_p == 0:
                r = maxassd
            elif n_g == 0:
                raise RuntimeError("The second supplied array does not contain any binary object.")
            else:
                r = 0.5 * (s_p / b_p + s_g / b_g)
            maxassd = maxassd if maxassd > r else r
            matrix[m][i] += s
            hd_matrix[m][i] += s
            assd_matrix[m][i] += r
        n[m] += 1
    return _full_matrix(matrix, n), _full_matrix(hd_matrix, n), _full_matrix(assd_matrix, n)


def matrix_text(matrix):
    """Rows of '%.4f' values joined by ',' (the layout of the reference's ``{modality}_trois_matrix.csv``)."""
    return "".join(",".join("%.4f" % v for v in row) + "\n" for row in matrix)


# ------------------------------------------------------------------------------------------- translation metrics (test phase)
# SSIM (Wang et al. 2004: 11x11 Gaussian window, sigma 1.5, population moments; what skimage's structural_similarity computes with
# gaussian_weights=True, sigma=1.5, use_sample_covariance=False -- skimage is not installed here: parity unpinned), PSNR and MAE of
# the unified translator's images, from the three per-slice sums of ``ops.image_similarity`` (csrc/similarity.hip).
def _device_f32(a, what):
    """A NumPy array of numbers as a float32 tensor on the current HIP device.  A tensor is taken as it is when it already is
    that -- float32 on a HIP device -- and any other tensor raises ``TypeError``: nothing is converted or moved silently."""
    import torch
    from .._hip import SmsutHipError
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.float32 or not a.is_cuda:
            raise TypeError(f"{what}: a tensor must be float32 on a HIP device, got {a.dtype} on {a.device}")
        return a
    a = np.asarray(a)
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise TypeError(f"{what}: expected an array of numbers, got {a.dtype}")
    if not torch.cuda.is_available():
        raise SmsutHipError("the translation metrics run on an MI355X (no HIP device visible; there is no CPU fallback)")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.device("cuda", torch.cuda.current_device()))


def _similarity_sums(a, b, data_range, what):
    """``(rows, h, w)``: the [D, 3] host array of ``ops.image_similarity`` for one image [H, W] or one volume [D, H, W]."""
    from .. import ops
    if np.ndim(a) not in (2, 3) or tuple(np.shape(a)) != tuple(np.shape(b)):
        raise ValueError(f"{what}: expected two [H, W] images or [D, H, W] volumes of one shape, got {tuple(np.shape(a))} and "
                         f"{tuple(np.shape(b))}")
    ta, tb = _device_f32(a, what), _device_f32(b, what)
    h, w = ta.shape[-2:]
    rows = ops.image_similarity(ta.reshape(-1, h, w), tb.reshape(-1, h, w), data_range)
    return rows.cpu().numpy(), int(h), int(w)


def _psnr_of(se, voxels, data_range):
    """10 log10(L^2 / MSE) with MSE = se / voxels; ``inf`` when the squared error is exactly 0."""
    if se == 0:
        return float("inf")
    return float(10.0 * np.log10(float(data_range) ** 2 / (se / voxels)))


def ssim(a, b, data_range):
    """Structural similarity of one image or volume on the GPU: the mean over the slices of each slice's mean SSIM over its
    window centres (the pixels at least 5 from every edge).  NumPy arrays or float32 device tensors -> Python float."""
    rows, h, w = _similarity_sums(a, b, data_range, "ssim")
    return float(np.mean(rows[:, 0] / float((h - 10) * (w - 10))))


def psnr(a, b, data_range):
    """Peak signal-to-noise ratio of one image or volume on the GPU: 10 log10(L^2 / MSE), MSE over all its voxels (fp64 sums of
    fp64 differences); ``inf`` for identical inputs."""
    rows, h, w = _similarity_sums(a, b, data_range, "psnr")
    return _psnr_of(rows[:, 1].sum(), rows.shape[0] * h * w, data_range)


def mae(a, b):
    """Mean absolute error of one image or volume on the GPU (fp64 sums of fp64 differences)."""
    rows, h, w = _similarity_sums(a, b, 1.0, "mae")
    return float(rows[:, 2].sum() / (rows.shape[0] * h * w))


TRANSLATION_TABLES = ("cycle", "paired")


def translation_tables(rows, names, cells, shapes, data_range=1.0):
    """The translation tables from per-slice sums.  ``rows``: float array [M, 3] = {sum of SSIM over window centres, SE, AE} per
    compared slice (``ops.image_similarity``); ``names``: its slice names 'm_pid_z'; ``cells``: per slice ``(row, col, table)``
    with table in ``TRANSLATION_TABLES``; ``shapes``: per slice ``(H, W)``.  Returns ``{table: (ssim, psnr, mae)}``, each an
    [n_modal, n_modal] fp64 array.  A slice belongs to the volume 'm_pid' of its name; within a cell
      volume SSIM = mean of its slices' SSIM (a slice's = its sum / ((H-10)(W-10))),
      volume PSNR = 10 log10(L^2 / (sum SE / voxels)), ``inf`` when sum SE == 0 (from the volume's MSE, not a mean of slice PSNRs),
      volume MAE  = sum AE / voxels,
    and the cell is the mean over its volumes (as ``get_mo_matrix`` averages a modality's volumes); a cell without data is NaN.
    Pure host code."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 3)
    names, cells, shapes = list(names), list(cells), list(shapes)
    if not (len(names) == len(cells) == len(shapes) == rows.shape[0]):
        raise ValueError(f"translation_tables: {rows.shape[0]} rows for {len(names)} names, {len(cells)} cells, {len(shapes)} shapes")
    vols = OrderedDict()                                 # (table, row, col, 'm_pid') -> [sum of slice SSIM, slices, SE, AE, voxels]
    for r, nm, (i, j, table), (h, w) in zip(rows, names, cells, shapes):
        if table not in TRANSLATION_TABLES or not (0 <= i < cfg.n_modal and 0 <= j < cfg.n_modal):
            raise ValueError(f"translation_tables: no cell {(i, j, table)!r}")
        m, pid, _ = nm.split("_")
        v = vols.setdefault((table, int(i), int(j), f"{m}_{pid}"), [0.0, 0, 0.0, 0.0, 0])
        v[0] += r[0] / float((h - 10) * (w - 10)); v[1] += 1
        v[2] += r[1]; v[3] += r[2]; v[4] += h * w
    sums = {t: np.zeros((3, cfg.n_modal, cfg.n_modal)) for t in TRANSLATION_TABLES}
    count = {t: np.zeros((cfg.n_modal, cfg.n_modal)) for t in TRANSLATION_TABLES}
    for (table, i, j, _), (s, n, se, ae, voxels) in vols.items():
        sums[table][0, i, j] += s / n
        sums[table][1, i, j] += _psnr_of(se, voxels, data_range)
        sums[table][2, i, j] += ae / voxels
        count[table][i, j] += 1
    out = {}
    for t in TRANSLATION_TABLES:
        with np.errstate(invalid="ignore", divide="ignore"):
            out[t] = tuple(np.where(count[t] > 0, sums[t][k] / count[t], np.nan) for k in range(3))
    return out


def translation_text(tables):
    """Six ``matrix_text`` blocks with an empty line between them: cycle SSIM, cycle PSNR, cycle MAE, paired SSIM, paired PSNR,
    paired MAE ('%.4f' values separated by ','; ``nan`` / ``inf`` as Python formats them)."""
    return "\n".join(matrix_text(m) for t in TRANSLATION_TABLES for m in tables[t])


class TranslationMeter:
    """The translation metrics of one test pass, kept on the device.  ``update`` compares a batch of image pairs with one
    ``ops.image_similarity`` launch and keeps its [N, 3] rows there, with the slices' names and the cell ``(row, col, table)``
    they count for; ``result`` makes the one stacked device-to-host copy and returns ``translation_tables`` of it.  Nothing waits
    for the device before ``result``."""

    def __init__(self, data_range=1.0):
        self.data_range = float(data_range)
        self._rows, self._names, self._cells, self._shapes = [], [], [], []

    def update(self, a, b, names, row, col, table):
        """Compare ``a`` with ``b`` (fp32 [N, H, W] or [N, 1, H, W] on the device); ``names``: N slice names 'm_pid_z'."""
        from .. import ops
        names = list(names)
        if table not in TRANSLATION_TABLES or not (0 <= int(row) < cfg.n_modal and 0 <= int(col) < cfg.n_modal):
            raise ValueError(f"TranslationMeter: no cell {(row, col, table)!r}")
        if len(names) != a.shape[0]:
            raise ValueError(f"TranslationMeter: {len(names)} names for {a.shape[0]} slices")
        for nm in names:
            if len(nm.split("_")) != 3:
                raise ValueError(f"TranslationMeter: slice name {nm!r} is not 'm_pid_z'")
        self._rows.append(ops.image_similarity(a, b, self.data_range))
        self._names += names
        self._cells += [(int(row), int(col), table)] * len(names)
        self._shapes += [(int(a.shape[-2]), int(a.shape[-1]))] * len(names)

    def rows(self):
        """Everything collected so far as one float64 host array [M, 3]: one stacked copy."""
        import torch
        if not self._rows:
            return np.zeros((0, 3))
        return torch.cat(self._rows).cpu().numpy()

    def result(self):
        return translation_tables(self.rows(), self._names, self._cells, self._shapes, self.data_range)


# ------------------------------------------------------------------------------------------- calibration (test phase)
# How far the network's probabilities can be trusted: expected / maximum calibration error (Guo et al. 2017: confidence bins of equal
# width), negative log-likelihood, Brier score and the reliability table, from the totals of ``ops.calibration_stats``
# (csrc/calibration.hip), and the one-parameter fix: a temperature fitted by Newton's method on the NLL.
class CalibrationTotals:
    """The calibration metrics of one totals vector of ``ops.calibration_stats`` (``ops.CalibrationLayout(classes, bins)``), in fp64
    on the host.  With n = the counted pixels, and per bin b its pixels n_b, accuracy acc_b and mean confidence conf_b:
    ECE = sum_b (n_b / n) |acc_b - conf_b|, MCE = the largest |acc_b - conf_b| of a non-empty bin; NLL, Brier and accuracy are
    means over the counted pixels.  Everything is NaN when nothing was counted.  Pure host code."""

    def __init__(self, totals, classes, bins):
        from ..ops import CalibrationLayout
        self.layout = CalibrationLayout(classes, bins)
        self.totals = np.asarray(totals, dtype=np.float64)
        if self.totals.shape != (self.layout.size,):
            raise ValueError(f"CalibrationTotals: expected {self.layout.size} totals, got shape {self.totals.shape}")
        self._bins, self._classes = self.layout.bins(self.totals), self.layout.classes(self.totals)

    @property
    def pixels(self):
        return float(self._bins[:, 0].sum())

    def _gaps(self):
        """(pixels, |accuracy - mean confidence|) of the non-empty bins"""
        has = self._bins[:, 0] > 0
        n = self._bins[has, 0]
        return n, np.abs(self._bins[has, 2] / n - self._bins[has, 1] / n)

    def ece(self):
        n, gap = self._gaps()
        return float((n / n.sum() * gap).sum()) if n.size else float("nan")

    def mce(self):
        n, gap = self._gaps()
        return float(gap.max()) if n.size else float("nan")

    def _mean(self, total):
        return float(total / self.pixels) if self.pixels else float("nan")

    def nll(self):
        return self._mean(self._classes[:, 2].sum())

    def brier(self):
        return self._mean(self._classes[:, 3].sum())

    def accuracy(self):
        return self._mean(self._bins[:, 2].sum())

    def reliability(self):
        """[bins, 5]: the bin's lower edge, upper edge, pixels, mean confidence, accuracy (NaN for an empty bin)."""
        b = self.layout.n_bins
        out = np.full((b, 5), np.nan)
        out[:, 0], out[:, 1], out[:, 2] = np.arange(b) / b, (np.arange(b) + 1.0) / b, self._bins[:, 0]
        has = self._bins[:, 0] > 0
        out[has, 3], out[has, 4] = self._bins[has, 1] / self._bins[has, 0], self._bins[has, 2] / self._bins[has, 0]
        return out

    def per_class(self):
        """[classes, 4] by TRUE class: pixels, accuracy (the class's recall), mean NLL, mean Brier (NaN for an absent class)."""
        out = np.full((self.layout.n_classes, 4), np.nan)
        out[:, 0] = self._classes[:, 0]
        has = self._classes[:, 0] > 0
        out[has, 1:] = self._classes[has, 1:] / self._classes[has, :1]
        return out

    def grad(self):
        return float(self.layout.grad(self.totals))

    def curv(self):
        return float(self.layout.curv(self.totals))

    def skipped(self):
        return int(self.layout.skipped(self.totals))

    def nonfinite(self):
        return int(self.layout.nonfinite(self.totals))

    def summary(self):
        """(ECE, MCE, NLL, Brier, accuracy): one row of the test phase's table."""
        return (self.ece(), self.mce(), self.nll(), self.brier(), self.accuracy())


class CalibrationMeter:
    """The calibration totals of one test pass, kept on the device: ``rows`` totals vectors (one per modality in the test phase;
    one by default) in a single fp64 tensor.  ``update`` adds a batch into a row with one ``ops.calibration_stats`` call and reads
    nothing back; the first metric asked for makes the ONE device-to-host copy (kept until the next ``update``).  Every metric takes
    ``row``: one row, or None for the sum of all rows."""

    def __init__(self, classes, bins=15, temperature=1.0, rows=1):
        from .. import ops
        self.layout = ops.CalibrationLayout(classes, bins)
        ops.calibration_beta(temperature)
        self.classes, self.bins, self.temperature, self.rows = int(classes), int(bins), float(temperature), int(rows)
        if self.rows < 1:
            raise ValueError(f"CalibrationMeter: needs at least one row, got {rows}")
        self._dev, self._host = None, None

    def update(self, out, msk, row=0):
        """Add the batch ``out`` (logits, logical NCHW on the device) / ``msk`` (int64 [N, H, W]) into ``row``."""
        import torch
        from .. import ops
        if not 0 <= int(row) < self.rows:
            raise ValueError(f"CalibrationMeter: no row {row} of {self.rows}")
        if not isinstance(out, torch.Tensor) or not out.is_cuda:
            raise TypeError("CalibrationMeter: the logits must be a tensor on a HIP device (no CPU fallback)")
        if self._dev is None:
            self._dev = torch.zeros(self.rows, self.layout.size, dtype=torch.float64, device=out.device)
        ops.calibration_stats(out, msk, self._dev[int(row)], classes=self.classes, bins=self.bins, temperature=self.temperature)
        self._host = None

    def totals(self):
        """Everything counted so far as a float64 host array [rows, size]: one copy."""
        if self._host is None:
            self._host = np.zeros((self.rows, self.layout.size)) if self._dev is None else self._dev.cpu().numpy()
        return self._host

    def result(self, row=None):
        t = self.totals()
        return CalibrationTotals(t.sum(axis=0) if row is None else t[int(row)], self.classes, self.bins)

    def ece(self, row=None):
        return self.result(row).ece()

    def mce(self, row=None):
        return self.result(row).mce()

    def nll(self, row=None):
        return self.result(row).nll()

    def brier(self, row=None):
        return self.result(row).brier()

    def accuracy(self, row=None):
        return self.result(row).accuracy()

    def reliability(self, row=None):
        return self.result(row).reliability()

    def per_class(self, row=None):
        return self.result(row).per_class()


def _device_logits(logits, labels, what):
    """Logits [N, C, H, W] and labels [N, H, W] as ``ops.calibration_stats`` takes them.  Tensors are taken as they are when they
    already are that (float32 / int64 on a HIP device), any other tensor raises ``TypeError``; NumPy arrays are uploaded (the logits
    in NHWC memory)."""
    import torch
    from .._hip import SmsutHipError
    if isinstance(logits, torch.Tensor) != isinstance(labels, torch.Tensor):
        raise TypeError(f"{what}: logits and labels must both be tensors or both be arrays")
    if isinstance(logits, torch.Tensor):
        if logits.dtype != torch.float32 or labels.dtype != torch.int64 or not logits.is_cuda or not labels.is_cuda:
            raise TypeError(f"{what}: tensors must be float32 logits and int64 labels on a HIP device, got {logits.dtype} on "
                            f"{logits.device} and {labels.dtype} on {labels.device}")
        return logits, labels
    z, y = np.asarray(logits), np.asarray(labels)
    if not np.issubdtype(z.dtype, np.floating) or not np.issubdtype(y.dtype, np.integer):
        raise TypeError(f"{what}: expected floating logits and integer labels, got {z.dtype} and {y.dtype}")
    if z.ndim != 4 or y.shape != (z.shape[0],) + z.shape[2:]:
        raise ValueError(f"{what}: expected logits [N, C, H, W] and labels [N, H, W], got {z.shape} and {y.shape}")
    if not torch.cuda.is_available():
        raise SmsutHipError("the calibration metrics run on an MI355X (no HIP device visible; there is no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    z = torch.from_numpy(np.ascontiguousarray(z.transpose(0, 2, 3, 1), dtype=np.float32)).to(dev).permute(0, 3, 1, 2)
    return z, torch.from_numpy(np.ascontiguousarray(y, dtype=np.int64)).to(dev)


def _calibration_of(logits, labels, classes, bins, temperature, what):
    z, y = _device_logits(logits, labels, what)
    meter = CalibrationMeter(z.shape[1] if classes is None else classes, bins, temperature)
    meter.update(z, y)
    return meter.result()


def ece(logits, labels, bins=15, classes=None, temperature=1.0):
    """Expected calibration error of one batch of logits [N, C, H, W] against labels [N, H, W] on the GPU (NumPy arrays or device
    tensors -> Python float)."""
    return _calibration_of(logits, labels, classes, bins, temperature, "ece").ece()


def nll(logits, labels, classes=None, temperature=1.0):
    """Mean negative log-likelihood of the labels under ``softmax(logits / temperature)``, on the GPU."""
    return _calibration_of(logits, labels, classes, 1, temperature, "nll").nll()


def brier(logits, labels, classes=None, temperature=1.0):
    """Mean Brier score, sum_k (p_k - [k == y])^2 per pixel, on the GPU."""
    return _calibration_of(logits, labels, classes, 1, temperature, "brier").brier()


def newton_inverse_temperature(evaluate, tol=1e-6, max_iter=30):
    """The safeguarded Newton iteration of the temperature fit, on beta = 1 / T from 1: ``evaluate(beta) -> (g, h)``, the first and
    second derivative of the summed NLL by beta (the NLL is convex in beta: h >= 0).  beta <- beta - g / h; when that would not
    leave beta > 0, or h is not positive, beta is halved instead.  Every iterate is rounded to float32, the format the kernel takes
    it in.  Stops when |new - beta| <= tol * beta, or after ``max_iter`` evaluations.  Returns ``(beta, evaluations)``."""
    beta = 1.0
    for it in range(1, int(max_iter) + 1):
        g, h = evaluate(beta)
        new = beta - g / h if h > 0 else 0.0
        if not new > 0:
            new = 0.5 * beta
        new = float(np.float32(new))
        done = abs(new - beta) <= tol * beta
        beta = new
        if done:
            break
    return beta, it


def fit_temperature(batches, classes, tol=1e-6, max_iter=30):
    """Temperature scaling (Guo et al. 2017): the T that minimises the NLL of ``softmax(logits / T)`` over ``batches``, a sequence
    of ``(logits, labels)`` pairs that stay on the device (``ops.calibration_stats``' arguments).  ``newton_inverse_temperature``
    with one launch per batch and one read-back of the two derivatives per iteration.  Returns ``(T, iterations)``."""
    import torch
    from .. import ops
    batches = list(batches)
    if not batches:
        raise ValueError("fit_temperature: no batches")
    layout = ops.CalibrationLayout(classes, 1)
    tail = slice(layout.size - 4, layout.size - 2)

    def evaluate(beta):
        out = torch.zeros(layout.size, dtype=torch.float64, device=batches[0][0].device)
        for z, y in batches:
            ops.calibration_stats(z, y, out, classes=layout.n_classes, bins=1, temperature=1.0 / beta)
        g, h = out[tail].tolist()
        return g, h

    beta, its = newton_inverse_temperature(evaluate, tol, max_iter)
    return 1.0 / beta, its


CALIBRATION_COLUMNS = ("ECE", "MCE", "NLL", "Brier", "accuracy")


def calibration_rows(meter):
    """[rows + 1, 5]: ``CALIBRATION_COLUMNS`` of every row of a ``CalibrationMeter`` and, last, of all rows together."""
    return np.array([meter.result(r).summary() for r in range(meter.rows)] + [meter.result().summary()])


def calibration_text(reliability, rows_raw, rows_fitted):
    """``{modality}_calibration.csv``: the reliability table (``CalibrationTotals.reliability``), an empty line, the
    ``calibration_rows`` at T = 1, an empty line, the same rows at the fitted temperature; '%.6f' values separated by ','
    (``nan`` as Python formats it)."""
    block = lambda m: "".join(",".join("%.6f" % v for v in row) + "\n" for row in np.asarray(m, dtype=np.float64))
    return block(reliability) + "\n" + block(rows_raw) + "\n" + block(rows_fitted)


class CalibrationReport:
    """What ``-p test`` gathers with ``cfg.test_calibration``: a ``CalibrationMeter`` at T = 1 with one row per modality, fed batch
    by batch, and the batches themselves -- logits and labels stay on the device as the validation loop left them (no copy, no
    second forward pass; 4 C bytes per pixel of the test set) -- for the temperature fit and the statistics at the fitted T."""

    def __init__(self, rows, bins=15):
        self.rows, self.bins = int(rows), int(bins)
        self.meter, self.batches = None, []

    def update(self, out, msk, row, classes=None):
        if self.meter is None:
            self.meter = CalibrationMeter(out.shape[1] if classes is None else classes, self.bins, rows=self.rows)
        self.meter.update(out, msk, row)
        self.batches.append((out, msk, int(row)))

    def finish(self):
        """``(text of the csv, fitted T, Newton iterations)``"""
        if self.meter is None:
            raise ValueError("CalibrationReport: no batch was fed")
        t, its = fit_temperature([(o, m) for o, m, _ in self.batches], self.meter.classes)
        fitted = CalibrationMeter(self.meter.classes, self.bins, temperature=t, rows=self.rows)
        for o, m, r in self.batches:
            fitted.update(o, m, r)
        return calibration_text(self.meter.reliability(), calibration_rows(self.meter), calibration_rows(fitted)), t, its


class StructureAgreement(NamedTuple):
    dice_agreement: np.ndarray                 # [K] mean over members of the Dice of the member's structure with the prediction's
    iou_all: np.ndarray                        # [K] voxels every member gave the class / voxels some member gave it
    volume_cv: np.ndarray                      # [K] population standard deviation of the members' volumes / their mean
    mean_entropy: np.ndarray                   # [K] mean predictive entropy (nat) inside the predicted structure
    voxels: np.ndarray                         # [K] int64: voxels of the predicted structure


QUALITY_COLUMNS = ("class", "voxels", "dice_agreement", "iou_all", "volume_cv", "mean_entropy")


def structure_agreement(counts, members):
    """The label-free, structure-wise quality measures of Roy et al. 2019 (Bayesian QuickNAT) from the int64 counts
    ``[K, 2 T + 4]`` that ``ops.tta_uncertainty`` accumulates over a volume (NumPy array or tensor; ``members`` = T; row k =
    ``{V, ALL, ANY, HSUM, V_0 .. V_{T-1}, I_0 .. I_{T-1}}``, ``ops.UncertaintyLayout``), per class, in fp64:
    ``dice_agreement = mean_t 2 I_t / (V_t + V)`` (each member against the consensus), ``iou_all = ALL / ANY``,
    ``volume_cv = pstdev_t(V_t) / mean_t(V_t)``, ``mean_entropy = HSUM / 2^20 / V``, ``voxels = V``.  A quantity is ``nan`` where
    its denominator is 0 (``dice_agreement``: where any member's is).  Pure host code; a device tensor is read back here."""
    from ..ops import UNCERTAIN_ENTROPY_SCALE, UncertaintyLayout
    lay = UncertaintyLayout(members)
    if hasattr(counts, "detach"):
        counts = counts.detach().cpu().numpy()
    c = np.asarray(counts)
    if c.dtype != np.int64:
        raise TypeError(f"structure_agreement: counts must be int64, got {c.dtype}")
    if c.ndim != 2 or c.shape[1] != lay.slots:
        raise ValueError(f"structure_agreement: counts must be [K, 2 T + 4] = [K, {lay.slots}] for {members} members, got {c.shape}")
    v = c[:, lay.V].astype(np.float64)
    vt, it = lay.member_voxels(c).astype(np.float64), lay.member_overlap(c).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = lambda a, b: np.where(b != 0, a / b, np.nan)
        dice = ratio(2.0 * it, vt + v[:, None]).mean(axis=1)
        iou = ratio(c[:, lay.ALL].astype(np.float64), c[:, lay.ANY].astype(np.float64))
        cv = ratio(vt.std(axis=1), vt.mean(axis=1))
        ent = ratio(c[:, lay.HSUM].astype(np.float64) / UNCERTAIN_ENTROPY_SCALE, v)
    return StructureAgreement(dice, iou, cv, ent, c[:, lay.V].copy())


def format_quality_csv(quality, names=None):
    """``quality.csv``: a header line (``QUALITY_COLUMNS``) and one line per class of a ``StructureAgreement``: the class (its
    index, or ``names[k]``), the voxel count, then the four scores as '%.6f' (``nan`` as Python formats it)."""
    k = len(quality.voxels)
    if names is not None and len(names) != k:
        raise ValueError(f"format_quality_csv: {len(names)} names for {k} classes")
    lines = [",".join(QUALITY_COLUMNS)]
    for i in range(k):
        scores = (quality.dice_agreement[i], quality.iou_all[i], quality.volume_cv[i], quality.mean_entropy[i])
        lines.append(",".join([str(i if names is None else names[i]), str(int(quality.voxels[i]))] + ["%.6f" % s for s in scores]))
    return "\n".join(lines) + "\n"


class Meter:
    """Running per-modality loss / dice with best tracking (utils.py:58-160), trimmed to what the trainers call."""

    def __init__(self, min_better_keys, max_better_keys, alpha=1.0):
        self.configs = OrderedDict([(k, "min") for k in min_better_keys] + [(k, "max") for k in max_better_keys])
        self.alpha = alpha
        self.best_values = self._zeros()
        self.pre_values = None
        self.cur_values = self._zeros()
        self.n = self._zeros()

    def _zeros(self):
        return {k: 0 for k in self.configs}

    @staticmethod
    def collect_loss_by(sample_loss, modal_id, n):
        k = "loss_" + str(modal_id)
        return {"loss": sample_loss * n, k: sample_loss * n}, {"loss": n, k: n}

    def __repr__(self):
        out = ""
        for k in self.configs:
            name = f"{k.split('_')[0]}_{cfg.Modality(int(k.split('_')[1])).name}" if "_" in k else k
            out += " %s: %.4f/%.4f," % (name, self.cur_values[k], self.best_values[k])
        return out

    def accumulate(self, values, n):
        for k, v in values.items():
            self.cur_values[k] += v
            self.n[k] += n[k]

    def update_cur(self, reset_best=False):
        for k in self.configs:
            if self.n[k] != 0:
                self.cur_values[k] /= self.n[k]
            if self.pre_values is not None:
                self.cur_values[k] = (1.0 - self.alpha) * self.pre_values[k] + self.alpha * self.cur_values[k]
        if self.pre_values is None or reset_best:
            self.best_values = deepcopy(self.cur_values)
            self.pre_values = deepcopy(self.cur_values)
        else:
            for k, f in self.configs.items():
                better = self.cur_values[k] < self.best_values[k] if f == "min" else self.cur_values[k] > self.best_values[k]
                if better:
                    self.best_values[k] = self.cur_values[k]
                self.pre_values[k] = self.cur_values[k]

    def reset_cur(self):
        self.cur_values = self._zeros()
        self.n = self._zeros()


class ScalarFetcher:
    """Per-iteration logging without stalling the device: the reference reads its loss scalars with ``.item()`` right after every
    iteration (trainer/uganConsisTrainer.py:148-149,157,183-188 -- 11 host syncs), which keeps the host from enqueueing iteration
    i + 1 while i runs.  Here the scalars of iteration i go to pinned host memory with a non-blocking copy and are HANDED OUT ONE
    ITERATION LATER (``push`` returns the previous item, whose copy has long finished); ``flush`` returns the last one.  Same values,
    same order -- the meter / log just see them one iteration late, and the device never waits for the host."""

    def __init__(self, numel: int, device, check_finite: bool = True):
        """``check_finite``: a NaN / Inf among the fetched scalars raises ``FloatingPointError`` naming the item's tag -- one
        iteration after it happened, but it happens: the kernels' own maxima (fmaxf) pass over NaNs silently."""
        import torch
        self._torch = torch
        self._check = check_finite
        self._bufs = [torch.empty(numel, dtype=torch.float32).pin_memory() if torch.device(device).type == "cuda"
                      else torch.empty(numel, dtype=torch.float32) for _ in range(2)]
        self._events = [None, None]
        self._tags = [None, None]
        self._cur = 0
        self._pending = None

    def _take(self, slot):
        if self._events[slot] is not None:
            self._events[slot].synchronize()
        vals = self._bufs[slot].tolist()
        if self._check and not all(v == v and abs(v) != float("inf") for v in vals):
            raise FloatingPointError(f"non-finite training scalars {vals} at {self._tags[slot]!r}")
        return vals, self._tags[slot]

    def push(self, scalars, tag=None):
        """Enqueue the device -> host copy of ``scalars`` (1-D float tensor); returns ``(values, tag)`` of the PREVIOUS push or None."""
        torch = self._torch
        prev = self._take(self._pending) if self._pending is not None else None
        slot = self._cur
        self._bufs[slot].copy_(scalars.detach().reshape(-1).float(), non_blocking=True)
        if scalars.is_cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(scalars.device))
            self._events[slot] = ev
        self._tags[slot] = tag
        self._pending, self._cur = slot, 1 - slot
        return prev

    def flush(self):
        if self._pending is None:
            return None
        out = self._take(self._pending)
        self._pending = None
        return out
