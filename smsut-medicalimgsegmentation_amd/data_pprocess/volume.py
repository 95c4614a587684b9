"""Raw volume -> processed dataset, on the device (the reference's data_pprocess/chaosPreparation.py:71-100,
atlasPreparation.py:63-92 and toPngAndSplit.py:34-61, without SimpleITK): resample to a common spacing with a cubic B-spline
(labels: nearest neighbour), centre-crop in plane, window to 8 bits, write the PNG tree ``BalanceDataset`` and the test phase read;
and the way back, ``restore_labels``, which puts a processed-grid label volume onto the scanner's grid.

Arrays are ``[D, H, W]`` = ``[z, y, x]``, spacings ``(sz, sy, sx)`` as for ``test_spacing``.  Reading DICOM / NIfTI is the caller's
business: inputs are NumPy arrays or tensors.

Index map (the single definition; csrc/volume.hip evaluates it in fp64): output index ``i`` of an axis reads the input at
``x = ((i + start) * old) / new``; the point is inside iff ``-0.5 <= x < old - 0.5`` on every axis, outside points are 0 (ITK's
same-origin resampling with its default pixel value).  The inverse, for ``restore_labels``: ``x = (j * new) / old - start``.
"""
import math
import os
from os.path import join as pjoin
from typing import NamedTuple, Tuple

import numpy as np
import torch

from .. import ops

NEW_SPACING = (5.0, 1.5, 1.5)          # (sz, sy, sx) mm: the reference's config.new_spacing (1.5, 1.5, 5) in array order
CROP_SIZE = 256
CT_WINDOW = (-1000.0, 400.0)           # toPngAndSplit.py:35
MR_PERCENTILES = (0.05, 99.5)          # toPngAndSplit.py:37


class ResamplePlan(NamedTuple):
    new_size: Tuple[int, int, int]     # the full resampled grid (z, y, x)
    spacing: Tuple[float, float, float]  # its voxel spacing: what ``test_spacing`` takes
    start: Tuple[int, int, int]        # first index of the cropped window on the resampled grid
    out_size: Tuple[int, int, int]     # the cropped window (new_z, crop, crop)


_check_size = ops._vol_size            # three axes of 1..4096, at most 2^31 - 1 voxels: the kernels' own limits


def _check_spacing(spacing):
    try:
        return ops.check_spacing(spacing, 3)
    except RuntimeError as e:
        raise ValueError(str(e)) from None


def resample_plan(old_size, old_spacing, new_spacing=NEW_SPACING, crop_size=CROP_SIZE):
    """The grid ``prepare_volume`` resamples to (chaosPreparation.py:76-99).  Per axis ``new = int(old * old_sp / new_sp)``, in
    plane ``max(crop_size, new)``; ``spacing = old_sp * old / new``; ``start = (new - crop_size) // 2`` in plane, 0 on z;
    ``out_size = (new_z, crop_size, crop_size)``.  Pure host code.  ``ValueError`` for ``new_z == 0``, a spacing that is not finite
    and positive, an axis outside 1..4096 or more than 2^31 - 1 voxels (in, resampled or out)."""
    old = _check_size("old_size", old_size)
    osp, nsp = _check_spacing(old_spacing), _check_spacing(new_spacing)
    crop = int(crop_size)
    if not 1 <= crop <= ops.VOL_MAX_DIM:
        raise ValueError(f"crop_size must lie in 1..{ops.VOL_MAX_DIM}, got {crop_size}")
    new = [int(o * a / b) for o, a, b in zip(old, osp, nsp)]
    if new[0] == 0:
        raise ValueError(f"the resampled volume has no slice: {old[0]} slices of {osp[0]} mm at {nsp[0]} mm")
    new[1], new[2] = max(crop, new[1]), max(crop, new[2])
    new = _check_size("new_size", new)
    out = _check_size("out_size", (new[0], crop, crop))
    spacing = tuple(a * o / n for a, o, n in zip(osp, old, new))
    start = (0, (new[1] - crop) // 2, (new[2] - crop) // 2)
    return ResamplePlan(new, spacing, start, out)


def _device_tensor(what, a, dtype):
    """A NumPy array is uploaded; a tensor must already be on the device (a CPU tensor is not moved silently)."""
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if not isinstance(a, torch.Tensor) or a.dim() != 3:
        raise ValueError(f"{what}: expected a [D, H, W] array or tensor")
    return a.to(dtype)


def window_bounds(vol, modality):
    """The 2-float device tensor ``(lo, hi)`` of toPngAndSplit.py:34-40 for the fp32 device tensor ``vol``.  ``'ct'``:
    ``(max(min v, -1000), min(max v, 400))``; any other modality: the 0.05 and 99.5 percentiles by NumPy's linear rule (ranks
    ``floor(t)`` and ``min(floor(t) + 1, n - 1)`` of ``t = q / 100 * (n - 1)``, interpolated in fp64 on the device, rounded once to
    fp32).  The order statistics are exact; nothing is read back."""
    n = vol.numel()
    if modality == "ct":
        v = ops.order_statistics(vol, [0, n - 1])
        lo, hi = CT_WINDOW
        return torch.stack([v[0].clamp(min=lo), v[1].clamp(max=hi)])
    ranks, frac = [], []
    for q in MR_PERCENTILES:
        t = q / 100.0 * (n - 1)
        lo = min(int(math.floor(t)), n - 1)
        ranks += [lo, min(lo + 1, n - 1)]
        frac.append(t - lo)
    v = ops.order_statistics(vol, ranks).double().view(2, 2)
    f = torch.tensor(frac, dtype=torch.float64, device=vol.device)
    a, b = v[:, 0], v[:, 1]
    d = b - a
    return torch.where(f >= 0.5, b - d * (1.0 - f), a + d * f).float()         # numpy's _lerp


FIELDS_OF_VIEW = ("crop", "full")


def prepare_volume(image, label, spacing, modality, new_spacing=NEW_SPACING, crop_size=CROP_SIZE, label_lut=None,
                   field_of_view="crop"):
    """Raw ``image`` (any real dtype) and ``label`` (uint8, or None) ``[D, H, W]`` with voxel ``spacing`` -> ``(image_u8, label_u8,
    plan)``: both ``[new_z, crop, crop]`` uint8 on the device (``label_u8`` None without a label), ``plan`` the ``ResamplePlan``
    (``plan.spacing`` is what ``test_spacing`` takes).  ``label_lut``: 256 uint8 entries applied to the raw label values while
    they are resampled (CHAOS' grey ranges -> classes, BTCV's label list).

    ``field_of_view``: ``'crop'`` is the reference's training preprocessing, the central ``crop_size`` window.  ``'full'`` returns
    the whole resampled grid ``plan.new_size`` and a plan with ``start = (0, 0, 0)`` and ``out_size = new_size``, with which
    ``restore_labels`` forces no zeros.  The 8-bit window bounds are still those of the central ``crop_size`` window (the intensity
    mapping the network was trained with), applied to the whole grid; the index map is a function of ``i + start``, so the central
    window of the full image is the cropped output."""
    if field_of_view not in FIELDS_OF_VIEW:
        raise ValueError(f"prepare_volume: field_of_view must be one of {list(FIELDS_OF_VIEW)}, got {field_of_view!r}")
    img = _device_tensor("image", image, torch.float32)
    plan = resample_plan(tuple(img.shape), spacing, new_spacing, crop_size)
    crop = plan
    if field_of_view == "full":
        plan = ResamplePlan(plan.new_size, plan.spacing, (0, 0, 0), plan.new_size)
    old = tuple(img.shape)
    vol = ops.resample_volume(ops.bspline_coefficients(img), plan.out_size, old, plan.new_size, plan.start)
    label_u8 = None
    if label is not None:
        lab = _device_tensor("label", label, torch.uint8)
        if tuple(lab.shape) != old:
            raise ValueError(f"label shape {tuple(lab.shape)} differs from the image's {old}")
        lut = None
        if label_lut is not None:
            if not isinstance(label_lut, torch.Tensor):
                label_lut = torch.from_numpy(np.asarray(label_lut, dtype=np.uint8).reshape(256))
            lut = label_lut.to(device=lab.device, dtype=torch.uint8)
        label_u8 = ops.resample_labels(lab, plan.out_size, old, plan.new_size, plan.start, lut=lut)
    (_, sy, sx), (_, ch, cw) = crop.start, crop.out_size
    central = vol if plan is crop else vol[:, sy:sy + ch, sx:sx + cw].contiguous()
    image_u8 = ops.window_u8(vol, window_bounds(central, modality))
    return image_u8, label_u8, plan


def restore_labels(pred_u8, plan, old_size):
    """A label volume on the processed grid (``plan.out_size``) back on the native grid ``old_size`` by the inverse map
    ``x = (j * new) / old - start``: nearest neighbour, 0 outside the plan's window (the crop; with a
    ``field_of_view='full'`` plan the whole resampled grid)."""
    old = _check_size("old_size", old_size)
    pred = _device_tensor("pred_u8", pred_u8, torch.uint8)
    if tuple(pred.shape) != tuple(plan.out_size):
        raise ValueError(f"pred_u8 has shape {tuple(pred.shape)}, the plan's window is {tuple(plan.out_size)}")
    return ops.resample_labels(pred, old, plan.new_size, old, (0, 0, 0), offset=plan.start)


def chaos_label_lut():
    """CHAOS' grey ranges -> classes 1..4 (chaosPreparation.py:25-29, 60-63) as a 256-entry table."""
    lut = np.zeros(256, dtype=np.uint8)
    for cls, (lo, hi) in enumerate(((55, 70), (110, 135), (175, 200), (240, 255)), start=1):
        lut[lo:hi + 1] = cls
    return lut


def write_slices(image_u8, label_u8, dst, modality, pid):
    """The tree ``BalanceDataset`` and the test phase read (toPngAndSplit.py:42-61): ``<dst>/<modality>/<pid>/images/
    <modality>_<pid>_<zzz>.png``, the same under ``labels/``, and the label volume ``<dst>/<modality>/<pid>/<modality>_<pid>.npy``.
    The one host transfer of the pipeline, once per volume."""
    from PIL import Image
    img = image_u8.cpu().numpy() if isinstance(image_u8, torch.Tensor) else np.asarray(image_u8)
    lab = label_u8.cpu().numpy() if isinstance(label_u8, torch.Tensor) else np.asarray(label_u8)
    if img.dtype != np.uint8 or lab.dtype != np.uint8 or img.ndim != 3 or img.shape != lab.shape:
        raise ValueError(f"write_slices: expected two uint8 [D, H, W] volumes of one shape, got {img.dtype} {img.shape} and "
                         f"{lab.dtype} {lab.shape}")
    pid = str(pid)
    root = pjoin(dst, modality, pid)
    os.makedirs(pjoin(root, "images"), exist_ok=True)
    os.makedirs(pjoin(root, "labels"), exist_ok=True)
    np.save(pjoin(root, f"{modality}_{pid}.npy"), lab)
    for z in range(img.shape[0]):
        name = f"{modality}_{pid}_{z:03d}.png"
        Image.fromarray(img[z]).save(pjoin(root, "images", name))
        Image.fromarray(lab[z]).save(pjoin(root, "labels", name))
    return root
