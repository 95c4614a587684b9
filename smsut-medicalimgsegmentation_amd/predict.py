"""Inference: one raw scan in, one label volume out.

    python -m smsut_amd.predict --trainer unet -i 000 --image scan.npy --spacing 5.0 1.5 1.5 --modality ct --tta flips --out out/

``Predictor`` runs a trained network (or an ensemble) over uint8 slices of the processed grid, with optional test-time augmentation:
the network sees the flipped / rotated copies of every slice (``ops.tta_expand``), and the class probabilities of all copies and all
networks are averaged on the un-transformed grid in one pass (``ops.tta_merge``, csrc/tta.hip).  ``predict_volume`` wraps it between
``prepare_volume`` (raw scanner array -> processed grid) and ``restore_labels`` (labels back on the scanner's grid), with the test
phase's 3-D connected-component cleanup in between.  ``field_of_view='full'`` / ``--field-of-view full`` labels the whole resampled
grid instead of its central 256 x 256 window: the network runs over overlapping windows (``Predictor.predict_windows``) whose class
probabilities are blended in one pass (``ops.window_blend``, csrc/window.hip).  ``uncertainty=True`` / ``--uncertainty`` adds, from the same pass over the
member logits (``ops.tta_uncertainty``, csrc/uncertainty.hip), per-voxel entropy, mutual information and vote count and the label-free
per-structure agreement scores (``misc.utils.structure_agreement``).  Everything stays on the device; reading DICOM / NIfTI is the caller's business
(``.npy`` in and out).  The reference has no inference entry point: its only path through a trained network is the test phase, which
needs a PNG tree, a split yaml and ground truth (trainer/baseTrainer.py:254-318).
"""
import argparse
import numbers
import os
import types
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import config as cfg
from . import ops
from .data_pprocess.volume import CROP_SIZE, FIELDS_OF_VIEW, NEW_SPACING, ResamplePlan, prepare_volume, restore_labels
from .misc.utils import StructureAgreement, format_quality_csv, structure_agreement


def group_plan(depth, batch_size):
    """How ``depth`` slices are cut into groups of ``batch_size``: a list of ``(start, count, padding)`` with ``count + padding ==
    batch_size``; only the last group is padded.  Pure host code."""
    depth, batch_size = int(depth), int(batch_size)
    if depth < 1 or batch_size < 1:
        raise ValueError(f"group_plan: needs at least one slice and a batch of at least one, got {depth} slices, batch {batch_size}")
    return [(s, min(batch_size, depth - s), batch_size - min(batch_size, depth - s)) for s in range(0, depth, batch_size)]


def _modules_of(forward):
    """The ``nn.Module`` s behind a forward callable, as far as they can be found: the callable itself, or, for a bound method of a
    trainer, its ``net`` / ``net2`` / ``ema``."""
    if isinstance(forward, torch.nn.Module):
        return [forward]
    owner = getattr(forward, "__self__", None)
    if isinstance(owner, torch.nn.Module):
        return [owner]
    return [m for m in (getattr(owner, a, None) for a in ("net", "net2", "ema")) if isinstance(m, torch.nn.Module)]


class Predictor:
    """``forward``: one callable ``img [B, 1, H, W] -> logits [B, C, H, W]`` (a trainer's ``_forward_eval``, a module) or a list of
    them (an ensemble: crossPse's two networks, mean-teacher's student and teacher).  ``tta``: a set name (``'none'``, ``'flips'``,
    ``'d4'``) or a list of transforms (``ops.tta_transforms``).  ``classes``: the leading channels that are classes (default: all;
    CoraNet: L + 1, head 0 of its 3L+1 channels).

    Slices are processed in groups of ``batch_size``: one ``tta_expand`` launch, one forward of ``batch_size`` images per (network,
    transform), one ``tta_merge`` launch.  The last group is padded with zero images to ``batch_size`` (as ``validate_epoch`` pads
    it: captured graphs are per shape) and the padding is dropped.  Working memory is one group's members, not the volume's; nothing
    is read back.  With one member and no confidence the prediction is ``ops.argmax_channels``' and the merge kernel does not run.

    ``temperature``: temperature scaling (``misc.utils.fit_temperature``; the ``temperature.txt`` of ``-p test`` with
    ``cfg.test_calibration``): one T for every forward, or one per forward of an ensemble.  A forward's logits are multiplied by the
    fp32 value of 1 / T (one elementwise launch per member) before ``ops.tta_merge``, which makes the averaged probabilities and
    the confidence those of the calibrated networks.  A forward whose T is None or 1 is left untouched: with no other T the path,
    and its output, are bit for bit those of a ``Predictor`` without the argument.  The one-member argmax is taken from the
    unscaled logits: a positive scale does not move it."""

    def __init__(self, forward, batch_size=None, tta="none", classes=None, temperature=None):
        self.forwards = list(forward) if isinstance(forward, (list, tuple)) else [forward]
        if not self.forwards or not all(callable(f) for f in self.forwards):
            raise TypeError("Predictor: forward must be a callable or a non-empty list of callables")
        self.batch_size = int(cfg.batch_size if batch_size is None else batch_size)
        if self.batch_size < 1:
            raise ValueError(f"Predictor: batch_size must be at least 1, got {batch_size}")
        self.transforms = ops.tta_transforms(tta)
        self.classes = None if classes is None else int(classes)
        self.members = len(self.forwards) * len(self.transforms)
        if isinstance(temperature, bool):
            raise TypeError("Predictor: temperature must be a number, a sequence of numbers or None, got a bool")
        if temperature is None or isinstance(temperature, numbers.Real):
            temperature = [temperature] * len(self.forwards)
        try:
            temperature = list(temperature)
        except TypeError:
            raise TypeError(f"Predictor: temperature must be a number, a sequence of numbers or None, got "
                            f"{type(temperature).__name__}") from None
        for t in temperature:
            if t is not None and (isinstance(t, bool) or not isinstance(t, numbers.Real)):
                raise TypeError(f"Predictor: a temperature must be a number or None, got {type(t).__name__}")
        if len(temperature) != len(self.forwards):
            raise ValueError(f"Predictor: {len(temperature)} temperatures for {len(self.forwards)} forwards")
        # per forward: None (untouched) or the fp32 inverse temperature its logits are multiplied by
        self.scales = [None if t is None or float(t) == 1.0 else ops.calibration_beta(t) for t in temperature]
        if self.members > ops.TTA_MAX_MEMBERS:
            raise ValueError(f"Predictor: {len(self.forwards)} networks x {len(self.transforms)} transforms = {self.members} members, "
                             f"at most {ops.TTA_MAX_MEMBERS}")

    def plan(self, depth):
        return group_plan(depth, self.batch_size)

    def predict_slices(self, image_u8, confidence=False):
        """``image_u8``: uint8 ``[D, H, W]`` on the device, the processed grid.  Returns ``(pred, conf)``: uint8 ``[D, H, W]`` and,
        with ``confidence``, the mean probability of the predicted class as fp32 ``[D, H, W]`` (else None), both on the device."""
        if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8:
            raise TypeError("predict_slices: image_u8 must be a uint8 tensor")
        if not image_u8.is_cuda:
            raise TypeError(f"predict_slices: image_u8 must be on a HIP device, got {image_u8.device} (no CPU fallback)")
        if image_u8.dim() != 3 or image_u8.shape[0] < 1:
            raise ValueError(f"predict_slices: expected [D >= 1, H, W] slices, got shape {tuple(image_u8.shape)}")
        d, h, w = image_u8.shape
        ops._tta_check_plane("predict_slices", self.transforms, h, w)
        image_u8 = image_u8.contiguous()
        for f in self.forwards:
            for m in _modules_of(f):
                m.eval()
        bs, tr = self.batch_size, self.transforms
        pred = torch.empty(d, h, w, dtype=torch.uint8, device=image_u8.device)
        conf = torch.empty(d, h, w, dtype=torch.float32, device=image_u8.device) if confidence else None
        with torch.no_grad():
            for start, count, padding in self.plan(d):
                x = ops.tta_expand(image_u8[start:start + count], tr)              # [T, count, 1, H, W]
                if padding:
                    full = torch.zeros(len(tr), bs, 1, h, w, dtype=torch.float32, device=x.device)
                    full[:, :count] = x
                    x = full
                outs = [f(x[t])[:count] for f in self.forwards for t in range(len(tr))]
                k = outs[0].shape[1] if self.classes is None else self.classes
                if len(outs) == 1 and not confidence and k == outs[0].shape[1]:
                    pred[start:start + count] = ops.argmax_channels(outs[0])
                else:
                    if any(s is not None for s in self.scales):
                        scale = [s for s in self.scales for _ in range(len(tr))]
                        outs = [o if s is None else o * s for o, s in zip(outs, scale)]
                    p, c, _ = ops.tta_merge(outs, tr * len(self.forwards), classes=k, want_conf=confidence)
                    pred[start:start + count] = p
                    if confidence:
                        conf[start:start + count] = c
        return pred, conf

    def predict_windows(self, image_u8, window, overlap=0.5, blend="gaussian", confidence=False):
        """Sliding-window inference over slices larger than the networks' training size.  ``image_u8``: uint8 ``[D, H, W]`` on the
        device with ``H, W >= window``; the networks see square ``window x window`` tiles at the origins of ``ops.window_plan(H |
        W, window, overlap)`` (square, so every transform set keeps working), and the tiles' class probabilities are blended on the
        ``H x W`` grid with the importance map ``blend`` (``ops.window_weights``: ``'gaussian'`` or ``'constant'``) in one pass
        (``ops.window_blend``, csrc/window.hip).  Returns ``(pred, conf)`` as ``predict_slices``.

        Slices are grouped, and the last group padded, as in ``predict_slices``.  Per group and per tile: ``tta_expand`` of the
        tile's slices, the forwards, the temperature scales, ``tta_merge(want_prob=True)`` -- for one member too, whose mean over
        T = 1 is its softmax -- then one ``window_blend`` per group.  Working memory is one group's tiles; nothing is read back.
        With one tile (the grid is the window) ``pred`` and ``conf`` are bitwise those of ``predict_slices(confidence=True)``."""
        if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8:
            raise TypeError("predict_windows: image_u8 must be a uint8 tensor")
        if image_u8.dim() != 3 or image_u8.shape[0] < 1:
            raise ValueError(f"predict_windows: expected [D >= 1, H, W] slices, got shape {tuple(image_u8.shape)}")
        if isinstance(window, bool) or not isinstance(window, numbers.Integral):
            raise TypeError(f"predict_windows: window must be an integer, got {window!r}")
        d, h, w = image_u8.shape
        win = int(window)
        if not 1 <= win <= min(h, w):
            raise ValueError(f"predict_windows: needs 1 <= window <= H, W, got window {win} on slices of {h} x {w}")
        ys, xs = ops.window_plan(h, win, overlap), ops.window_plan(w, win, overlap)
        if len(ys) * len(xs) > ops.WINDOW_MAX_TILES:
            raise ValueError(f"predict_windows: {len(ys)} x {len(xs)} windows of {win} at overlap {overlap} on {h} x {w}, at most "
                             f"{ops.WINDOW_MAX_TILES}")
        if blend not in ops.WINDOW_BLENDS:
            raise ValueError(f"predict_windows: unknown blend {blend!r}; expected one of {list(ops.WINDOW_BLENDS)}")
        ops._tta_check_plane("predict_windows", (), h, w)                   # (the tiles are square: any transform fits them)
        if not image_u8.is_cuda:
            raise TypeError(f"predict_windows: image_u8 must be on a HIP device, got {image_u8.device} (no CPU fallback)")
        image_u8 = image_u8.contiguous()
        for f in self.forwards:
            for m in _modules_of(f):
                m.eval()
        bs, tr, dev = self.batch_size, self.transforms, image_u8.device
        weights = ops.window_weights(win, blend, dev)
        pred = torch.empty(d, h, w, dtype=torch.uint8, device=dev)
        conf = torch.empty(d, h, w, dtype=torch.float32, device=dev) if confidence else None
        scale = [s for s in self.scales for _ in range(len(tr))]
        with torch.no_grad():
            for start, count, padding in self.plan(d):
                tiles = []
                for y0 in ys:
                    for x0 in xs:
                        x = ops.tta_expand(image_u8[start:start + count, y0:y0 + win, x0:x0 + win], tr)   # [T, count, 1, win, win]
                        if padding:
                            full = torch.zeros(len(tr), bs, 1, win, win, dtype=torch.float32, device=dev)
                            full[:, :count] = x
                            x = full
                        outs = [f(x[t])[:count] for f in self.forwards for t in range(len(tr))]
                        k = outs[0].shape[1] if self.classes is None else self.classes
                        outs = [o if s is None else o * s for o, s in zip(outs, scale)]
                        tiles.append(ops.tta_merge(outs, tr * len(self.forwards), classes=k, want_prob=True)[2])
                p, c, _ = ops.window_blend(tiles, ys, xs, (h, w), weights, weights, want_conf=confidence)
                pred[start:start + count] = p
                if confidence:
                    conf[start:start + count] = c
        return pred, conf

    def predict_uncertain(self, image_u8):
        """``predict_slices(confidence=True)`` with the uncertainty of the prediction (``ops.tta_uncertainty``): returns
        ``UncertainSlices(pred, conf, entropy, mutual_info, votes, counts)``, the maps ``[D, H, W]`` on the device and ``counts``
        the int64 ``[classes, 2 members + 4]`` agreement counts of the whole volume (``misc.utils.structure_agreement``).  Same
        grouping, padding of the last group and trimming as ``predict_slices``; one ``tta_uncertainty`` call per group, also for
        one member (whose entropy is then the network's own, with ``mutual_info`` 0 and ``votes`` 1); the padded slices never
        reach it, so they count nowhere.  ``pred`` and ``conf`` are bitwise those of ``predict_slices(confidence=True)``."""
        if not isinstance(image_u8, torch.Tensor) or image_u8.dtype != torch.uint8:
            raise TypeError("predict_uncertain: image_u8 must be a uint8 tensor")
        if not image_u8.is_cuda:
            raise TypeError(f"predict_uncertain: image_u8 must be on a HIP device, got {image_u8.device} (no CPU fallback)")
        if image_u8.dim() != 3 or image_u8.shape[0] < 1:
            raise ValueError(f"predict_uncertain: expected [D >= 1, H, W] slices, got shape {tuple(image_u8.shape)}")
        d, h, w = image_u8.shape
        ops._tta_check_plane("predict_uncertain", self.transforms, h, w)
        image_u8 = image_u8.contiguous()
        for f in self.forwards:
            for m in _modules_of(f):
                m.eval()
        bs, tr, dev = self.batch_size, self.transforms, image_u8.device
        pred, votes = (torch.empty(d, h, w, dtype=torch.uint8, device=dev) for _ in range(2))
        conf, entropy, mutual = (torch.empty(d, h, w, dtype=torch.float32, device=dev) for _ in range(3))
        counts = None
        with torch.no_grad():
            for start, count, padding in self.plan(d):
                x = ops.tta_expand(image_u8[start:start + count], tr)              # [T, count, 1, H, W]
                if padding:
                    full = torch.zeros(len(tr), bs, 1, h, w, dtype=torch.float32, device=dev)
                    full[:, :count] = x
                    x = full
                outs = [f(x[t])[:count] for f in self.forwards for t in range(len(tr))]
                k = outs[0].shape[1] if self.classes is None else self.classes
                if counts is None:
                    counts = torch.zeros(k, ops.UncertaintyLayout(self.members).slots, dtype=torch.int64, device=dev)
                if any(s is not None for s in self.scales):
                    scale = [s for s in self.scales for _ in range(len(tr))]
                    outs = [o if s is None else o * s for o, s in zip(outs, scale)]
                u = ops.tta_uncertainty(outs, tr * len(self.forwards), classes=k, counts=counts)
                for whole, part in zip((pred, conf, entropy, mutual, votes), u):
                    whole[start:start + count] = part
        return UncertainSlices(pred, conf, entropy, mutual, votes, counts)


class UncertainSlices(NamedTuple):
    pred: torch.Tensor                         # uint8 [D, H, W]
    conf: torch.Tensor                         # fp32 [D, H, W]: the mean probability of the predicted class
    entropy: torch.Tensor                      # fp32 [D, H, W]: the entropy of the mean probabilities (nat)
    mutual_info: torch.Tensor                  # fp32 [D, H, W]: the members' disagreement (BALD)
    votes: torch.Tensor                        # uint8 [D, H, W]: the members whose own label is the prediction
    counts: torch.Tensor                       # int64 [classes, 2 members + 4] (ops.UncertaintyLayout)


class PredictResult(NamedTuple):
    labels: torch.Tensor                       # uint8: on the scanner's grid when restored, else the processed grid
    labels_processed: torch.Tensor             # uint8 [new_z, crop, crop] (field_of_view='full': plan.new_size): the processed grid, after the cleanup
    confidence: Optional[torch.Tensor]         # fp32, processed grid, or None
    plan: ResamplePlan


class UncertainResult(NamedTuple):
    labels: torch.Tensor                       # as PredictResult
    labels_processed: torch.Tensor
    confidence: Optional[torch.Tensor]
    plan: ResamplePlan
    entropy: torch.Tensor                      # fp32, processed grid: the entropy of the mean probabilities (nat)
    mutual_info: torch.Tensor                  # fp32, processed grid: the members' disagreement (BALD)
    votes: torch.Tensor                        # uint8, processed grid: the members whose own label is the prediction
    quality: StructureAgreement                # per class, from the prediction BEFORE the cleanup (misc.utils.structure_agreement)
    counts: torch.Tensor                       # int64 [classes, 2 members + 4], on the device: what ``quality`` was computed from


def predict_volume(predictor, image, spacing, modality, cleanup=True, restore=True, confidence=False, new_spacing=NEW_SPACING,
                   crop_size=CROP_SIZE, uncertainty=False, field_of_view="crop", overlap=0.5, blend="gaussian"):
    """Raw ``image`` ``[D, H, W]`` (NumPy array or device tensor, any real dtype) with voxel ``spacing`` ``(sz, sy, sx)`` ->
    ``PredictResult``: ``prepare_volume`` -> ``predictor.predict_slices`` -> the test phase's 3-D 18-neighbour connected-component
    cleanup (``cleanup``) -> ``restore_labels`` onto the input's grid (``restore``).  The confidence stays on the processed grid.

    ``uncertainty``: the slices go through ``predictor.predict_uncertain`` instead and the result is an ``UncertainResult``: the
    same four fields (the same labels, bit for bit), the entropy, mutual-information and vote maps on the processed grid, and
    ``quality``, the label-free per-structure scores.  The maps, the counts and ``quality`` describe the prediction BEFORE the
    connected-component cleanup: the members' agreement on what the networks said, not on what the cleanup kept.

    ``field_of_view``: ``'crop'`` (the default) predicts the central ``crop_size`` window of the resampled grid, the training
    preprocessing, and ``labels`` is 0 outside it.  ``'full'`` predicts the whole resampled grid by sliding windows of ``crop_size``
    (``predictor.predict_windows`` with ``overlap`` and ``blend``): ``labels_processed`` and ``confidence`` are on the full grid,
    ``plan`` is the full plan.  Not together with ``uncertainty`` (``ValueError``): the per-member maps across tiles are not built."""
    if field_of_view not in FIELDS_OF_VIEW:
        raise ValueError(f"predict_volume: field_of_view must be one of {list(FIELDS_OF_VIEW)}, got {field_of_view!r}")
    if uncertainty and field_of_view == "full":
        raise ValueError("predict_volume: uncertainty=True is not available with field_of_view='full'")
    image_u8, _, plan = prepare_volume(image, None, spacing, modality, new_spacing=new_spacing, crop_size=crop_size,
                                       field_of_view=field_of_view)
    if field_of_view == "full":
        pred, conf = predictor.predict_windows(image_u8, int(crop_size), overlap=overlap, blend=blend, confidence=confidence)
    elif uncertainty:
        u = predictor.predict_uncertain(image_u8)
        pred, conf = u.pred, (u.conf if confidence else None)
    else:
        pred, conf = predictor.predict_slices(image_u8, confidence=confidence)
    if cleanup:
        pred = ops.cc_filter(pred, cfg.n_modal, per_slice=False)
    labels = restore_labels(pred, plan, tuple(image.shape)) if restore else pred
    if uncertainty:
        return UncertainResult(labels, pred, conf, plan, u.entropy, u.mutual_info, u.votes,
                               structure_agreement(u.counts, predictor.members), u.counts)
    return PredictResult(labels, pred, conf, plan)


TRAINERS = {"unet": ("unetTrainer", "UnetTrainer"), "crossPse": ("crossPseTrainer", "crossPseTrainer"),
            "meanTeacher": ("meanTeacherTrainer", "meanTeacherTrainer"), "coraNet": ("coraNetTrainer", "coraNetTrainer"),
            "dtc": ("dtcTrainer", "dtcTrainer"), "ugan": ("uganTrainer", "UGANTrainer"),
            "uganShp0": ("uganShp0Trainer", "UGANShp0Trainer"), "uganConsis": ("uganConsisTrainer", "UGANConsisTrainer")}


def make_parser():
    p = argparse.ArgumentParser(prog="python -m smsut_amd.predict", description="Segment one raw scan with a trained model.")
    p.add_argument("--trainer", required=True, choices=sorted(TRAINERS), help="the method the model was trained with")
    p.add_argument("-nm", "--expr_name", type=str, help="the run directory's name under config.expr_root (default: the trainer's class)")
    p.add_argument("-i", "--model_id", type=str, required=True)
    p.add_argument("-wh", "--which_ckpt", type=str, default="last")
    p.add_argument("--image", required=True, help="the raw volume [D, H, W] as .npy")
    p.add_argument("--spacing", type=float, nargs=3, required=True, metavar=("SZ", "SY", "SX"))
    p.add_argument("--modality", required=True, help="'ct' windows to [-1000, 400]; any other name to the 0.05 / 99.5 percentiles")
    p.add_argument("--tta", default="none", choices=sorted(ops.TTA_SETS))
    p.add_argument("--confidence", action="store_true", help="also write confidence.npy (processed grid)")
    p.add_argument("--uncertainty", action="store_true", help="also write entropy.npy, mutual_information.npy, votes.npy (processed "
                   "grid) and quality.csv: label-free agreement scores per structure")
    p.add_argument("--temperature", default=None, help="temperature scaling of the probabilities: a number, or the path of the "
                   "temperature.txt that -p test writes with config.test_calibration")
    p.add_argument("--field-of-view", dest="field_of_view", default="crop", choices=list(FIELDS_OF_VIEW),
                   help="'crop' labels the central 256 x 256 window of the resampled grid (0 outside it); 'full' labels the whole "
                   "grid by blended sliding windows")
    p.add_argument("--overlap", type=float, default=0.5, help="--field-of-view full: the windows' overlap, 0 <= overlap < 1")
    p.add_argument("--blend", default="gaussian", choices=list(ops.WINDOW_BLENDS), help="--field-of-view full: the windows' "
                   "importance map")
    p.add_argument("--batch_size", type=int, default=None)
    p.add_argument("--out", required=True, help="directory for labels.npy, labels_processed.npy (and confidence.npy, and the files of "
                   "--uncertainty)")
    return p


def read_temperature(arg):
    """``--temperature``: None, a number, or the path of a file whose first word is one (``temperature.txt``)."""
    if arg is None:
        return None
    try:
        return float(arg)
    except ValueError:
        pass
    with open(arg) as f:
        words = f.read().split()
    if not words:
        raise ValueError(f"--temperature: {arg} is empty")
    return float(words[0])


def write_uncertainty(out_dir, res):
    """``--uncertainty``: the three maps of an ``UncertainResult`` as .npy and its ``quality`` as quality.csv"""
    np.save(os.path.join(out_dir, "entropy.npy"), res.entropy.cpu().numpy())
    np.save(os.path.join(out_dir, "mutual_information.npy"), res.mutual_info.cpu().numpy())
    np.save(os.path.join(out_dir, "votes.npy"), res.votes.cpu().numpy())
    with open(os.path.join(out_dir, "quality.csv"), "w") as f:
        f.write(format_quality_csv(res.quality))


def trainer_forwards(trainer):
    """The eval forwards of a trainer built in its test phase and loaded with ``load_model``: its ``_forward_eval``.  A checkpoint
    here holds ``net`` alone -- crossPse's ``net2`` and the teachers are never saved with it, as in the reference -- so the
    command line has one network to wrap; an ensemble of separately loaded networks goes through ``Predictor([f1, f2], ...)``."""
    return [trainer._forward_eval]


def main(argv=None):
    args = make_parser().parse_args(argv)
    import importlib
    mod, cls = TRAINERS[args.trainer]
    trainer_cls = getattr(importlib.import_module(f"{__package__}.trainer.{mod}"), cls)
    t = trainer_cls("test", types.SimpleNamespace(fold=0, expr_name=args.expr_name, model_id=args.model_id, write_env=False))
    t.load_model(args.model_id, args.which_ckpt)
    t.net.to(t.device)
    predictor = Predictor(trainer_forwards(t), batch_size=args.batch_size, tta=args.tta, classes=cfg.n_label + 1,
                          temperature=read_temperature(args.temperature))
    image = np.load(args.image)
    res = predict_volume(predictor, image, tuple(args.spacing), args.modality, confidence=args.confidence,
                         uncertainty=args.uncertainty, field_of_view=args.field_of_view, overlap=args.overlap, blend=args.blend)
    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "labels.npy"), res.labels.cpu().numpy())
    np.save(os.path.join(args.out, "labels_processed.npy"), res.labels_processed.cpu().numpy())
    if args.confidence:
        np.save(os.path.join(args.out, "confidence.npy"), res.confidence.cpu().numpy())
    if args.uncertainty:
        write_uncertainty(args.out, res)
    return res


if __name__ == "__main__":
    main()
