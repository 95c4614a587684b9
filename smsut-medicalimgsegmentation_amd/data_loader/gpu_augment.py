"""Joint geometric augmentation on the device: the reference runs JointRotate(+-15 deg),
JointElasticDeform(sigma 9-13, 3x3 control points, p = 0.5) and JointRandomResizedCrop(size, scale 0.6-1.0,
ratio 3/4-4/3) per slice in PIL worker processes (data_loader/externalTransforms.py:45-90, config.py:60-71, order:
baseLoader.py:92-98); at thousands of slices per second per GPU that does not keep up, so they run as device passes per batch.

r04: the passes follow the reference's own structure.  When no slice of the batch drew the elastic deformation, rotation and crop
are composed into ONE bilinear / nearest resampling (``smsut_warp_joint``; pinned to PIL's rotate -> crop + resize outputs,
tests/golden/augment_pil.npz).  When one did, the batch takes the reference's three steps: rotate (bilinear image, nearest labels,
values rounded to the 8-bit grid as PIL stores them), ``elasticdeform.deform_random_grid(order=[0, 0])`` restated
(``smsut_elastic_deform``: cubic-B-spline interpolation of the P x P control displacements, ORDER-0 sampling of image AND labels,
zeros outside -- slices that did not draw it carry zero displacements, an exact copy), crop + resize.  Out-of-image samples read 0 =
black on the [0, 1] scale the passes run on (ToTensor's range; Normalize(0.5, 0.5) comes after, as in baseLoader.py:104-108).

Parameter draws follow the reference's distributions (uniform angle; torchvision's RandomResizedCrop.get_params: up to
10 tries of area ~ U(scale) * HW and log-uniform aspect ratio, central fallback; elastic control offsets ~ N(0, sigma)
with sigma ~ U(sigmas), applied with probability p).  ``elasticdeform`` is a third-party package that is not installed here (and
not pinned by the reference): its published algorithm is restated (oracle/augment_oracle.py::elastic_deform_grid builds it from
scipy.ndimage's spline routines, the code elasticdeform's C extension derives from); parity at that boundary is UNPINNED.

The photometric half (``colorJitter`` / ``gammaCorrect``, baseLoader.py:102-109) follows the joint passes: ``GpuPhotometricAugment`` /
``photometric`` below, two launches per batch (``csrc/photometric.hip``), pinned bit for bit to Pillow (tests/golden/photometric_pil.npz).
"""
import math
import random

import numpy as np
import torch

from .. import _hip as H


def spline_prefilter(ctrl):
    """Cubic B-spline coefficients of control values along the last two axes, mirror boundary (what
    ``scipy.ndimage.spline_filter1d(order=3, mode='mirror')`` computes along each axis, which is how elasticdeform's ``deform_grid``
    prefilters its displacement grid): after it, the spline through the coefficients INTERPOLATES the control values.  Host side
    (P x P values per slice); float64 inside.  ``ctrl`` [..., P, P] tensor -> same shape, float32."""
    c = np.asarray(ctrl, dtype=np.float64).copy()
    z = math.sqrt(3.0) - 2.0                                   # the pole of the cubic B-spline filter
    for ax in (-2, -1):
        c = np.moveaxis(c, ax, -1)
        n = c.shape[-1]
        if n > 1:
            c = c * ((1.0 - z) * (1.0 - 1.0 / z))              # gain
            # causal initialisation: sum over the mirrored signal, exact for short lines
            zn = z ** (n - 1)
            acc = c[..., 0] + zn * c[..., n - 1]
            z1, z2 = z, zn * zn / z
            for k in range(1, n - 1):
                acc = acc + (z1 + z2) * c[..., k]
                z1, z2 = z1 * z, z2 / z
            c[..., 0] = acc / (1.0 - zn * zn)
            for k in range(1, n):
                c[..., k] = c[..., k] + z * c[..., k - 1]
            c[..., n - 1] = (z / (z * z - 1.0)) * (c[..., n - 1] + z * c[..., n - 2])
            for k in range(n - 2, -1, -1):
                c[..., k] = z * (c[..., k + 1] - c[..., k])
        c = np.moveaxis(c, -1, ax)
    return torch.from_numpy(c.astype(np.float32))


def resized_crop_params(height, width, scale=(0.6, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """torchvision.transforms.RandomResizedCrop.get_params (as called by externalTransforms.py:51): (i, j, h, w)."""
    area = height * width
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    for _ in range(10):
        target_area = area * random.uniform(scale[0], scale[1])
        aspect = math.exp(random.uniform(log_ratio[0], log_ratio[1]))
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= width and 0 < h <= height:
            return random.randint(0, height - h), random.randint(0, width - w), h, w
    in_ratio = float(width) / float(height)                    # fallback: central crop
    if in_ratio < min(ratio):
        w, h = width, int(round(width / min(ratio)))
    elif in_ratio > max(ratio):
        h, w = height, int(round(height * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def affine_for(angle_deg, crop, in_hw, out_hw):
    """2x3 matrix mapping an OUTPUT pixel (xo, yo) to SOURCE coordinates: output grid -> crop window (i, j, h, w) of the
    rotated image -> rotate by ``angle`` about the image centre back into the source image."""
    (i, j, h, w), (H_, W_), (Ho, Wo) = crop, in_hw, out_hw
    sx, sy = w / Wo, h / Ho                                      # pixel-centre aligned resize (PIL box resampling model)
    # position in the rotated image: xr = j + (xo + 0.5) * sx - 0.5
    cx, cy = (W_ - 1) / 2.0, (H_ - 1) / 2.0
    a = math.radians(angle_deg)
    ca, sa = math.cos(a), math.sin(a)
    # source = R(a) * (pr - c) + c, with pr = (xr, yr)
    bx, by = j + 0.5 * sx - 0.5 - cx, i + 0.5 * sy - 0.5 - cy
    return [ca * sx, -sa * sy, ca * bx - sa * by + cx,
            sa * sx, ca * sy, sa * bx + ca * by + cy]


class GpuJointAugment:
    def __init__(self, data_aug, out_size):
        self.cfg = dict(data_aug or {})
        self.out = int(self.cfg.get("resizeCrop_size", out_size)) if self.cfg.get("resizeCrop") else None
        self.points = int(self.cfg.get("elasticDeform_points", 3))

    def draw(self, n, in_hw):
        """Per-sample parameters (host RNG, reference draw order per sample: rotate, elastic, crop): (angles, crops, control
        displacements [n, 2, P, P] or None when no slice drew the deformation, output size)."""
        H_, W_ = in_hw
        out_hw = (self.out, self.out) if self.out else in_hw
        angs, crops, ctrl, any_el = [], [], [], False
        P = self.points
        for _ in range(n):
            ang = random.uniform(-self.cfg["rotate_degrees"], self.cfg["rotate_degrees"]) if self.cfg.get("rotate") else 0.0
            c = torch.zeros(2, P, P)
            if self.cfg.get("elasticDeform"):
                s = random.uniform(*self.cfg["elasticDeform_sigmas"])            # externalTransforms.py:80 (drawn before the coin)
                if random.random() < 0.5:
                    c = torch.tensor([[[random.gauss(0.0, s) for _ in range(P)] for _ in range(P)] for _ in range(2)])
                    any_el = True
            crops.append(resized_crop_params(H_, W_) if self.cfg.get("resizeCrop") else (0, 0, H_, W_))
            angs.append(ang)
            ctrl.append(c)
        return angs, crops, (torch.stack(ctrl) if any_el else None), out_hw

    def __call__(self, img, msk=None, params=None):
        """img [N,1,H,W] on the [0, 1] scale (zeros = black outside the image), msk [N,H,W] int64 or None.

        The resampling path is chosen PER SLICE (a slice's pixels must not depend on what its batchmates drew):
          * a slice that did not draw the elastic deformation: rotation and crop + resize composed into ONE bilinear pass -- the form
            ``tests/golden/augment_pil.npz`` pins against PIL's two 8-bit steps (``tests/test_augment_pil_cpu.py``: within 1.5 grey
            levels mean of rotate -> 8-bit -> resized_crop, externalTransforms.py:45-66);
          * a slice that did: the reference's three steps -- rotate, round to the 8-bit grid PIL hands on, elastic deformation
            (order 0), crop + resize."""
        n, _, H_, W_ = img.shape
        angs, crops, ctrl, (Ho, Wo) = params if params is not None else self.draw(n, (H_, W_))

        def composed(im, mk, idx):
            aff = torch.tensor([affine_for(angs[i], crops[i], (H_, W_), (Ho, Wo)) for i in idx], dtype=torch.float32)
            return warp_joint(im, mk, aff, None, Ho, Wo)

        def three_steps(im, mk, idx, ct):
            full = (0, 0, H_, W_)
            rot = torch.tensor([affine_for(angs[i], full, (H_, W_), (H_, W_)) for i in idx], dtype=torch.float32)
            im, mk = warp_joint(im, mk, rot, None, H_, W_)
            im = torch.round(im * 255.0) / 255.0             # PIL hands an 8-bit image on (F.rotate -> Image)
            im, mk = elastic_deform(im, mk, ct)
            crop = torch.tensor([affine_for(0.0, crops[i], (H_, W_), (Ho, Wo)) for i in idx], dtype=torch.float32)
            return warp_joint(im, mk, crop, None, Ho, Wo)

        if ctrl is None:                                     # nobody drew the deformation
            return composed(img, msk, range(n))
        drew = ctrl.flatten(1).abs().sum(1) > 0              # (a drawn grid of exact zeros has probability 0 and IS the identity)
        ie = [i for i in range(n) if bool(drew[i])]
        ip = [i for i in range(n) if not bool(drew[i])]
        if not ip:
            return three_steps(img, msk, ie, ctrl)
        oimg = torch.empty(n, 1, Ho, Wo, dtype=torch.float32, device=img.device)
        omsk = torch.empty(n, Ho, Wo, dtype=torch.int64, device=img.device) if msk is not None else None
        for idx, fn in ((ip, lambda im, mk: composed(im, mk, ip)), (ie, lambda im, mk: three_steps(im, mk, ie, ctrl[ie]))):
            if not idx:
                continue
            sel = torch.tensor(idx, device=img.device)
            a, b = fn(img.index_select(0, sel), msk.index_select(0, sel) if msk is not None else None)
            oimg.index_copy_(0, sel, a)
            if omsk is not None:
                omsk.index_copy_(0, sel, b)
        return oimg, omsk


def elastic_deform(img, msk, ctrl):
    """``elasticdeform.deform_random_grid([img, msk], order=[0, 0])`` given its control displacements ``ctrl`` [N,2,P,P] (dy, dx in
    pixels): one launch of ``smsut_elastic_deform``."""
    n, c, H_, W_ = img.shape
    assert c == 1, "slices are single-channel (config.img_channels)"
    dev = img.device
    img = img.contiguous()
    coef = spline_prefilter(ctrl).to(dev).contiguous()
    oimg = torch.empty_like(img)
    omsk = None
    if msk is not None:
        msk = msk.to(torch.int64).contiguous()
        omsk = torch.empty_like(msk)
    H.call("smsut_elastic_deform", img, msk, coef, oimg, omsk, n, H_, W_, int(ctrl.shape[-1]), H.stream_ptr())
    return oimg, omsk


def warp_joint(img, msk, aff, ctrl, Ho, Wo):
    """One launch of ``smsut_warp_joint``: img [N,1,H,W] fp32 (device), msk [N,H,W] int64 or None, aff [N,6], ctrl
    [N,2,P,P] or None."""
    n, c, H_, W_ = img.shape
    assert c == 1, "slices are single-channel (config.img_channels)"
    dev = img.device
    img = img.contiguous()
    aff = aff.to(dev, torch.float32).contiguous()
    P = 0 if ctrl is None else int(ctrl.shape[-1])
    if ctrl is not None:
        ctrl = ctrl.to(dev, torch.float32).contiguous()
    oimg = torch.empty(n, 1, Ho, Wo, dtype=torch.float32, device=dev)
    omsk = None
    if msk is not None:
        msk = msk.to(torch.int64).contiguous()
        omsk = torch.empty(n, Ho, Wo, dtype=torch.int64, device=dev)
    H.call("smsut_warp_joint", img, msk, aff, ctrl, oimg, omsk, n, H_, W_, Ho, Wo, P, H.stream_ptr())
    return oimg, omsk


# ---- photometric augmentation: ColorJitter + RandomGammaCorrection (baseLoader.py:102-109, externalTransforms.py:23-43) --------------

def gamma_table(gamma):
    """torchvision's ``F.adjust_gamma`` for an 8-bit PIL image, gain 1: the 256-entry table ``int((255 + 1 - 1e-3) * (l / 255) **
    gamma)`` built in float64 and applied with ``Image.point``.  torchvision is not installed here and the reference does not pin a
    version: this is its published formula restated; parity at that boundary is UNPINNED.  -> uint8 [256]."""
    g = float(gamma)
    return np.array([min(255, int((255 + 1 - 1e-3) * (l / 255.0) ** g)) for l in range(256)], dtype=np.uint8)


_OUT_TABS = {}


def level_table(device, normalize):
    """The 256 output values of the photometric pass, on ``device``.  ``normalize=False``: level / 255 (IEEE fp32 quotient, ToTensor's
    scale).  ``normalize=True``: what the loader's own chain ``uint8 -> float().div_(255.0) -> sub_(0.5).div_(0.5)`` yields for every
    level, computed ONCE by that chain on the device -- the normalised batch is then bit-identical to what the loader produces from
    the same levels, by construction."""
    key = (str(torch.device(device)), bool(normalize))
    if key not in _OUT_TABS:
        if normalize:
            _OUT_TABS[key] = torch.arange(256, dtype=torch.uint8, device=device).float().div_(255.0).sub_(0.5).div_(0.5)
        else:
            _OUT_TABS[key] = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(device)
    return _OUT_TABS[key]


def photometric(img, jitter=None, gammas=None, normalize=False, out_tab=None):
    """The photometric pass with explicit parameters.  img: fp32 on the device, [N,1,H,W] or [N,H,W], on the [0, 1] scale (first
    quantised to the 8-bit level PIL would hold: floor(x * 255 + 0.5), clamped).

    jitter: None, or per slice ``(order, b, c)`` -- order 0: brightness then contrast, 1: contrast then brightness; brightness =
    PIL blend(0, v, b), contrast = blend(m, v, c) with m the rounded mean of the slice as it is at that step (``ImageEnhance``).
    gammas: None, or per slice a gamma or None (not drawn).  Output: ``out_tab[level]`` -- level / 255, the Normalize(0.5, 0.5)
    values with ``normalize=True``, or a caller's 256-float device table.  One launch, two with jitter (the histogram)."""
    if not img.is_cuda:
        raise H.SmsutHipError("the photometric pass runs on a HIP device (no CPU fallback in the product path)")
    assert img.dtype == torch.float32 and (img.dim() == 3 or (img.dim() == 4 and img.shape[1] == 1)), "slices are single-channel fp32"
    n, hw = int(img.shape[0]), int(img.shape[-1] * img.shape[-2])
    dev = img.device
    img = img.contiguous()
    rows = np.zeros((n, 4), dtype=np.float32)
    if jitter is not None:
        assert len(jitter) == n
        rows[:, :3] = np.asarray([(float(o), b, c) for (o, b, c) in jitter], dtype=np.float32).reshape(n, 3)
    tabs = np.zeros((0, 256), dtype=np.uint8)
    if gammas is not None and any(g is not None for g in gammas):
        assert len(gammas) == n
        ident = np.arange(256, dtype=np.uint8)
        tabs = np.stack([ident if g is None else gamma_table(g) for g in gammas])
        rows[:, 3] = [0.0 if g is None else 1.0 for g in gammas]
    # parameter rows and gamma tables travel in ONE upload: [n * 16 bytes of fp32 rows | n * 256 bytes of tables]
    buf = torch.from_numpy(np.concatenate([rows.view(np.uint8).ravel(), tabs.ravel()])).to(dev)
    params = buf[:n * 16].view(torch.float32)
    gtab = buf[n * 16:] if len(tabs) else None
    if out_tab is None:
        out_tab = level_table(dev, normalize)
    assert out_tab.is_cuda and out_tab.dtype == torch.float32 and out_tab.numel() == 256 and out_tab.is_contiguous()
    part = None
    if jitter is not None:
        part = level_histogram(img, _partials=True)
    out = torch.empty_like(img)
    H.call("smsut_photo_apply", img, part, params, gtab, out_tab, out, n, hw, H.stream_ptr())
    return out


def level_histogram(img, _partials=False):
    """Histogram of the quantised 8-bit levels per slice (``smsut_photo_hist``): int32 [N, 256] -- the per-workgroup rows summed
    (``_partials``: the rows themselves, [N, G, 256], as the apply kernel reads them)."""
    if not img.is_cuda:
        raise H.SmsutHipError("the photometric pass runs on a HIP device (no CPU fallback in the product path)")
    n, hw = int(img.shape[0]), int(img.shape[-1] * img.shape[-2])
    img = img.contiguous()
    g = H.call("smsut_photo_parts", hw)
    part = torch.empty(n, g, 256, dtype=torch.int32, device=img.device)
    H.call("smsut_photo_hist", img, part, n, hw, H.stream_ptr())
    return part if _partials else part.sum(1, dtype=torch.int32)


class GpuPhotometricAugment:
    """``colorJitter`` and ``gammaCorrect`` of ``config.data_aug`` as one device pass per batch.

    ColorJitter(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.125) is always applied when on; on the reference's mode-L slices
    saturation (ImageEnhance.Color's degenerate image is the image itself) and hue (torchvision returns L images untouched) are the
    identity, so a slice's jitter is b, c and which of the two comes first.  RandomGammaCorrection draws gamma, then a coin (p)."""
    brightness = 0.4             # the reference hard-codes these (baseLoader.py:104)
    contrast = 0.4
    saturation = 0.4
    hue = 0.125
    gamma_p = 0.5

    def __init__(self, data_aug):
        self.cfg = dict(data_aug or {})
        self.jitter = bool(self.cfg.get("colorJitter"))
        self.gamma = bool(self.cfg.get("gammaCorrect"))
        self.gammas = tuple(self.cfg.get("gammaCorrect_gammas", (0.7, 1.5)))

    @property
    def enabled(self):
        return self.jitter or self.gamma

    def draw(self, n):
        """Per-sample parameters from the host ``random``, in the reference's order per sample: the four jitter factors (brightness,
        contrast, saturation, hue: the last two are drawn because the reference draws them, and dropped) and the shuffle of the four
        adjustments -- of which only whether brightness precedes contrast matters, a fair coin --, then gamma, then the gamma coin
        (externalTransforms.py:35-38: drawn before the coin, like the elastic sigma).  -> (jitter, gammas) as ``photometric`` takes them."""
        jit, gam = ([] if self.jitter else None), ([] if self.gamma else None)
        for _ in range(n):
            if self.jitter:
                b = random.uniform(max(0.0, 1.0 - self.brightness), 1.0 + self.brightness)
                c = random.uniform(max(0.0, 1.0 - self.contrast), 1.0 + self.contrast)
                random.uniform(max(0.0, 1.0 - self.saturation), 1.0 + self.saturation)
                random.uniform(-self.hue, self.hue)
                order = [0, 1, 2, 3]
                random.shuffle(order)
                jit.append((0 if order.index(0) < order.index(1) else 1, b, c))
            if self.gamma:
                g = random.uniform(self.gammas[0], self.gammas[1])
                gam.append(g if random.random() < self.gamma_p else None)
        return jit, gam

    def __call__(self, img, params=None, normalize=False):
        """img [N,1,H,W] fp32 on the [0, 1] scale -> the augmented slices on that scale, or normalised to [-1, 1] (``normalize``: the
        pass then stands in for the loader's Normalize(0.5, 0.5))."""
        if not img.is_cuda:
            raise H.SmsutHipError("the photometric pass runs on a HIP device (no CPU fallback in the product path)")
        jit, gam = params if params is not None else self.draw(int(img.shape[0]))
        return photometric(img, jit, gam, normalize=normalize)
