"""fp64 reference of the test-time-augmentation ops (csrc/tta.hip), built from ``torch.flip`` / ``torch.rot90`` exactly as the
transforms are defined: ``g = r + 4 f``, ``F_g(x) = rot90(flip(x, [-1]) if f else x, k=r, dims=(-2, -1))``.  Host code only."""
import numpy as np
import torch


def fwd(x, g):
    """``F_g`` on the last two axes."""
    r, f = g & 3, g >> 2
    return torch.rot90(torch.flip(x, [-1]) if f else x, k=r, dims=(-2, -1))


def inv(y, g):
    """``F_g^-1``: back onto the un-transformed grid."""
    r, f = g & 3, g >> 2
    x = torch.rot90(y, k=-r, dims=(-2, -1))
    return torch.flip(x, [-1]) if f else x


def expand_ref(img_u8, transforms):
    """uint8 ``[N, H, W]`` -> fp32 ``[T, N, 1, H, W]``: the loader's conversion (fp32, in its order), then ``F_g``."""
    x = img_u8.float().div(255).sub(.5).div(.5)
    return torch.stack([fwd(x, g) for g in transforms]).unsqueeze(2)


def first_max(p):
    """Index of the first maximum along the last axis (no NaN in these tests)."""
    return torch.argmax((p == p.max(dim=-1, keepdim=True).values).to(torch.uint8), dim=-1)


def merge_ref(members, transforms, classes=None):
    """``members``: T arrays / tensors ``[N, H, W, C]`` (the NHWC logits of the network run on member t).  Returns fp64
    ``(pred [N, H, W] int64, conf [N, H, W], prob [N, H, W, K], gap [N, H, W])``: the softmax of channels ``0 .. K-1`` of each
    member put back with ``F_g^-1``, their mean, its first maximum, and the distance between the two largest mean probabilities
    (inf with one class)."""
    acc = None
    for z, g in zip(members, transforms):
        z = torch.as_tensor(np.asarray(z) if not isinstance(z, torch.Tensor) else z).double()
        k = z.shape[-1] if classes is None else classes
        p = torch.softmax(z[..., :k], dim=-1)                       # [N, h, w, K] on the member's grid
        p = inv(p.permute(0, 3, 1, 2), g).permute(0, 2, 3, 1)       # transforms act on the two spatial axes
        acc = p if acc is None else acc + p
    mean = acc / len(transforms)
    pred = first_max(mean)
    conf = mean.gather(-1, pred.unsqueeze(-1)).squeeze(-1)
    if mean.shape[-1] > 1:
        top2 = torch.topk(mean, 2, dim=-1).values
        gap = top2[..., 0] - top2[..., 1]
    else:
        gap = torch.full_like(conf, float("inf"))
    return pred, conf, mean, gap


def budget(k, t):
    """The absolute error budget of ``prob`` / ``conf``: 2^-24 (2 K + T + 8) -- one rounding in z - m, expf within an ulp or two,
    K - 1 additions in s, one division, T accumulations, one final division; |d| e^d <= 1/e bounds how the error of the exponent's
    argument propagates."""
    return 2.0 ** -24 * (2 * k + t + 8)
