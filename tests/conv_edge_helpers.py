"""Guard / poison buffers, seeded inputs and the fp64 references shared by the convolution edge tests
(``test_conv_families_gpu.py``, ``test_conv3x3_edges_gpu.py``, ``test_f16_edges_gpu.py``).  Tensors are NHWC, weights ``[KH][KW][Cin][Cout]``."""
import numpy as np
import torch
import torch.nn.functional as F

from conftest import rel_err

SENT = 12345.0
GUARD = 256
NAN = float("nan")
SENT_H = 12344.0             # the sentinel of an fp16 buffer (12345 is not an fp16 number)


def poisoned(n_floats):
    """n_floats of NaN (a partial that is read but never written shows) followed by a sentinel guard in the same allocation"""
    buf = torch.full((int(n_floats) + GUARD,), float("nan"), device="cuda")
    buf[int(n_floats):] = SENT
    return buf, buf[int(n_floats):]


def guarded_out(n):
    buf = torch.full((n + GUARD,), SENT, device="cuda")
    return buf, buf[n:]


def untouched(*guards):
    return all(bool((g == (SENT_H if g.dtype == torch.float16 else SENT)).all()) for g in guards)


def out_buf(*shape):
    """an output tensor of NaN with the sentinel guard behind it: (tensor, guard)"""
    n = int(np.prod(shape))
    buf, guard = poisoned(n)
    return buf[:n].view(*shape), guard


def out_buf_h(*shape):
    """out_buf for an fp16 output (the half-storage forms)"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), float("nan"), device="cuda", dtype=torch.float16)
    buf[n:] = SENT_H
    return buf[:n].view(*shape), buf[n:]


def based_buf(base):
    """a copy of the CPU tensor ``base`` on the device with the sentinel guard behind it (the accumulate forms add into it)"""
    n = base.numel()
    buf, guard = poisoned(n)
    buf[:n] = base.reshape(-1).cuda()
    return buf[:n].view(*base.shape), guard


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def check(tag, got, ref, bar):
    e = rel_err(got.detach().cpu().numpy(), ref.detach().numpy())
    print(f"{tag}: rel_err {e:.3g} bar {bar:.3g}")
    assert e < bar, tag
    return e


def cdiv(a, b):
    return (a + b - 1) // b


def conv_ref(x, w, bias, stride, pad, gy=None):
    """fp64 reference of a convolution on NHWC x and [KH][KW][Cin][Cout] w: y, and with gy also (gx, gw, gb), all in the kernels'
    layouts"""
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = w.double().permute(3, 2, 0, 1).requires_grad_(True)
    b64 = bias.double().requires_grad_(True) if bias is not None else None
    y = F.conv2d(x64, w64, b64, stride=stride, padding=pad)
    if gy is None:
        return y.detach().permute(0, 2, 3, 1)
    grads = torch.autograd.grad(y, [x64, w64] + ([b64] if bias is not None else []), gy.double().permute(0, 3, 1, 2))
    return (y.detach().permute(0, 2, 3, 1), grads[0].permute(0, 2, 3, 1), grads[1].permute(2, 3, 1, 0),
            grads[2] if bias is not None else None)


def conv3_64(x, w):
    """fp64 3x3 stride-1 pad-1 conv: x [n,h,w,ci] (any float dtype), w [3,3,ci,co] -> [n,h,w,co]"""
    return F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)


def dgrad3_64(gy, w):
    """fp64 gradient of that conv with respect to its input: gy [n,h,w,co] -> [n,h,w,ci]"""
    return F.conv_transpose2d(gy.double().permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)


def wgrad3_64(x, gy):
    """fp64 gradient of that conv with respect to its weights: [3,3,ci,co]"""
    ci, co = x.shape[3], gy.shape[3]
    gw = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2).contiguous(), (co, ci, 3, 3),
                                     gy.double().permute(0, 3, 1, 2).contiguous(), padding=1)
    return gw.permute(2, 3, 1, 0)


def tap_conv3_64(x, wtap, tap):
    """conv3_64 for a kernel that is zero outside tap (dy, dx) = divmod(tap, 3): one shifted matrix product.  wtap [ci, co]"""
    n, h, w, ci = x.shape
    dy, dx = divmod(tap, 3)
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    return xp[:, dy:dy + h, dx:dx + w, :] @ wtap.double()


def tap_dgrad3_64(gy, wtap, tap):
    """dgrad3_64 for that kernel: gx[i, j] = gy[i - dy + 1, j - dx + 1] @ wtap^T"""
    n, h, w, co = gy.shape
    dy, dx = divmod(tap, 3)
    gp = F.pad(gy.double(), (0, 0, 1, 1, 1, 1))
    return gp[:, 2 - dy:2 - dy + h, 2 - dx:2 - dx + w, :] @ wtap.double().t()


def tile_sums(v, th, tw):
    """sums of v [n, h, w, c] over th x tw pixel tiles (the plane padded with zeros to whole tiles): [n, tiles_y * tiles_x, c]"""
    n, h, w, c = v.shape
    ty, tx = cdiv(h, th), cdiv(w, tw)
    vp = F.pad(v, (0, 0, 0, tx * tw - w, 0, ty * th - h))
    return vp.view(n, ty, th, tx, tw, c).sum((2, 4)).reshape(n, ty * tx, c)


def fp16_exact(t):
    """every value survives the conversion to fp16 unchanged"""
    return bool((t.half().double() == t.double()).all())


def sums_exact(v, unit, th=None, tw=None):
    """fp32 sums of v (fp64, [n, h, w, c]) over th x tw tiles (default: over everything) are exact in ANY order: every value is a
    multiple of the power of two `unit` and sum |v| / unit stays below 2^24, so no partial sum ever needs a 25th bit"""
    q = v / unit
    if not bool((q == q.round()).all()):
        return False
    tot = tile_sums(q.abs(), th, tw).max() if th else q.abs().sum()
    return float(tot) < 2.0 ** 24
