"""Guard / poison buffers, seeded inputs and the fp64 references shared by the convolution edge tests
(``test_conv_families_gpu.py``, ``test_conv3x3_edges_gpu.py``).  Tensors are NHWC, weights ``[KH][KW][Cin][Cout]``."""
import numpy as np
import torch
import torch.nn.functional as F

from conftest import rel_err

SENT = 12345.0
GUARD = 256
NAN = float("nan")


def poisoned(n_floats):
    """n_floats of NaN (a partial that is read but never written shows) followed by a sentinel guard in the same allocation"""
    buf = torch.full((int(n_floats) + GUARD,), float("nan"), device="cuda")
    buf[int(n_floats):] = SENT
    return buf, buf[int(n_floats):]


def guarded_out(n):
    buf = torch.full((n + GUARD,), SENT, device="cuda")
    return buf, buf[n:]


def untouched(*guards):
    return all(bool((g == SENT).all()) for g in guards)


def out_buf(*shape):
    """an output tensor of NaN with the sentinel guard behind it: (tensor, guard)"""
    n = int(np.prod(shape))
    buf, guard = poisoned(n)
    return buf[:n].view(*shape), guard


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
