"""Helpers shared by test_instnorm_gpu.py and test_restail_gpu.py: the kernels' fp32 pre-activation restated in numpy, and buffers
whose unwritten parts and guards are poison, so that a read of something never written or a store past the end shows."""
import numpy as np
import torch

SENT = 0x5A5A5A5A
GUARD_ROWS = 256            # the strided finalize addresses up to 255 rows past an image's block in its last round


def aff32(v, m, r, g, b):
    """in_affine (common.h) on NHWC data: fma(v - m, r * g, b) rounded once to fp32.  v [N, HW, C], m / r [N, C], g / b [C], numpy
    float32.  The fp32 difference and product are formed as the kernel forms them; their product is exact in fp64, so the sum is
    the fma's exact argument (rounded once, to ~2^-29 at the worst, before the final rounding to fp32)."""
    d = (v - m[:, None, :]).astype(np.float32)
    p = (r[:, None, :] * g[None, None, :]).astype(np.float32)
    return (d.astype(np.float64) * p + b[None, None, :]).astype(np.float32)


def gpu_mask(x, mean, rstd, g, b):
    """The activation mask the kernels use: sign of in_affine(x, mean, rstd, gamma, beta) = fma(x - mean, rstd * gamma, beta) in
    fp32 (common.h).  The fp32 difference and product are formed exactly as the kernel does; their product is exact in fp64, so the
    sign of the fp64 sum is the sign of the fma.  (The fp64 reference then differentiates with THIS mask: a pre-activation within
    an ulp of 0 must not flip between the two and move a, b by a whole gradient element.)"""
    xn = x.numpy()
    d = (xn - mean.cpu().numpy()[:, :, None, None]).astype(np.float32)
    p = (rstd.cpu().numpy() * g.cpu().numpy()[None, :]).astype(np.float32)[:, :, None, None]
    pre = d.astype(np.float64) * p + b.cpu().numpy().astype(np.float64)[None, :, None, None]
    return torch.from_numpy(pre > 0)


def _poisoned(n_floats, row_floats):
    """a partial buffer of NaN with a NaN guard of GUARD_ROWS rows behind it; returns (buffer, guard view)"""
    buf = torch.full((n_floats + GUARD_ROWS * row_floats,), float("nan"), device="cuda")
    return buf, buf[n_floats:]


def _tickets(n):
    t = torch.full((n + 64,), SENT, dtype=torch.int32, device="cuda")
    t[:n] = 0
    return t


def _check_guards(parts, tickets, outs, n, c):
    for g in parts:
        assert torch.isnan(g).all(), "a partial was stored past the last image's block"
    assert int(tickets[:n].abs().sum()) == 0, "tickets not zero again"
    assert bool((tickets[n:] == SENT).all()), "the ticket guard was written"
    for o in outs:
        assert bool((o[n * c:] == 12345.0).all()), "an output was written past [N][C]"
        assert torch.isfinite(o[:n * c]).all()
