"""autograd plumbing over the HIP C-ABI (``_hip.py``): one ``torch.autograd.Function`` per kernel family.

Memory conventions (what the kernels see):
  * activations: logical NCHW tensors whose memory is dense NHWC (``torch.channels_last``);
  * conv / linear weights: logical OIHW (the reference's ``state_dict`` shapes) whose memory is
    ``[KH][KW][Cin][Cout]`` -- a permuted *view*, so checkpoints keep the reference's keys and shapes
    while the kernels read coalesced ``Cout``-contiguous rows;
  * ConvTranspose2d weights: logical ``[Cin, Cout, 2, 2]``, memory ``[kh][kw][Cin][Cout]`` (four 1x1-conv
    matrices, one per output tap).

Every family on the discriminator path is closed under differentiation (its ``backward`` is written
with other differentiable Functions), because WGAN-GP differentiates D's backward again
(reference trainer/uganShp0Trainer.py:127-134, ``create_graph=True``).
"""
from __future__ import annotations

import contextlib
import math
import numbers
import os as _os
from typing import NamedTuple, Optional

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _hip as H

IN_EPS = 1e-5

_INPUT_GRADS_ONLY = False


@contextlib.contextmanager
def input_grads_only():
    """Inside this context the backward of conv / norm skips parameter gradients.  Used around the
    WGAN-GP ``autograd.grad(out_src, x_hat, create_graph=True)`` call, which needs d/dx only."""
    global _INPUT_GRADS_ONLY
    prev, _INPUT_GRADS_ONLY = _INPUT_GRADS_ONLY, True
    try:
        yield
    finally:
        _INPUT_GRADS_ONLY = prev


_FIRST_ORDER = False


@contextlib.contextmanager
def first_order_pass():
    """Forward passes inside this context are differentiated at most ONCE, so modules may use the first-order-only fused
    forms (``res_tail`` in BottleBlock).  The default stays closed under differentiation: the discriminator's x_hat pass of
    WGAN-GP (``autograd.grad(..., create_graph=True)``, reference uganShp0Trainer.py:127-134) must not take them."""
    global _FIRST_ORDER
    prev, _FIRST_ORDER = _FIRST_ORDER, True
    try:
        yield
    finally:
        _FIRST_ORDER = prev


def first_order_only():
    return _FIRST_ORDER


# ------------------------------------------------------------------------------------------- layout helpers
# Tensors produced by these ops already have the kernels' layouts, so the helpers below are no-ops on the hot path; a caller
# that hands in another layout gets a converting COPY (a full extra pass).  That must not happen silently inside a timed
# step: every copy is counted (``layout_copies()``; bench.py reports the count of its timed region) and
# ``SMSUT_STRICT_LAYOUT=1`` turns it into an error.
_LAYOUT_COPIES = 0
_STRICT_LAYOUT = _os.environ.get("SMSUT_STRICT_LAYOUT", "0") not in ("0", "")


def layout_copies() -> int:
    return _LAYOUT_COPIES


def _count_copy(what, t):
    global _LAYOUT_COPIES
    _LAYOUT_COPIES += 1
    if _STRICT_LAYOUT:
        raise RuntimeError(f"SMSUT_STRICT_LAYOUT: {what} got a tensor of shape {tuple(t.shape)} / strides {t.stride()} that needs a "
                           "converting copy")


def nhwc(x: torch.Tensor) -> torch.Tensor:
    """Return ``x`` (logical NCHW, fp32) with dense NHWC memory."""
    if x.dim() != 4:
        raise ValueError(f"expected a 4-D NCHW tensor, got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise TypeError("SMSUT HIP ops compute in fp32")
    n, c, h, w = x.shape
    want = (h * w * c, 1, w * c, c)
    st = x.stride()
    if all(x.size(d) == 1 or st[d] == want[d] for d in range(4)):
        return x
    _count_copy("nhwc()", x)
    out = torch.empty_strided((n, c, h, w), want, dtype=x.dtype, device=x.device)
    out.copy_(x)
    return out


def new_act(n, c, h, w, like: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    return torch.empty_strided((n, c, h, w), (h * w * c, 1, w * c, c), dtype=dtype, device=like.device)


def hwio_strides(o, i, kh, kw):
    return (1, o, kw * i * o, i * o)


def hwio(w: torch.Tensor) -> torch.Tensor:
    """Logical OIHW weight with [KH][KW][I][O] memory (a no-op for parameters created by ``new_weight``)."""
    o, i, kh, kw = w.shape
    want = hwio_strides(o, i, kh, kw)
    st = w.stride()
    if all(w.size(d) == 1 or st[d] == want[d] for d in range(4)):
        return w
    _count_copy("hwio()", w)
    out = torch.empty_strided((o, i, kh, kw), want, dtype=w.dtype, device=w.device)
    out.copy_(w)
    return out


def new_weight(o, i, kh, kw, device=None) -> torch.Tensor:
    return torch.empty_strided((o, i, kh, kw), hwio_strides(o, i, kh, kw), dtype=torch.float32, device=device)


def convT_strides(ci, co, kh, kw):
    # memory [kh][kw][ci][co]
    return (co, 1, kw * ci * co, ci * co)


def new_convT_weight(ci, co, kh=2, kw=2, device=None) -> torch.Tensor:
    return torch.empty_strided((ci, co, kh, kw), convT_strides(ci, co, kh, kw), dtype=torch.float32, device=device)


def convT_w(w: torch.Tensor) -> torch.Tensor:
    ci, co, kh, kw = w.shape
    want = convT_strides(ci, co, kh, kw)
    st = w.stride()
    if all(w.size(d) == 1 or st[d] == want[d] for d in range(4)):
        return w
    _count_copy("convT_w()", w)
    out = torch.empty_strided(tuple(w.shape), want, dtype=w.dtype, device=w.device)
    out.copy_(w)
    return out


def new_linear_weight(out_f, in_f, device=None) -> torch.Tensor:
    """Logical [out, in] with [in][out] memory == HWIO of a 1x1 conv."""
    return torch.empty_strided((out_f, in_f), (1, out_f), dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------------- fp16-operand convolutions
# BASELINE config 5 (512 x 512 slices): the 3x3 MFMA convolutions convert their operands to fp16 while staging them into
# LDS (v_mfma_f32_16x16x16_f16, fp32 accumulate); tensors, InstanceNorm statistics, losses and optimizers stay fp32.
# ``SMSUT_CONV_DTYPE=f16`` or ``set_conv_dtype("f16")``.  Applies to the fused BasicBlock (generator, U-Net) and to generic
# convs inside ``first_order_pass()`` (the discriminator passes that are differentiated once); the WGAN-GP x_hat pass, which
# is differentiated twice, keeps fp32 operands.  Layers whose channel counts are not multiples of 16 (stems, heads, the 8-channel
# first block) and every 1x1 conv (HBM-bound streaming kernels) stay fp32 as well.
CONV_F16 = _os.environ.get("SMSUT_CONV_DTYPE", "f32").lower() in ("f16", "fp16", "half")


def set_conv_dtype(name: str):
    global CONV_F16
    if name not in ("f32", "f16"):
        raise ValueError("conv operand dtype is 'f32' or 'f16'")
    CONV_F16 = name == "f16"


def conv_dtype() -> str:
    return "f16" if CONV_F16 else "f32"


# ------------------------------------------------------------------------------------------- prepared Winograd weights
# The large-reduction Winograd kernel (csrc/conv_wino.hip, reductions >= 64 channels) transforms its weights U = G g G^T per
# workgroup and chunk -- about a tenth of its time -- unless a prepared image of the weight tensor comes WITH THE CALL (smsut_wino_prepare,
# passed with the call): then it copies the image by LDS-DMA.  An image is only right while the weights it was made from are
# unchanged, so images are made on entry of a scope in which the caller guarantees exactly that (a trainer's forward / backward
# phase: weights change in optimizer.step(), between phases) and forgotten when it closes; a module called
# outside such a scope runs the on-the-fly form.  Results are bit-identical either way.
_WINO_MIN_K = 64
# Images in force: (weight data_ptr, form 0 forward / 1 data-gradient) -> device address.  HOST-side state of this wrapper, filled
# and emptied by the ``wino_prepared`` scopes; the C-ABI library keeps none (r03's smsut_wino_bind* registry is gone): the image
# travels as an argument of the `_pre` entry points.
_WINO_ACTIVE = {}


def _conv3(name, w, transposed, *args):
    """``H.call(name, *args)`` for a conv entry point that may run the streamed-weight Winograd kernel -- through its ``_pre`` form,
    with the prepared image of ``w`` for this form as the argument before the stream, when an enclosing ``wino_prepared`` scope
    holds one (fp32 entry points only).  ``args[-1]`` is the stream."""
    wu = _WINO_ACTIVE.get((w.data_ptr(), transposed & 1)) if (_WINO_ACTIVE and not name.endswith("_f16")) else None
    if wu is None:
        return H.call(name, *args)
    return H.call(name + "_pre", *args[:-1], wu, args[-1])


class _WinoForm:
    """Images of ONE form (0: forward, 1: data-gradient) of a module's eligible 3x3 weights + the host-side argument arrays."""

    def __init__(self, ent):
        import ctypes
        self.weights = [e[0] for e in ent]
        self.n = n = len(ent)
        if n == 0:
            return
        sizes = [16 * e[2] * e[3] for e in ent]
        self.images = torch.empty(sum(sizes), dtype=torch.float32, device=ent[0][0].device)
        PA, IA = ctypes.c_void_p * n, ctypes.c_int * n
        offs = [0]
        for z in sizes[:-1]:
            offs.append(offs[-1] + z)
        base = self.images.data_ptr()
        self._keep = (PA(*[w.data_ptr() for w in self.weights]), PA(*[base + 4 * o for o in offs]), IA(*[e[2] for e in ent]),
                      IA(*[e[3] for e in ent]), IA(*[e[1] for e in ent]))
        self._addr = tuple(ctypes.addressof(a) for a in self._keep)
        # (weight address, form) -> device address of its image: what _conv3 passes to the `_pre` entry points inside a scope
        self._entries = [((w.data_ptr(), e[1]), base + 4 * o) for w, e, o in zip(self.weights, ent, offs)]

    def enter(self):
        """Returns the previous bindings of this form's keys (what ``exit`` restores: a nested scope over the same module hands the
        OUTER scope's images back instead of dropping them -- ADVICE r04)."""
        if self.n == 0:
            return ()
        # ALWAYS re-made on entry (one launch for all tensors of the form): a weight's ``_version`` is no witness of its
        # contents -- the fused optimizers (torch.optim.SGD / Adam(fused=True), what the trainers use) update in place without
        # moving it, and so does anything that writes through ``.data``
        H.call("smsut_wino_prepare", *self._addr, self.n, _s())
        prev = tuple((key, _WINO_ACTIVE.get(key)) for key, _ in self._entries)
        for key, addr in self._entries:
            _WINO_ACTIVE[key] = addr
        return prev

    @staticmethod
    def exit(prev):
        for key, addr in prev:
            if addr is None:
                _WINO_ACTIVE.pop(key, None)
            else:
                _WINO_ACTIVE[key] = addr


class _WinoSet:
    def __init__(self, module: torch.nn.Module):
        ent = ([], [])                                       # per form: (weight, transposed, Kdim, Ndim)
        seen = set()
        for m in module.modules():
            w = getattr(m, "weight", None)
            if not isinstance(w, torch.Tensor) or w.dim() != 4 or not w.is_cuda or w.dtype != torch.float32:
                continue
            co, ci, kh, kw = w.shape
            if (kh, kw) != (3, 3) or getattr(m, "stride", 1) != 1 or getattr(m, "padding", 1) != 1 or w.data_ptr() in seen:
                continue
            if w.stride() != hwio_strides(co, ci, 3, 3) or ci % 16 or co % 16:
                continue
            seen.add(w.data_ptr())
            if ci >= _WINO_MIN_K:
                ent[0].append((w, 0, ci, co))
            if co >= _WINO_MIN_K:
                ent[1].append((w, 1, co, ci))
        self.ptrs = self._layout(module)
        self.forms = (_WinoForm(ent[0]), _WinoForm(ent[1]))

    @staticmethod
    def _layout(module):
        return tuple(p.data_ptr() for p in module.parameters() if p.dim() == 4)

    def stale_layout(self, module):
        """parameters re-created or moved since the images were laid out (``.to(device)``, a re-built layer)"""
        return self._layout(module) != self.ptrs

    def __deepcopy__(self, memo):                            # copy.deepcopy(module) (EMA teachers): the copy lays out its own
        return None

    def __reduce__(self):
        return (type(None), ())


@contextlib.contextmanager
def wino_prepared(*modules: torch.nn.Module, forms: str = "fb"):
    """Scope in which the 3x3 weights of ``modules`` do not change.  ``forms``: "f" (the forward convolutions run inside), "b"
    (their data-gradients), "fb".  On entry the Winograd images of those forms are made from the weights as they are NOW (one
    launch per module and form -- inside a hipGraph capture it becomes part of the captured phase, which therefore never
    depends on what another phase left behind) and bound for the convolutions inside; unbound on exit."""
    active = []
    if not CONV_F16:
        for m in modules:
            ws = m.__dict__.get("_smsut_wino_set")
            if ws is None or ws.stale_layout(m):
                ws = _WinoSet(m)
                m.__dict__["_smsut_wino_set"] = ws
            if "f" in forms:
                active.append(ws.forms[0])
            if "b" in forms:
                active.append(ws.forms[1])
    entered = []                                             # (form, previous bindings), in entry order
    try:
        for f in active:                                     # inside the try: a failing enter() leaves no binding of an earlier form behind
            entered.append((f, f.enter()))
        yield
    finally:
        for f, prev in reversed(entered):
            f.exit(prev)


def _grad_scale(t: torch.Tensor) -> torch.Tensor:
    """Device float[2] = {s, 1/s}: power-of-two scale that brings max|t| into [2^13, 2^14] -- gradient tensors sit far below
    fp16's normal range (|gy| ~ 1e-7 at 512^2); the f16 kernels multiply by s before converting and by 1/s after."""
    out = torch.empty(2, dtype=torch.float32, device=t.device)
    H.call("smsut_absmax_scale", t, t.numel(), out, _ws(H.call("smsut_absmax_scale_ws", t.numel()), t), _s())
    return out


def _grad_scale_from(amax: torch.Tensor) -> torch.Tensor:
    """The same scale from maxima the producing kernels handed over (``amax``: a slice of device floats): no pass over the tensors."""
    out = torch.empty(2, dtype=torch.float32, device=amax.device)
    H.call("smsut_absmax_finish", amax, amax.numel(), out, _s())
    return out


def _grad_scale2(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """One scale for two gradient tensors that feed the same fp16 accumulators (the fused-shortcut data- / weight-gradient reads
    [gy | gs] as one operand): max over both."""
    out = torch.empty(2, dtype=torch.float32, device=a.device)
    H.call("smsut_absmax_scale2", a, a.numel(), b, b.numel(), out, _ws(H.call("smsut_absmax_scale_ws", a.numel()), a), _s())
    return out


def _ws(numel: int, like: torch.Tensor) -> torch.Tensor:
    return torch.empty(max(int(numel), 1), dtype=torch.float32, device=like.device)


def _s():
    return H.stream_ptr()


def _vec(like: torch.Tensor, *shape) -> torch.Tensor:
    """Uninitialised fp32 tensor on ``like``'s device: per-image / per-channel statistics and their gradients."""
    return torch.empty(*shape, dtype=torch.float32, device=like.device)


# ------------------------------------------------------------------------------------------- convolution
def _out_size(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


def _conv_fwd_launch(x, w, bias, stride, pad, want_stats=False, f16=False):
    n, ci, h, wd = x.shape
    co, ci2, kh, kw = w.shape
    assert ci == ci2, f"conv: Cin mismatch {ci} vs {ci2}"
    ho, wo = _out_size(h, kh, stride, pad), _out_size(wd, kw, stride, pad)
    y = new_act(n, co, ho, wo, x)
    if kh == 1 and kw == 1 and stride == 1 and pad == 0 and H.call("smsut_conv1x1_supported", ci, co):
        tiles = H.call("smsut_conv1x1_tiles", n, h * wd, co) if (want_stats and bias is None) else 0
        part = _ws(n * tiles * co * 2, x) if tiles else None
        H.call("smsut_conv1x1_fwd", x, w, y, part, n, h * wd, ci, co, 0, _s())
        if bias is not None:
            H.call("smsut_bias_add", y, bias, y, n * ho * wo, co, _s())
        if tiles:
            y._smsut_in_partials = (part, tiles)
        return y
    if kh == kw and H.call("smsut_conv2d_mfma_supported", kh, stride, pad, ci, co):
        f16 = f16 and bool(H.call("smsut_conv2d_f16_supported", kh, ci, co))
        if want_stats and bias is None:
            # fused InstanceNorm statistics: the conv epilogue leaves {sum, sum^2} partials that the following
            # instnorm_act picks up from the tensor object (side channel; autograd is unaffected)
            tiles = H.call("smsut_conv2d_mfma_tiles", n, h, wd, ci, co, kh, int(f16))
            part = _ws(n * tiles * co * 2, x)
            _conv3("smsut_conv2d_fwd_mfma_stats_f16" if f16 else "smsut_conv2d_fwd_mfma_stats", w, 0, x, w, y, part, n, h, wd, ci, co,
                   kh, _s())
            y._smsut_in_partials = (part, tiles)
            return y
        if f16:
            H.call("smsut_conv2d_fwd_mfma_f16", x, w, y, None, n, h, wd, ci, co, kh, 0, _s())
        else:
            _conv3("smsut_conv2d_fwd_mfma", w, 0, x, w, y, n, h, wd, ci, co, kh, 0, _s())
        if bias is not None:
            H.call("smsut_bias_add", y, bias, y, n * ho * wo, co, _s())
    elif (kh == 4 and kw == 4 and stride == 1 and pad == 1
          and H.call("smsut_conv2d_k4_supported", ci, co)):
        # networks.NLayerDiscriminator (networks.py:977-1032): 4x4 s1 p1 on the matrix cores
        H.call("smsut_conv2d_k4_fwd", x, w, y, n, h, wd, ci, co, 0, _s())
        if bias is not None:
            H.call("smsut_bias_add", y, bias, y, n * ho * wo, co, _s())
    elif kh == kw and H.call("smsut_conv2d_small_supported", kh, ci, co):
        H.call("smsut_conv2d_small_fwd", x, w, bias, y, n, h, wd, ci, ho, wo, co, kh, stride, pad, _s())
    else:
        H.call("smsut_conv2d_fwd_generic", x, w, bias, y, n, h, wd, ci, ho, wo, co, kh, kw, stride, pad, _s())
    return y


def _conv_dgrad_launch(gy, w, h, wd, stride, pad, f16=False):
    n, co, ho, wo = gy.shape
    co2, ci, kh, kw = w.shape
    assert co == co2
    gx = new_act(n, ci, h, wd, gy)
    one_by_one = kh == 1 and kw == 1 and stride == 1 and pad == 0
    if one_by_one and co % 4 != 0 and H.call("smsut_conv1x1_thin_supported", ci, co):   # heads: 1, 5 channels
        H.call("smsut_conv1x1_thin_dgrad", gy, w, gx, n, h * wd, ci, co, _s())
        return gx
    if kh == 1 and kw == 1 and stride == 1 and pad == 0 and H.call("smsut_conv1x1_supported", co, ci):
        H.call("smsut_conv1x1_fwd", gy, w, gx, None, n, h * wd, co, ci, 1, _s())
        return gx
    if kh == kw and H.call("smsut_conv2d_mfma_supported", kh, stride, pad, co, ci):
        if f16 and H.call("smsut_conv2d_f16_supported", kh, co, ci):
            H.call("smsut_conv2d_fwd_mfma_f16", gy, w, gx, _grad_scale(gy), n, h, wd, co, ci, kh, 1, _s())
        else:
            _conv3("smsut_conv2d_fwd_mfma", w, 1, gy, w, gx, n, h, wd, co, ci, kh, 1, _s())
    elif (kh == 4 and kw == 4 and stride == 1 and pad == 1
          and H.call("smsut_conv2d_k4_supported", ci, co)):
        H.call("smsut_conv2d_k4_fwd", gy, w, gx, n, h, wd, ci, co, 1, _s())
    elif kh == kw and H.call("smsut_conv2d_small_supported", kh, ci, co):
        H.call("smsut_conv2d_small_dgrad", gy, w, gx, n, h, wd, ci, ho, wo, co, kh, stride, pad, _s())
    else:
        H.call("smsut_conv2d_dgrad_generic", gy, w, gx, n, h, wd, ci, ho, wo, co, kh, kw, stride, pad, _s())
    return gx


def _conv_wgrad_launch(x, gy, kh, kw, stride, pad, f16=False):
    n, ci, h, wd = x.shape
    _, co, ho, wo = gy.shape
    gw = new_weight(co, ci, kh, kw, device=x.device)
    one_by_one = kh == 1 and kw == 1 and stride == 1 and pad == 0
    if one_by_one and co % 4 != 0 and H.call("smsut_conv1x1_thin_supported", ci, co):
        H.call("smsut_conv1x1_thin_wgrad", x, gy, gw, _ws(H.call("smsut_conv1x1_thin_wgrad_ws", ci), x), n, h * wd, ci, co, _s())
        return gw
    if kh == 1 and kw == 1 and stride == 1 and pad == 0 and ci % 4 == 0 and co % 4 == 0:
        H.call("smsut_conv1x1_wgrad", x, gy, gw, _ws(H.call("smsut_conv1x1_wgrad_ws", n, h * wd, ci, co), x), n, h * wd, ci, co, _s())
        return gw
    if (f16 and kh == 3 and kw == 3 and stride == 1 and pad == 1
            and H.call("smsut_conv2d_wgrad_f16_supported", n, h, wd, ci, co)):
        ws = _ws(H.call("smsut_conv2d_wgrad_f16_ws", n, h, wd, ci, co), x)
        H.call("smsut_conv2d_wgrad_f16", x, None, 0, gy, gw, ws, _grad_scale(gy), n, h, wd, ci, co, _s())
        return gw
    if kh == kw and H.call("smsut_conv2d_wgrad_mfma_supported", kh, stride, pad, ci, co):
        ws = _ws(H.call("smsut_conv2d_wgrad_mfma_ws", n, h, wd, ci, co, kh), x)
        H.call("smsut_conv2d_wgrad_mfma", x, gy, gw, ws, n, h, wd, ci, co, kh, _s())
    elif (kh == 4 and kw == 4 and stride == 1 and pad == 1
          and H.call("smsut_conv2d_k4_supported", ci, co)):
        ws = _ws(H.call("smsut_conv2d_k4_wgrad_ws", n, h, wd, ci, co), x)
        H.call("smsut_conv2d_k4_wgrad", x, gy, gw, ws, n, h, wd, ci, co, _s())
    elif kh == kw and H.call("smsut_conv2d_flat_wgrad_supported", kh, stride, ci, co):
        ws = _ws(H.call("smsut_conv2d_flat_wgrad_ws", n, ho, wo, ci, co, kh), x)
        H.call("smsut_conv2d_flat_wgrad", x, gy, gw, ws, n, h, wd, ci, ho, wo, co, kh, stride, pad, _s())
    else:
        ws = _ws(H.call("smsut_conv2d_wgrad_generic_ws", n, ho, wo, ci, co, kh, kw), x)
        H.call("smsut_conv2d_wgrad_generic", x, gy, gw, ws, n, h, wd, ci, ho, wo, co, kh, kw, stride, pad, _s())
    return gw


def conv_fwd_kernel_name(cin, cout, k, stride, pad, n=1, h=0, w=0):
    """Which device kernel ``conv2d`` dispatches to for this layer shape: (symbol, 'mfma' | 'generic')."""
    if H.call("smsut_conv2d_mfma_supported", k, stride, pad, cin, cout):
        if h and w and H.call("smsut_conv2d_mfma_persistent", n, h, w, cin, cout, k, 0):
            return "conv_mfma_fwd_p", "mfma"
        return "conv_mfma_fwd", "mfma"
    return "conv_fwd_naive", "generic"


class Conv2dFn(Function):
    """y = conv2d(x, w) (+ bias).  Reference: nn.Conv2d uses at network/blocks.py:10-16,123; ugan.py:70,202,214-215."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, pad, want_stats=False):
        x, w = nhwc(x), hwio(w)
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        ctx.geom = (stride, pad)
        ctx.f16 = CONV_F16 and _FIRST_ORDER          # passes differentiated once only; the WGAN-GP x_hat pass stays fp32
        return _conv_fwd_launch(x, w, bias, stride, pad, want_stats, ctx.f16)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride, pad = ctx.geom
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = Conv2dDgradFn.apply(gy, w, x.shape[2], x.shape[3], stride, pad, ctx.f16)
        if not _INPUT_GRADS_ONLY:
            if ctx.needs_input_grad[1]:
                gw = Conv2dWgradFn.apply(x, gy, w.shape[2], w.shape[3], stride, pad, ctx.f16)
            if ctx.has_bias and ctx.needs_input_grad[2]:
                gb = SumPerChannelFn.apply(gy)
        return gx, gw, gb, None, None, None


class Conv2dDgradFn(Function):
    """gx = conv2d_backward_data(gy, w); bilinear in (gy, w) so its backward is a conv and a wgrad."""

    @staticmethod
    def forward(ctx, gy, w, h, wd, stride, pad, f16=False):
        gy, w = nhwc(gy), hwio(w)
        ctx.save_for_backward(gy, w)
        ctx.geom = (h, wd, stride, pad)
        return _conv_dgrad_launch(gy, w, h, wd, stride, pad, f16)

    @staticmethod
    def backward(ctx, ggx):
        gy, w = ctx.saved_tensors
        h, wd, stride, pad = ctx.geom
        d_gy = d_w = None
        if ctx.needs_input_grad[0]:
            d_gy = Conv2dFn.apply(ggx, w, None, stride, pad, False)
        if ctx.needs_input_grad[1]:
            d_w = Conv2dWgradFn.apply(ggx, gy, w.shape[2], w.shape[3], stride, pad)
        return d_gy, d_w, None, None, None, None, None


class Conv2dWgradFn(Function):
    """gw = conv2d_backward_weight(x, gy); bilinear in (x, gy)."""

    @staticmethod
    def forward(ctx, x, gy, kh, kw, stride, pad, f16=False):
        x, gy = nhwc(x), nhwc(gy)
        ctx.save_for_backward(x, gy)
        ctx.geom = (kh, kw, stride, pad)
        return _conv_wgrad_launch(x, gy, kh, kw, stride, pad, f16)

    @staticmethod
    def backward(ctx, ggw):
        x, gy = ctx.saved_tensors
        kh, kw, stride, pad = ctx.geom
        d_x = d_gy = None
        if ctx.needs_input_grad[0]:
            d_x = Conv2dDgradFn.apply(gy, ggw, x.shape[2], x.shape[3], stride, pad)
        if ctx.needs_input_grad[1]:
            d_gy = Conv2dFn.apply(x, ggw, None, stride, pad, False)
        return d_x, d_gy, None, None, None, None, None


class SumPerChannelFn(Function):
    """out[c] = sum_{n,h,w} x[n,c,h,w]  (bias gradient)."""

    @staticmethod
    def forward(ctx, x):
        x = nhwc(x)
        n, c, h, w = x.shape
        ctx.shape = (n, c, h, w)
        out = torch.empty(c, dtype=torch.float32, device=x.device)
        rows = n * h * w
        H.call("smsut_colsum", x, out, _ws(H.call("smsut_colsum_ws", rows, c), x), rows, c, _s())
        return out

    @staticmethod
    def backward(ctx, g):
        n, c, h, w = ctx.shape
        return BroadcastChannelFn.apply(g, n, h, w)


class BroadcastChannelFn(Function):
    """out[n,c,h,w] = v[c]  (adjoint of SumPerChannelFn)."""

    @staticmethod
    def forward(ctx, v, n, h, w):
        c = v.numel()
        y = new_act(n, c, h, w, v)
        H.call("smsut_fill", y, 0.0, y.numel(), _s())
        H.call("smsut_bias_add", y, v.contiguous(), y, n * h * w, c, _s())
        return y

    @staticmethod
    def backward(ctx, g):
        return SumPerChannelFn.apply(g), None, None, None


def cl(x):
    """Autograd-tracked conversion to NHWC memory (a no-op for tensors produced by these ops)."""
    return x.contiguous(memory_format=torch.channels_last)


def conv2d(x, w, bias=None, stride=1, pad=0, stats=False):
    """``stats=True``: the caller promises to feed the result straight into ``instnorm_act``; the conv epilogue then
    also produces the InstanceNorm statistics partials (saves one full pass over the output)."""
    y = Conv2dFn.apply(cl(x), w, bias, stride, pad, stats)
    return y


class ConvT2x2Fn(Function):
    """ConvTranspose2d(k=2, s=2, bias=False) (network/blocks.py:41): four 1x1 MFMA convs, one per output tap."""

    @staticmethod
    def forward(ctx, x, w):
        x, w = nhwc(x), convT_w(w)
        n, ci, h, wd = x.shape
        ci2, co, kh, kw = w.shape
        assert ci == ci2 and kh == 2 and kw == 2
        if not H.call("smsut_convT2x2_mfma_supported", ci, co):
            raise H.SmsutHipError(f"ConvTranspose2x2 needs channel counts that are multiples of 4, got {ci}->{co}")
        ctx.save_for_backward(x, w)
        y = new_act(n, co, 2 * h, 2 * wd, x)
        if H.call("smsut_convT2x2_ps_supported", ci, co):        # one 1x1 pass over x with pixel-shuffle stores
            H.call("smsut_convT2x2_fwd_ps", x, w, y, n, h, wd, ci, co, _s())
        else:
            H.call("smsut_convT2x2_fwd_mfma", x, w, y, n, h, wd, ci, co, _s())
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = nhwc(gy)
        n, ci, h, wd = x.shape
        co = w.shape[1]
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = new_act(n, ci, h, wd, x)
            H.call("smsut_convT2x2_dgrad_mfma", gy, w, gx, n, h, wd, ci, co, _s())
        if ctx.needs_input_grad[1]:
            gw = new_convT_weight(ci, co, 2, 2, device=x.device)
            if H.call("smsut_convT2x2_ps_supported", ci, co):
                ws = _ws(H.call("smsut_convT2x2_wgrad_ps_ws", n, h, wd, ci, co), x)
                H.call("smsut_convT2x2_wgrad_ps", x, gy, gw, ws, n, h, wd, ci, co, _s())
            else:
                ws = _ws(H.call("smsut_convT2x2_wgrad_mfma_ws", n, h, wd, ci, co), x)
                H.call("smsut_convT2x2_wgrad_mfma", x, gy, gw, ws, n, h, wd, ci, co, _s())
        return gx, gw


def conv_transpose2x2(x, w):
    return ConvT2x2Fn.apply(x, w)


def linear(x2d, w, bias):
    """nn.Linear on [P, in] rows as a 1x1 conv over P 'images' of 1x1 pixels (network/ugan.py:295)."""
    p, cin = x2d.shape
    y = conv2d(x2d.reshape(p, cin, 1, 1), w.view(w.shape[0], w.shape[1], 1, 1), bias)
    return y.reshape(p, -1)


# ------------------------------------------------------------------------------------------- instance norm (+act)
class InstNormActFn(Function):
    """y = act(InstanceNorm(x) * gamma + beta); act = LeakyReLU(slope) or identity (network/blocks.py:19-32)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, slope, has_act):
        x = nhwc(x)
        n, c, h, w = x.shape
        y = new_act(n, c, h, w, x)
        mean, rstd = _vec(x, n, c), _vec(x, n, c)
        fused = getattr(x, "_smsut_in_partials", None)
        if fused is not None:
            part, tiles = fused
            H.call("smsut_instnorm_fwd_partials", x, gamma, beta, y, mean, rstd, part, tiles, n, h * w, c,
                   IN_EPS, float(slope), int(has_act), _s())
            del x._smsut_in_partials
        else:
            chunks = H.call("smsut_in_chunks", n, h * w, c)
            H.call("smsut_instnorm_fwd", x, gamma, beta, y, mean, rstd, _ws(n * chunks * c * 3, x), n, h * w, c,
                   IN_EPS, float(slope), int(has_act), _s())
        ctx.save_for_backward(x, mean, rstd, gamma, beta)       # y is NOT kept: the mask is recomputed from x
        ctx.cfg = (float(slope), bool(has_act))
        ctx.mark_non_differentiable(mean, rstd)
        ctx.set_materialize_grads(False)
        return y, mean, rstd

    @staticmethod
    def backward(ctx, gy, _gm, _gr):
        if gy is None:          # reached only through the (non-differentiable) mask input of the double backward
            return None, None, None, None, None
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        slope, has_act = ctx.cfg
        want_affine = (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) and not _INPUT_GRADS_ONLY
        gx, gg, gb = InstNormActBwdFn.apply(gy, x, beta, mean, rstd, gamma, slope, has_act, want_affine)
        if not want_affine:
            gg = gb = None
        return gx, gg, gb, None, None


class InstNormActBwdFn(Function):
    """(gx, ggamma, gbeta) of InstNormActFn; its own backward is the closed-form second derivative
    (csrc/norm.hip header) needed by the gradient penalty."""

    @staticmethod
    def forward(ctx, gy, x, beta, mean, rstd, gamma, slope, has_act, want_affine):
        gy = nhwc(gy)
        n, c, h, w = x.shape
        gx = new_act(n, c, h, w, x)
        a, b = _vec(x, n, c), _vec(x, n, c)
        gg, gb = _vec(x, c), _vec(x, c)
        chunks = H.call("smsut_in_chunks", n, h * w, c)
        H.call("smsut_instnorm_bwd", gy, x, beta if has_act else None, mean, rstd, gamma, gx, a, b,
               gg if want_affine else None, gb if want_affine else None, _ws(n * chunks * c * 3, x),
               n, h * w, c, slope, _s())
        ctx.save_for_backward(gy, x, beta, mean, rstd, gamma, a, b)
        ctx.cfg = (slope, has_act, want_affine)
        ctx.set_materialize_grads(False)
        return gx, gg, gb

    @staticmethod
    @once_differentiable
    def backward(ctx, v, ug, ub):
        gy, x, beta, mean, rstd, gamma, a, b = ctx.saved_tensors
        slope, has_act, want_affine = ctx.cfg
        if v is None:                       # only the affine gradients were used downstream
            v = torch.zeros_like(x)
        v = nhwc(v)
        n, c, h, w = x.shape
        d_gy = new_act(n, c, h, w, x)
        d_x = new_act(n, c, h, w, x)
        d_gamma = torch.empty(c, dtype=torch.float32, device=x.device)
        chunks = H.call("smsut_in_chunks", n, h * w, c)
        if not want_affine:
            ug = ub = None
        H.call("smsut_instnorm_bwd2", v, ug, ub, gy, x, beta if has_act else None, mean, rstd, gamma, a, b,
               d_gy, d_x, d_gamma, _ws(n * chunks * c * 3, x), _ws(3 * n * c, x), n, h * w, c, slope, _s())
        return d_gy, d_x, None, None, None, d_gamma, None, None, None


class InstNormActPoolFn(Function):
    """avg_pool2(lrelu(InstanceNorm(x) * gamma + beta)) as ONE op -- bn1 -> relu -> avgpool of a stride-2 BottleBlock
    (reference network/blocks.py:99-107) for passes that are differentiated once (the discriminator's real | fake pass and D(x_fake);
    the WGAN-GP x_hat pass keeps the twice-differentiable InstNormActFn + AvgPool2Fn).  x is a raw conv output that carries the
    statistics partials of the conv epilogue.  Forward: one read of x, a quarter-size write; backward: the full-resolution gradient
    0.25 * g[h/2][w/2] is formed while loading in both passes.  Bit-identical to the two-op composition."""

    @staticmethod
    def forward(ctx, x, gamma, beta, slope):
        x = nhwc(x)
        n, c, h, w = x.shape
        part, tiles = x._smsut_in_partials
        del x._smsut_in_partials
        y = new_act(n, c, h // 2, w // 2, x)
        mean, rstd = _vec(x, n, c), _vec(x, n, c)
        H.call("smsut_instnorm_pool_fwd_partials", x, gamma, beta, y, mean, rstd, part, tiles, n, h, w, c, IN_EPS, float(slope), _s())
        ctx.save_for_backward(x, mean, rstd, gamma, beta)
        ctx.slope = float(slope)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        gy = nhwc(gy)
        n, c, h, w = x.shape
        want_affine = (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) and not _INPUT_GRADS_ONLY
        gx = new_act(n, c, h, w, x)
        a, b = _vec(x, n, c), _vec(x, n, c)
        gg = _vec(x, c) if want_affine else None
        gb = torch.empty_like(gg) if want_affine else None
        chunks = H.call("smsut_in_chunks", n, h * w, c)
        H.call("smsut_instnorm_pool_bwd", gy, x, beta, mean, rstd, gamma, gx, a, b, gg, gb, _ws(n * chunks * c * 3, x), n, h, w, c,
               ctx.slope, _s())
        return gx, gg, gb, None


IN_ACT_POOL = bool(int(_os.environ.get("SMSUT_IN_ACT_POOL", "1")))       # stride-2 BottleBlock, first-order passes: IN + act + pool as one op


def instnorm_act_pool_fusable(x):
    """x carries conv-epilogue statistics, even plane, whole channel quads, and the pass is differentiated at most once."""
    return (IN_ACT_POOL and first_order_only() and hasattr(x, "_smsut_in_partials") and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
            and x.shape[1] % 4 == 0 and x.dtype == torch.float32)


def instnorm_act_pool(x, gamma, beta, slope: float):
    return InstNormActPoolFn.apply(cl(x), gamma, beta, float(slope))


def instnorm_act(x, gamma, beta, slope: Optional[float]):
    """slope=None -> no activation."""
    y, _, _ = InstNormActFn.apply(cl(x), gamma, beta, 0.0 if slope is None else slope, slope is not None)
    return y


# ------------------------------------------------------------------------------------------- residual tail
class ResTailFn(Function):
    """out = act(IN(y2; g2, b2) + IN(s; gs, bs))  -- the tail of BasicBlock / BottleBlock (network/blocks.py:74-79, 110-116)
    as ONE pass forward (plus the statistics finalisation) and one reduce + one apply pass backward, instead of two
    normalise kernels, an add and their separate backwards.  First-order only.  y2 / s may carry the statistics partials
    of the conv epilogue that produced them (``_smsut_in_partials``)."""

    @staticmethod
    def forward(ctx, y2, g2, b2, s, gs, bs, slope, pool=False):
        # pool (r05): also returns avg_pool2(out) -- the next stride-2 BottleBlock's shortcut input -- written by the same pass; the backward
        # then takes the two gradients (through conv1 of the next block, through its pooled shortcut) without a pooling-backward pass
        # and without autograd's accumulation kernel (smsut_restail_*_pool with idx = null)
        y2, s = nhwc(y2), nhwc(s)
        n, c, h, w = y2.shape
        hw = h * w
        st = _s()

        def stats(t):
            m, r = _vec(t, n, c), _vec(t, n, c)
            part, tiles = t._smsut_in_partials            # res_tail_fusable() checked that both inputs carry them
            del t._smsut_in_partials
            H.call("smsut_in_finalize_fwd", part, tiles, m, r, n, hw, c, IN_EPS, st)
            return m, r
        m2, r2 = stats(y2)
        ms, rs = stats(s)
        out = new_act(n, c, h, w, y2)
        ctx.pool = bool(pool)
        if pool:
            pooled = new_act(n, c, h // 2, w // 2, y2)
            H.call("smsut_restail_fwd_pool", y2, m2, r2, g2, b2, s, ms, rs, gs, bs, out, pooled, None, n, h, w, c, float(slope), 0, st)
        else:
            H.call("smsut_restail_fwd", y2, m2, r2, g2, b2, s, ms, rs, gs, bs, out, n, hw, c, float(slope), st)
        ctx.save_for_backward(y2, s, out, m2, r2, ms, rs, g2, gs, b2, bs)
        ctx.slope = float(slope)
        return (out, pooled) if pool else out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_pooled=None):
        y2, s, out, m2, r2, ms, rs, g2, gs, b2, bs = ctx.saved_tensors
        n, c, h, w = y2.shape
        if ctx.pool and g_out is None:                   # (pooled path alone)
            g_out = new_act(n, c, h, w, y2)
            H.call("smsut_avgpool2_bwd", nhwc(g_pooled), g_out, n, h, w, c, _s())
            g_pooled = None
        mp = ctx.pool and g_pooled is not None
        g_out = nhwc(g_out)
        hw = h * w
        gy2, gs_t = new_act(n, c, h, w, y2), new_act(n, c, h, w, y2)
        a_t, b2_t, bs_t = _vec(y2, n, c), _vec(y2, n, c), _vec(y2, n, c)
        gg2, gb2, ggs, gbs = _vec(y2, c), _vec(y2, c), _vec(y2, c), _vec(y2, c)
        chunks = H.call("smsut_in_chunks", n, hw, c)
        if mp:
            H.call("smsut_restail_bwd_pool", g_out, nhwc(g_pooled), None, y2, m2, r2, g2, b2, s, ms, rs, gs, bs, gy2, gs_t, a_t, b2_t,
                   bs_t, gg2, gb2, ggs, gbs, _ws(n * chunks * c * 3, y2), None, None, n, h, w, c, ctx.slope, 0, _s())
        else:
            H.call("smsut_restail_bwd", g_out, out, y2, m2, r2, g2, b2, s, ms, rs, gs, bs, gy2, gs_t, a_t, b2_t, bs_t, gg2, gb2,
                   ggs, gbs, _ws(n * chunks * c * 3, y2), n, hw, c, ctx.slope, _s())
        return gy2, gg2, gb2, gs_t, ggs, gbs, None, None


def res_tail_fusable(y2, s):
    """Both raw conv outputs come with their statistics partials (MFMA / streaming 1x1 conv epilogues) and the pass will
    be differentiated at most once."""
    return (FUSED_BLOCK and FUSED_RES_TAIL and first_order_only() and hasattr(y2, "_smsut_in_partials") and hasattr(s, "_smsut_in_partials")
            and y2.shape == s.shape)


def res_tail(y2, g2, b2, s, gs, bs, slope):
    return ResTailFn.apply(y2, g2, b2, s, gs, bs, slope)


TAIL_AVGPOOL = bool(int(_os.environ.get("SMSUT_TAIL_AVGPOOL", "1")))     # BottleBlock -> stride-2 BottleBlock: tail + the next shortcut's pooling


def res_tail_pool_fusable(y2):
    return TAIL_AVGPOOL and y2.shape[1] % 4 == 0 and y2.shape[2] % 2 == 0 and y2.shape[3] % 2 == 0


def res_tail_pool(y2, g2, b2, s, gs, bs, slope):
    """(out, avg_pool2(out)) of a BottleBlock whose output feeds a stride-2 BottleBlock (one pass; see ResTailFn)."""
    return ResTailFn.apply(y2, g2, b2, s, gs, bs, slope, True)


# ------------------------------------------------------------------------------------------- fused BasicBlock
FUSED_BLOCK = bool(int(_os.environ.get("SMSUT_FUSED_BLOCK", "1")))
FUSED_RES_TAIL = bool(int(_os.environ.get("SMSUT_FUSED_RES_TAIL", "1")))       # BottleBlock tail in first_order_pass()
VIRTUAL_CAT = bool(int(_os.environ.get("SMSUT_VIRTUAL_CAT", "1")))   # block-after-concat reads [up, skip] in place (no cat tensor)
SPLIT_DGRAD = bool(int(_os.environ.get("SMSUT_SPLIT_DGRAD", "1")))   # block-after-concat: gradient written into the two parts
AMAX_HANDOVER = bool(int(_os.environ.get("SMSUT_AMAX_HANDOVER", "1")))    # fp16 operands: gradient maxima from the producing kernels


def basic_block_fusable(x, w1, ws):
    """The fused path needs the MFMA kernels on every conv of the block: channel counts that are multiples of 4."""
    co, ci = w1.shape[0], w1.shape[1]
    return (FUSED_BLOCK and x.is_cuda and ci % 4 == 0 and co % 4 == 0 and ci >= 4 and co >= 4
            and (ws is not None or ci == co))


# ------------------------------------------------------------------------------------------- in-launch InstanceNorm finalize
# The three statistics-producing convs of a fused BasicBlock (conv1 + shortcut, conv2, conv2's data-gradient) can finalise their
# InstanceNorm statistics INSIDE the launch (csrc/common.h FinRef: the workgroup whose partials complete an image combines them --
# same order, same bits as the separate smsut_in_finalize_* launch, which disappears: ~150 launches of 4.7 us on the generator's
# critical path per uganConsis iteration).  The kernels count arrivals in TICKETS: int32 [N], zero on entry, zero again on exit.
# They come from here:
#   * eager launches: slices of ONE zero-initialised ring per device (1 Mi ints; a slice is handed out again only after ~30 000
#     later calls, long after its launch has run -- and every launch leaves its slice zeroed);
#   * inside a GraphedPhase capture: slices of a per-capture chunk allocated (and zero-filled: one fill node, replayed first) in
#     that graph's own pool -- a replay re-zeroes its tickets before use, and no eager launch ever shares them;
#   * inside somebody else's stream capture: no in-launch finalize (the separate launch runs).
# It is carried by conv1 + shortcut and conv2 (forward; the two go together: conv2 reads what conv1's launch finalised), conv2's
# data-gradient and the residual tail's backward.  ``SMSUT_FIN=0`` switches the whole thing off (A/B).
FIN_ON = bool(int(_os.environ.get("SMSUT_FIN", "1")))
_TICKET_RING = {}            # device index -> [tensor, position]
_TICKET_CHUNKS = {}          # (device index, capture seq) -> [tensor, position]: the chunk being filled
_TICKET_KEEP = []            # every chunk ever made, for the life of the process (32 KB each)
_TICKET_RING_INTS = 1 << 20
_TICKET_CHUNK_INTS = 1 << 13


def _tickets(n: int, like: torch.Tensor):
    """int32 [n] zeroed tickets for one in-launch-finalize call on ``like``'s device, or None when the call must not use them."""
    if not FIN_ON:
        return None
    from . import graphs
    dev = like.device.index or 0
    if graphs._CAPTURING > 0:
        key = (dev, graphs.CAPTURE_SEQ)
        ent = _TICKET_CHUNKS.get(key)
        if ent is None or ent[1] + n > ent[0].numel():
            ent = _TICKET_CHUNKS[key] = [torch.zeros(max(_TICKET_CHUNK_INTS, n), dtype=torch.int32, device=like.device), 0]
            _TICKET_KEEP.append(ent[0])              # (a full chunk stays allocated: its slices are baked into the graph)
        t = ent[0][ent[1]:ent[1] + n]
        ent[1] += n
        return t
    if torch.cuda.is_current_stream_capturing():
        return None
    ent = _TICKET_RING.get(dev)
    if ent is None:
        ent = _TICKET_RING[dev] = [torch.zeros(_TICKET_RING_INTS, dtype=torch.int32, device=like.device), 0]
    if ent[1] + n > _TICKET_RING_INTS:
        ent[1] = 0
    t = ent[0][ent[1]:ent[1] + n]
    ent[1] += n
    return t


def _fin_available(like: torch.Tensor) -> bool:
    """May a launch made NOW on ``like``'s device finalise in the launch?  Depends on the phase (eager, a GraphedPhase capture, somebody else's
    capture); asked through ``_tickets`` because the probe also makes the ring / the capture's chunk that the launches behind it draw from."""
    return _tickets(0, like) is not None


def _wu(w, transposed):
    """The prepared Winograd image of ``w`` for this form inside a ``wino_prepared`` scope (the `_pre` argument), else None."""
    return _WINO_ACTIVE.get((w.data_ptr(), transposed & 1)) if _WINO_ACTIVE else None


# ------------------------------------------------------------------------------------------- paired weight gradients
# A uganConsis iteration runs the generator twice with the same weights -- G(x_real) and the cycle pass G(x_fake) (reference
# trainer/uganConsisTrainer.py:152,159) -- and differentiates both passes in one G-step (:179), so every 3x3 layer has its weight
# gradient computed TWICE over 16 slices, and autograd adds the two.  At 16 slices the fixed part of a weight-gradient launch
# (prologue, first-row latency, cross-strip combine, slab store, the split-slab sum behind it) is a third of its time.  Inside
# ``pair_wgrads()`` scopes the fused blocks' backward therefore PAIRS the two passes: the node that runs first parks its operands
# (``_PAIR_STASH``, keyed by the weight's storage -- the cycle pass runs on parameter aliases of the same storage) and returns no
# weight gradient; the node of the other pass launches ONE ``smsut_conv2d_wgrad_pair`` over both image sets and returns the sum.
# Same products, summed in the kernel's accumulators instead of by a separate add; deterministic (autograd's order is).
# Where ``smsut_conv2d_wgrad_pair_supported`` says no, the two passes keep two launches.
_PAIR_FWD = False
_PAIR_STASH = {}


@contextlib.contextmanager
def pair_wgrads():
    """Forward scope: fused blocks run inside take part in weight-gradient pairing.  The caller guarantees that every weight used
    inside such scopes is used an EVEN number of times before ``pair_assert_empty()`` (the trainer: both generator passes)."""
    global _PAIR_FWD
    prev, _PAIR_FWD = _PAIR_FWD, True
    try:
        yield
    finally:
        _PAIR_FWD = prev


def pair_reset():
    """Forget parked operands (start of an iteration: an iteration that died half-way must not pair with the next one)."""
    _PAIR_STASH.clear()


def pair_flush():
    """End of the iteration's LAST backward (inside that phase, so that a captured phase holds these launches too): operand sets
    still parked have no partner in this iteration -- e.g. the cycle pass' segmentation branch gets no gradient before the
    consistency term switches on (reference uganConsisTrainer.py:165: iter >= 1000), so the G(x_real) nodes of that branch wait in
    vain -- and are computed alone, as they would have been without pairing, and handed to their weight's ``.grad``."""
    if not _PAIR_STASH:
        return 0
    n = 0
    for key in list(_PAIR_STASH):
        for mine, single, deliver in _PAIR_STASH.pop(key):
            deliver(single(mine))
            n += 1
    return n


def pair_assert_empty():
    """After ``pair_flush()``: nothing may be parked across iterations."""
    if _PAIR_STASH:
        n = sum(len(v) for v in _PAIR_STASH.values())
        _PAIR_STASH.clear()
        raise RuntimeError(f"ops.pair_wgrads: {n} parked weight-gradient operand set(s) were never computed (pair_flush() missing "
                           "at the end of the iteration's last backward)")


def _add_grad(p, g):
    """What autograd's AccumulateGrad does for a leaf, for a gradient that arrives outside the engine (``pair_flush``)."""
    if p.grad is None:
        p.grad = g
    else:
        p.grad = p.grad + g


class WgradSet(NamedTuple):
    """One pass' operands of a fused block's 3x3 weight-gradient launch -- exactly what a parked entry keeps alive.  x2: the second part of a
    virtual cat; gs: the shortcut's output gradient (conv1 + shortcut in one launch); (mean, rstd) of x: normalised while staging (conv2 on y1)."""
    x: torch.Tensor; x2: Optional[torch.Tensor]; gy: torch.Tensor; gs: Optional[torch.Tensor]                     # noqa: E702
    mean: Optional[torch.Tensor]; rstd: Optional[torch.Tensor]; n: int                                            # noqa: E702


def _pair_wgrad(key, mine: WgradSet, launch, single, deliver):
    """Park ``mine`` under ``key`` and return None, or -- when the other pass is parked there -- launch the paired weight gradient over both
    sets and return gw [rows][ci][co] (flat).  ``launch``: what both sets share, (rows, ca, gamma, beta, slope, (h, w, ci, co)).  ``single(set)``:
    the one-set launch (flat: where the library refuses the pair at the partner's batch size; for ``pair_flush``, which hands it to ``deliver``)."""
    rows, ca, gamma, beta, slope, dims = launch
    lst = _PAIR_STASH.get(key)
    if not lst:
        _PAIR_STASH.setdefault(key, []).append((mine, single, deliver))
        return None
    other = lst.pop()[0]
    if not lst:
        del _PAIR_STASH[key]
    cat, aff, sc = int(mine.x2 is not None), int(mine.mean is not None), int(mine.gs is not None)
    if not H.call("smsut_conv2d_wgrad_pair_supported", mine.n, other.n, *dims, cat, aff, sc):
        return single(mine) + single(other)
    gw = torch.empty(rows * dims[2] * dims[3], dtype=torch.float32, device=mine.x.device)
    ws = _ws(H.call("smsut_conv2d_wgrad_pair_ws", mine.n, other.n, *dims, cat, aff, sc), mine.x)
    H.call("smsut_conv2d_wgrad_pair", *mine, *other, ca, gamma if aff else None, beta if aff else None, float(slope), gw, ws, *dims, _s())
    return gw


class BlockPlan(NamedTuple):
    """What one fused BasicBlock launches: decided once, at the top of ``BasicBlockFn.forward`` (``_block_plan``), launched by the ``_bb_*``
    stages, carried to the backward as ``ctx.plan``.  Shapes and forms only, no tensors.  DESIGN.md 4b lists what sets each field and what
    each stage launches for it; cat: (ca, cb) of a block whose input is cat([xa, xb], 1); t3 / t3b: statistics tiles of conv1 / conv2."""
    n: int; h: int; w: int; ci: int; co: int                                                                      # noqa: E702
    cat: Optional[tuple]; has_sc: bool; virtual: bool; pool: bool; slope: float                                   # noqa: E702
    f16a: bool; f16: bool; hs: bool; fused_sc: bool; fin: bool; inaff: bool; pair: bool                           # noqa: E702
    t3: int; t3b: int                                                                                             # noqa: E702


def _block_plan(like, cat, virtual, co, has_sc, slope, pool) -> BlockPlan:
    n, ci, h, w = like.shape
    ci, vc = (cat[0] + cat[1], 1) if virtual else (ci, 0)
    # fp16 operands (config 5): both 3x3 convs of the block and their gradients, when every reduction is whole 16-channel chunks; same tile
    # selection / statistics layout as the fp32 forms  (per conv: the 8 -> 16 first block keeps conv1 in fp32 -- half of a 16-channel chunk
    # would be padding -- but its 16 -> 16 conv2 qualifies)
    f16a = CONV_F16 and ci % 16 == 0 and co % 16 == 0
    f16 = CONV_F16 and co % 16 == 0
    t3 = H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 3, int(f16a))    # tile shape depends on (N, H, W, Cin, Cout, dtype)
    t3b = H.call("smsut_conv2d_mfma_tiles", n, h, w, co, co, 3, int(f16))
    # conv1 and the 1x1 shortcut read the same block input: one pass (the shortcut is conv1's centre tap with its own weights)
    fused_sc = has_sc and bool(H.call("smsut_conv2d_fwd_sc_f16_supported" if f16a else "smsut_conv2d_fwd_sc_supported", n, h, w, ci, co, vc))
    # fp16 operands: the block-internal raw conv outputs y1, y2, s never leave the block -- stored as fp16 (half the HBM bytes
    # of every pass over them: conv epilogues, IN apply, both tail passes, the BST mask read), arithmetic on them in fp32
    # (the 8 -> 16 first block: conv1 stays on fp32 operands -- the 8-channel form has no fp16 twin -- and stores fp16 all the same)
    hs = ((f16a or ci == 8) and f16 and fused_sc and bool(H.call("smsut_conv2d_f16_hs_supported", n, h, w, ci, co, vc))
          and bool(H.call("smsut_conv2d_f16_hs_supported", n, h, w, co, co, 0)))
    # conv2 / wgrad2 normalise y1 while staging, for blocks of whole 16-channel tiles (r04: the register-row weight gradient takes
    # the transform for +3 us at 16 -> 16 @256^2; the LDS-staged 16-channel kernel paid +55 us, which kept the 16-channel blocks
    # out until then: uganConsis -1.0 %, U-Net -1.0 %)
    inaff = not f16 and co % 16 == 0 and bool(H.call("smsut_conv2d_mfma_persistent", n, h, w, co, co, 3, 0))
    # in-launch finalize of all three statistics sets of the block (fp32, fused shortcut, conv2 on the raw y1: the forms whose
    # kernels carry it) -- decided once, so that the block never mixes the two ways for one statistics set
    fin = fused_sc and not (f16a or hs) and inaff and _fin_available(like)
    return BlockPlan(n, h, w, ci, co, cat, has_sc, virtual, pool, slope, f16a, f16, hs, fused_sc, fin, inaff, _PAIR_FWD and not CONV_F16, t3, t3b)


def _bb_conv1(p: BlockPlan, x, x2, w1, ws, st):
    """conv1 (+ the 1x1 shortcut: ``fused_sc``) with statistics from the epilogue; (x, x2): the parts of a virtual cat, else (x, None)."""
    n, h, w, ci, co = p[:5]
    act_dt = torch.float16 if p.hs else torch.float32
    s = ps = ms = rs = None
    p1 = _ws(n * p.t3 * co * 2, x)
    y1 = new_act(n, co, h, w, x, act_dt)
    if p.fused_sc:
        s, ps = new_act(n, co, h, w, x, act_dt), _ws(n * p.t3 * co * 2, x)
    m1, r1 = _vec(x, n, co), _vec(x, n, co)
    if p.hs:
        H.call("smsut_conv2d_fwd_mfma_stats_sc_f16_hs", x, x2, w1, ws, y1, s, p1, ps, n, h, w, ci, co, st)
    elif p.fin:
        # statistics of y1 AND of the shortcut finalised inside the launch (no smsut_in_finalize_* behind it)
        ms, rs = _vec(x, n, co), _vec(x, n, co)
        H.call("smsut_conv2d_fwd_mfma_stats_sc_fin", x, x2, w1, ws, y1, s, p1, ps, _tickets(n, x), m1, r1, ms, rs, IN_EPS,
               n, h, w, ci, co, _wu(w1, 0), st)
    elif p.fused_sc:
        _conv3("smsut_conv2d_fwd_mfma_stats_sc_f16" if p.f16a else "smsut_conv2d_fwd_mfma_stats_sc", w1, 0, x, x2, w1, ws, y1, s,
               p1, ps, n, h, w, ci, co, st)
    elif p.virtual:
        _conv3("smsut_conv2d_fwd_mfma_stats_cat_f16" if p.f16a else "smsut_conv2d_fwd_mfma_stats_cat", w1, 0, x, x2, w1, y1, p1, n, h, w, ci, co, st)
    else:
        _conv3("smsut_conv2d_fwd_mfma_stats_f16" if p.f16a else "smsut_conv2d_fwd_mfma_stats", w1, 0, x, w1, y1, p1, n, h, w, ci, co, 3, st)
    return y1, p1, m1, r1, s, ps, ms, rs


def _bb_conv2(p: BlockPlan, y1, p1, m1, r1, g1, b1, w2, ps, ms, rs, st):
    """conv2 on act(IN1(y1)), normalised while staging (``inaff``, ``hs``) or applied into a1 first; then the statistics still due."""
    n, h, w, _, co = p[:5]
    hw, slope, a1 = h * w, p.slope, None
    y2 = new_act(n, co, h, w, y1, torch.float16 if p.hs else torch.float32)
    p2 = _ws(n * p.t3b * co * 2, y1)
    if p.fin:                                            # (m2, r2 -- like m1, r1, ms, rs -- written by the conv launch itself)
        m2, r2 = _vec(y1, n, co), _vec(y1, n, co)
        H.call("smsut_conv2d_fwd_mfma_stats_inaff_fin", y1, w2, y2, p2, m1, r1, g1, b1, slope, _tickets(n, y1), m2, r2, IN_EPS,
               n, h, w, co, co, _wu(w2, 0), st)
    elif p.inaff:
        # conv2 (and later its weight gradient) normalise the raw conv1 output while staging their tiles: a1 is never built
        H.call("smsut_in_finalize_fwd", p1, p.t3, m1, r1, n, hw, co, IN_EPS, st)
        _conv3("smsut_conv2d_fwd_mfma_stats_inaff", w2, 0, y1, w2, y2, p2, m1, r1, g1, b1, slope, n, h, w, co, co, st)
    elif p.hs:
        # conv2 (and later its weight gradient) widen the raw fp16 y1, normalise + activate and round it while staging: the
        # operand bits smsut_instnorm_fwd_partials_hs2 would have stored -- a1 and the pass that writes it disappear
        H.call("smsut_in_finalize_fwd", p1, p.t3, m1, r1, n, hw, co, IN_EPS, st)
        H.call("smsut_conv2d_fwd_mfma_stats_inaff_f16_hsx", y1, w2, y2, p2, m1, r1, g1, b1, slope, n, h, w, co, co, st)
    else:
        a1 = new_act(n, co, h, w, y1)
        H.call("smsut_instnorm_fwd_partials", y1, g1, b1, a1, m1, r1, p1, p.t3, n, hw, co, IN_EPS, slope, 1, st)
        _conv3("smsut_conv2d_fwd_mfma_stats_f16" if p.f16 else "smsut_conv2d_fwd_mfma_stats", w2, 0, a1, w2, y2, p2, n, h, w, co, co, 3, st)
    if not p.fin:
        m2, r2 = _vec(y1, n, co), _vec(y1, n, co)
        if p.fused_sc:
            ms, rs = _vec(y1, n, co), _vec(y1, n, co)    # both sets are due now: ONE launch of the latency-bound finalize
            H.call("smsut_in_finalize_fwd2", p2, p.t3b, m2, r2, ps, p.t3, ms, rs, n, hw, co, IN_EPS, st)
        else:
            H.call("smsut_in_finalize_fwd", p2, p.t3b, m2, r2, n, hw, co, IN_EPS, st)
    return y2, a1, m2, r2, ms, rs


def _bb_shortcut(p: BlockPlan, x, x2, ws, st):
    """The 1x1 shortcut as a launch of its own (no fused form for the shape) and its statistics."""
    n, h, w, ci, co = p[:5]
    hw, s = h * w, new_act(n, co, h, w, x)
    t1s = H.call("smsut_conv1x1_tiles", n, hw, co) if H.call("smsut_conv1x1_supported", ci, co) else 0     # the streaming 1x1 kernel's
    t1 = t1s if (t1s or p.virtual) else H.call("smsut_conv2d_mfma_tiles", n, h, w, ci, co, 1, 0)   # (virtual: basic_block_cat_fusable saw t1s > 0)
    ps = _ws(n * t1 * co * 2, x)
    if p.virtual:
        H.call("smsut_conv1x1_fwd_cat", x, x2, p.cat[0], ws, s, ps, n, hw, ci, co, st)
    elif t1s:
        H.call("smsut_conv1x1_fwd", x, ws, s, ps, n, hw, ci, co, 0, st)
    else:
        H.call("smsut_conv2d_fwd_mfma_stats", x, ws, s, ps, n, h, w, ci, co, 1, st)
    ms, rs = _vec(x, n, co), _vec(x, n, co)
    H.call("smsut_in_finalize_fwd", ps, t1, ms, rs, n, hw, co, IN_EPS, st)
    return s, ms, rs


def _bb_tail(p: BlockPlan, y2, m2, r2, g2, b2, s, ms, rs, gs, bs, st):
    """IN2, the shortcut's IN, the residual add and the activation in one pass (+ the level's max-pool).  -> out, pooled, pool_idx"""
    n, h, w, _, co = p[:5]
    out, pooled, idx = new_act(n, co, h, w, y2), None, None
    if p.pool:
        pooled = new_act(n, co, h // 2, w // 2, y2)
        idx = torch.empty(n * (h // 2) * (w // 2) * co, dtype=torch.uint8, device=y2.device)
        H.call("smsut_restail_fwd_pool", y2, m2, r2, g2, b2, s, ms, rs, gs, bs, out, pooled, idx, n, h, w, co, p.slope, int(p.hs), st)
    else:
        H.call("smsut_restail_fwd_hs" if p.hs else "smsut_restail_fwd", y2, m2, r2, g2, b2, s, ms, rs, gs, bs, out, n, h * w, co, p.slope, st)
    return out, pooled, idx


class BlockBwd(NamedTuple):
    """The backward's own decisions (``_block_bwd_plan``, at the top of ``BasicBlockFn.backward``)."""
    chunks: int                           # partial-sum chunks of the InstanceNorm-backward reductions
    nb: int; amax1: bool                  # amax handover: slots per tensor of [gy2 | gs_t | gy1], 0 = none / max |gy1| comes too       # noqa: E702
    tail: str; fin_ok: bool               # "pool" | "hs" | "amax" | "fin" | "plain" / the tail's backward may finalise in its launch   # noqa: E702
    pers2: bool; fin_b: bool              # conv2's data-gradient emits the IN-backward partial sums / and finalises them       # noqa: E702
    f16w1: bool; f16w2: bool              # fp16-operand weight gradient of conv1 / conv2                             # noqa: E702
    pair1: bool; pair2: bool              # the weight gradient of conv1 + shortcut / conv2 goes through ``_pair_wgrad``   # noqa: E702
    fused_wsc16: bool; fused_wsc: bool    # conv1's and the shortcut's weight gradients in one pass over x: fp16 / any operands  # noqa: E702
    fused_dsc16: bool                     # their data-gradients in one pass on fp16 operands (asked for: it decides the scale)
    dx: Optional[str]                     # block-input gradient: None (not wanted) | "sc_f16" | "sc" | "split" | "accum" | "accum_k1"


def _block_bwd_plan(p: BlockPlan, needs, mp, fin_available) -> BlockBwd:
    """``mp``: both outputs of a pool block bring a gradient; ``fin_available()``: the finalize probe of THIS phase (the forward may
    have run in another), asked at most once and only where a launch could use it."""
    n, h, w, ci, co = p[:5]
    f16a, f16, hs, has_sc, cat = p.f16a, p.f16, p.hs, p.has_sc, p.cat is not None
    needs = tuple(needs) + (False,) * (14 - len(needs))  # (``basic_block`` passes no xa, xb, pool: their entries are missing, not False)
    chunks = H.call("smsut_in_chunks", n, h * w, co)
    # fp16 operands: the kernels that write gy2 / gs_t / gy1 hand their absolute maxima over (one slot per workgroup:
    # [gy2 | gs_t | gy1], nb each), the scales of the gradient operands come from those slots instead of a pass over each tensor
    nb = H.call("smsut_amax_blocks", n, h * w, co) if (f16 or f16a) and AMAX_HANDOVER else 0
    fin_ok = not hs and not nb and (mp or has_sc) and fin_available()
    tail = "pool" if mp else "hs" if hs else "amax" if nb else "fin" if fin_ok else "plain"
    pers2 = bool(H.call("smsut_conv2d_mfma_persistent", n, h, w, co, co, 3, int(f16)))
    fin_b = pers2 and p.fin and fin_ok                   # (p.fin: fp32 operands, conv shortcut -- so the probe above was made)
    amax1 = pers2 and nb > 0 and (hs or f16a)
    f16w2 = f16 and bool(H.call("smsut_conv2d_wgrad_f16_supported", n, h, w, co, co))
    f16w1 = f16a and bool(H.call("smsut_conv2d_wgrad_f16_supported", n, h, w, ci, co))
    # (p.pair: fp32 operands -- no hs, no f16w*, no fused_wsc16 -- so the pair queries are asked where the fp32 launches are due)
    pair2 = p.pair and bool(H.call("smsut_conv2d_wgrad_pair_supported", n, n, h, w, co, co, 0, int(p.inaff), 0))
    split_c = p.cat[0] if cat else 0
    fused_wsc16 = has_sc and f16w1 and bool(H.call("smsut_conv2d_wgrad_sc_f16_supported", n, h, w, ci, co))
    fused_dsc16 = (has_sc and f16a and (needs[0] or needs[11] or needs[12])
                   and bool(H.call("smsut_conv2d_dgrad_sc_f16_supported", n, h, w, co, ci, split_c)))
    fused_wsc = fused_wsc16 or (has_sc and not f16w1 and bool(H.call("smsut_conv2d_wgrad_sc_supported", n, h, w, ci, co)))
    pair1 = p.pair and fused_wsc and bool(H.call("smsut_conv2d_wgrad_pair_supported", n, n, h, w, ci, co, int(p.virtual), 0, 1))
    dx = None
    if (needs[11] or needs[12]) if cat else needs[0]:
        if fused_dsc16:
            dx = "sc_f16"
        elif has_sc and not f16a and H.call("smsut_conv2d_dgrad_sc_supported", n, h, w, co, ci, split_c):
            dx = "sc"
        elif (cat and has_sc and split_c % 16 == 0 and H.call("smsut_conv1x1_supported", co, ci)
                and H.call("smsut_conv2d_mfma_split_supported", n, h, w, co, ci, split_c)):
            dx = "split"
        else:
            dx = "accum" if not has_sc or H.call("smsut_conv1x1_supported", co, ci) else "accum_k1"    # (the shortcut's: streaming 1x1 | MFMA k = 1)
    return BlockBwd(chunks, nb, amax1, tail, fin_ok, pers2, fin_b, f16w1, f16w2, pair1, pair2, fused_wsc16, fused_wsc, fused_dsc16, dx)


def _bb_tail_bwd(p: BlockPlan, b: BlockBwd, g_out, g_pooled, pool_idx, out, y2, m2, r2, g2, b2, s, ms, rs, gs, bs, st):
    """Residual tail: gradients of both raw conv outputs (or of the identity) in one reduce + one apply pass."""
    n, h, w, _, co = p[:5]
    hw, slope = h * w, p.slope
    gy2, gs_t = new_act(n, co, h, w, y2), new_act(n, co, h, w, y2)
    a_t, b2_t, bs_t = _vec(y2, n, co), _vec(y2, n, co), _vec(y2, n, co)
    gg2, gb2 = _vec(y2, co), _vec(y2, co)
    ggs, gbs = (_vec(y2, co), _vec(y2, co)) if p.has_sc else (None, None)
    amax = _vec(y2, 3 * b.nb) if b.nb else None
    tk = _tickets(n, y2) if b.tail == "pool" and b.fin_ok else None
    io = (y2, m2, r2, g2, b2, s, ms, rs, gs, bs, gy2, gs_t, a_t, b2_t, bs_t, gg2, gb2, ggs, gbs, _ws(n * b.chunks * co * 3, y2))
    if b.tail == "pool":
        H.call("smsut_restail_bwd_pool", g_out, g_pooled, pool_idx, *io, tk, amax, n, h, w, co, slope, int(p.hs), st)
    elif b.tail in ("hs", "amax"):
        H.call("smsut_restail_bwd_hs" if p.hs else "smsut_restail_bwd_amax", g_out, out, *io, amax, n, hw, co, slope, st)
    elif b.tail == "fin":
        # the per-image means of the tail's backward finalised inside the partial-sum launch (two launches instead of three)
        H.call("smsut_restail_bwd_fin", g_out, out, *io, _tickets(n, y2), n, hw, co, slope, st)
    else:
        H.call("smsut_restail_bwd", g_out, out, *io, n, hw, co, slope, st)
    return gy2, gs_t, gg2, gb2, ggs, gbs, amax


def _bb_dgrad2(p: BlockPlan, b: BlockBwd, gy2, w2, y1, m1, r1, g1, b1, amax, st):
    """conv2's data-gradient + IN1 / LeakyReLU backward (mask recomputed from y1).  -> gy1, gg1, gb1, sc2 (the scale of gy2)"""
    n, h, w, _, co = p[:5]
    hw, slope, f16, hs, nb = h * w, p.slope, p.f16, p.hs, b.nb
    ga1, gy1 = new_act(n, co, h, w, gy2), new_act(n, co, h, w, gy2)
    a1m, b1m, gg1, gb1 = _vec(gy2, n, co), _vec(gy2, n, co), _vec(gy2, co), _vec(gy2, co)
    sc2 = (_grad_scale_from(amax[:nb]) if amax is not None else _grad_scale(gy2)) if f16 else None   # serves conv2's data- and weight-gradient
    if not b.pers2:
        if f16:
            H.call("smsut_conv2d_fwd_mfma_f16", gy2, w2, ga1, sc2, n, h, w, co, co, 3, 1, st)
        else:
            _conv3("smsut_conv2d_fwd_mfma", w2, 1, gy2, w2, ga1, n, h, w, co, co, 3, 1, st)
        H.call("smsut_instnorm_bwd", ga1, y1, b1, m1, r1, g1, gy1, a1m, b1m, gg1, gb1, _ws(n * b.chunks * co * 3, gy2), n, hw, co, slope, st)
        return gy1, gg1, gb1, sc2
    # the dgrad epilogue masks its result and emits the InstanceNorm-backward partial sums: no reduction pass
    pb = _ws(n * p.t3b * co * 2, gy2)                    # (the tiles of conv2's forward: same shape, same operand dtype)
    if f16:
        H.call("smsut_conv2d_dgrad_mfma_bwdstats_f16_hs" if hs else "smsut_conv2d_dgrad_mfma_bwdstats_f16", gy2, w2, ga1, pb, y1, m1, r1, g1, b1,
               sc2, slope, n, h, w, co, co, st)
    elif b.fin_b:                                        # in-launch finalize of the backward pair: a1m, b1m written by the launch itself
        H.call("smsut_conv2d_dgrad_mfma_bwdstats_fin", gy2, w2, ga1, pb, y1, m1, r1, g1, b1, slope, _tickets(n, gy2), a1m, b1m,
               n, h, w, co, co, _wu(w2, 1), st)
    else:
        _conv3("smsut_conv2d_dgrad_mfma_bwdstats", w2, 1, gy2, w2, ga1, pb, y1, m1, r1, g1, b1, slope, n, h, w, co, co, st)
    if not b.fin_b:
        H.call("smsut_in_finalize_bwd", pb, p.t3b, a1m, b1m, n, hw, co, st)
    if hs or b.amax1:
        H.call("smsut_in_apply_bwd_hs" if hs else "smsut_in_apply_bwd_amax", ga1, y1, m1, r1, g1, a1m, b1m, gy1, gg1, gb1,
               amax[2 * nb:] if b.amax1 else None, n, hw, co, st)
    else:
        H.call("smsut_in_apply_bwd", ga1, y1, m1, r1, g1, a1m, b1m, gy1, gg1, gb1, n, hw, co, st)
    return gy1, gg1, gb1, sc2


def _bb_wgrad2(p: BlockPlan, b: BlockBwd, pair_w, y1, a1, gy2, w2, sc2, m1, r1, g1, b1, st):
    """conv2's weight gradient; None when the operands were parked for the other generator pass (``_pair_wgrad``)."""
    (n, h, w, _, co), slope = p[:5], p.slope
    if p.hs or b.f16w2:
        gw2 = new_weight(co, co, 3, 3, device=gy2.device)
        wws = _ws(H.call("smsut_conv2d_wgrad_f16_ws", n, h, w, co, co), gy2)
        if p.hs:
            H.call("smsut_conv2d_wgrad_f16_xh_inaff", y1, gy2, gw2, wws, sc2, m1, r1, g1, b1, slope, n, h, w, co, co, st)
        else:
            H.call("smsut_conv2d_wgrad_f16", a1, None, 0, gy2, gw2, wws, sc2, n, h, w, co, co, st)
        return gw2

    def single2(t):                                      # -> flat [9][co][co]
        g = _vec(t.x, 9 * co * co)
        wws2 = _ws(H.call("smsut_conv2d_wgrad_mfma_ws", t.n, h, w, co, co, 3), t.x)
        if t.mean is not None:
            H.call("smsut_conv2d_wgrad_mfma_inaff", t.x, t.gy, g, wws2, t.mean, t.rstd, g1, b1, slope, t.n, h, w, co, co, _s())
        else:
            H.call("smsut_conv2d_wgrad_mfma", t.x, t.gy, g, wws2, t.n, h, w, co, co, 3, _s())
        return g
    as_w2 = lambda g: torch.as_strided(g, (co, co, 3, 3), hwio_strides(co, co, 3, 3))     # noqa: E731
    mine2 = WgradSet(y1, None, gy2, None, m1, r1, n) if p.inaff else WgradSet(a1, None, gy2, None, None, None, n)
    if not b.pair2:
        return as_w2(single2(mine2))
    # the other generator pass through this layer is (or will be) parked under the weight's storage: one launch for both
    leaf2 = pair_w[1]
    gw2 = _pair_wgrad(("w2", w2.data_ptr()), mine2, (9, 0, g1, b1, slope, (h, w, co, co)), single2, lambda g: _add_grad(leaf2, as_w2(g)))
    return None if gw2 is None else as_w2(gw2)


def _bb_wgrad1(p: BlockPlan, b: BlockBwd, pair_w, x, x2, gy1, gs_t, w1, amax, st):
    """Weight gradients of conv1 and of the shortcut; (x, x2, ca): the parts of a virtual cat, else (x, None, 0).  -> gw1, gws (None,
    None when the operands were parked for the other generator pass), sc1 (fp16 operands: the scale of conv1's gradient operand)"""
    n, h, w, ci, co = p[:5]
    hw, ca = h * w, (p.cat[0] if p.virtual else 0)
    as_w1 = lambda g: torch.as_strided(g, (co, ci, 3, 3), hwio_strides(co, ci, 3, 3))                     # noqa: E731
    as_ws = lambda g: torch.as_strided(g, (co, ci, 1, 1), hwio_strides(co, ci, 1, 1), 9 * ci * co)        # noqa: E731
    # fp16 operands: the fused-shortcut kernels read [gy1 | gs_t] as ONE operand -> one scale over both tensors
    if not p.f16a:
        sc1 = None
    elif b.fused_wsc16 or b.fused_dsc16:
        sc1 = _grad_scale_from(amax[b.nb:]) if b.amax1 else _grad_scale2(gy1, gs_t)
    else:
        sc1 = _grad_scale_from(amax[2 * b.nb:]) if b.amax1 else _grad_scale(gy1)
    # fused: both weight gradients in one pass over x: rows 0..8 = conv1's taps, row 9 = the 1x1 shortcut's
    if b.fused_wsc16:
        g10 = _vec(x, 10 * ci * co)
        H.call("smsut_conv2d_wgrad_sc_f16", x, x2, ca, gy1, gs_t, g10, _ws(H.call("smsut_conv2d_wgrad_sc_f16_ws", n, h, w, ci, co), x),
               sc1, n, h, w, ci, co, st)
        return as_w1(g10), as_ws(g10), sc1
    if b.fused_wsc:
        def single1(t):                                  # -> flat [10][ci][co]
            g = _vec(t.x, 10 * ci * co)
            H.call("smsut_conv2d_wgrad_mfma_sc", t.x, t.x2, ca, t.gy, t.gs, g,
                   _ws(H.call("smsut_conv2d_wgrad_sc_ws", t.n, h, w, ci, co), t.x), t.n, h, w, ci, co, _s())
            return g
        mine1 = WgradSet(x, x2, gy1, gs_t, None, None, n)
        if b.pair1:
            leaf1, leafs = pair_w[0], pair_w[2]
            g10 = _pair_wgrad(("w1", w1.data_ptr()), mine1, (10, ca, None, None, p.slope, (h, w, ci, co)), single1,
                              lambda g: (_add_grad(leaf1, as_w1(g)), _add_grad(leafs, as_ws(g))))
        else:
            g10 = single1(mine1)
        return (None, None, sc1) if g10 is None else (as_w1(g10), as_ws(g10), sc1)     # (None: parked for the other pass / pair_flush)
    gw1 = new_weight(co, ci, 3, 3, device=x.device)
    wws = _ws(H.call("smsut_conv2d_wgrad_f16_ws", n, h, w, ci, co) if b.f16w1 else H.call("smsut_conv2d_wgrad_mfma_ws", n, h, w, ci, co, 3), x)
    if b.f16w1:
        H.call("smsut_conv2d_wgrad_f16", x, x2, ca, gy1, gw1, wws, sc1, n, h, w, ci, co, st)
    elif p.virtual:
        H.call("smsut_conv2d_wgrad_mfma_cat", x, x2, ca, gy1, gw1, wws, n, h, w, ci, co, 3, st)
    else:
        H.call("smsut_conv2d_wgrad_mfma", x, gy1, gw1, wws, n, h, w, ci, co, 3, st)
    if not p.has_sc:
        return gw1, None, sc1
    gws = new_weight(co, ci, 1, 1, device=x.device)
    wws1 = _ws(H.call("smsut_conv1x1_wgrad_ws", n, hw, ci, co), x)
    if p.virtual:
        H.call("smsut_conv1x1_wgrad_cat", x, x2, ca, gs_t, gws, wws1, n, hw, ci, co, st)
    else:
        H.call("smsut_conv1x1_wgrad", x, gs_t, gws, wws1, n, hw, ci, co, st)
    return gw1, gws, sc1


def _bb_dgrad1(p: BlockPlan, b: BlockBwd, gy1, gs_t, w1, ws, sc1, st):
    """Block-input gradient (conv1's data-gradient + the shortcut's, the identity's being gs_t itself) into the parts (ga, gb) of a cat or into
    gx.  ONE ladder for both: fused fp16, fused fp32, (cat) split 1x1 + split 3x3 on top, shortcut first + the 3x3 accumulating on top."""
    n, h, w, ci, co = p[:5]
    hw, split = h * w, p.cat is not None
    ca, cb = p.cat if split else (0, 0)
    ga, gb = (new_act(n, ca, h, w, gy1), new_act(n, cb, h, w, gy1)) if split else (None, None)
    gx = None if (split and b.dx[:5] != "accum") else new_act(n, ci, h, w, gy1) if p.has_sc else gs_t
    d0, d1 = (ga, gb) if split else (gx, None)           # where the fused forms write
    if b.dx == "sc_f16":
        H.call("smsut_conv2d_dgrad_mfma_sc_f16", gy1, gs_t, w1, ws, d0, d1, sc1, ca, n, h, w, co, ci, st)
    elif b.dx == "sc":
        # conv1's and the shortcut's data-gradients in ONE pass (the shortcut's is the centre tap of a second
        # reduction half), written straight into the destination: no 1x1 kernel, no accumulate pass
        H.call("smsut_conv2d_dgrad_mfma_sc", gy1, gs_t, w1, ws, d0, d1, ca, n, h, w, co, ci, st)
    elif b.dx == "split":
        # shortcut gradient first, the 3x3 data-gradient accumulates on top -- both straight into (ga, gb)
        H.call("smsut_conv1x1_fwd_split", gs_t, ws, ga, gb, ca, n, hw, co, ci, 1, st)
        if p.f16a:
            H.call("smsut_conv2d_fwd_mfma_split_f16", gy1, w1, ga, gb, sc1, ca, n, h, w, co, ci, 3, st)
        else:
            _conv3("smsut_conv2d_fwd_mfma_split", w1, 1, gy1, w1, ga, gb, ca, n, h, w, co, ci, 3, st)
    else:
        # the shortcut's gradient lands in gx first; the 3x3 data-gradient then accumulates into it in its store
        # epilogue (transposed | 2), which replaces a separate 3-pass add
        if b.dx == "accum_k1":
            H.call("smsut_conv2d_fwd_mfma", gs_t, ws, gx, n, h, w, co, ci, 1, 1, st)
        elif p.has_sc:
            H.call("smsut_conv1x1_fwd", gs_t, ws, gx, None, n, hw, co, ci, 1, st)
        if p.f16a:
            H.call("smsut_conv2d_fwd_mfma_f16", gy1, w1, gx, sc1, n, h, w, co, ci, 3, 3, st)
        else:
            _conv3("smsut_conv2d_fwd_mfma", w1, 1, gy1, w1, gx, n, h, w, co, ci, 3, 3, st)
        if split:
            H.call("smsut_concat2", ga, ca, gb, cb, gx, n * hw, 1, st)
    return (None, ga, gb) if split else (gx, None, None)


class BasicBlockFn(Function):
    """out = act(IN(conv3x3(act(IN(conv3x3(x))))) + IN(conv1x1(x)) | x)   (network/blocks.py:53-80).

    Forward: every conv emits the InstanceNorm statistics of its output from its epilogue; IN2, the shortcut's IN, the
    residual add and the activation are ONE pass (``smsut_restail_fwd``) -- z2 / zs never exist in HBM.
    Backward: the tail is one reduce + one apply pass producing the gradients of both raw conv outputs.
    (Also tried and measured slower on MI355X, r01: applying act(IN(.)) in conv2's / wgrad2's input staging and the
    LeakyReLU-mask + IN-backward sums in dgrad2's epilogue -- the extra VALU work and the registers it needs, 102 -> 157
    VGPRs, cost the MFMA kernels more than the memory passes they remove.)  First-order only (generator / U-Net)."""

    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, ws, gs, bs, slope, xa=None, xb=None, pool=False):
        # pool (r05): the block closes an encoder level -- returns (out, max_pool2(out)); the residual tail writes both in one pass and
        # the backward takes the two gradients (skip connection, pooled path) without a pooling-backward pass (smsut_restail_*_pool)
        # xa, xb (optional): x is cat([xa, xb], 1), already materialised and passed detached; the backward then writes the
        # block-input gradient straight into the two parts (split-output data-gradients) instead of returning d/dx
        # x None (with xa, xb): the cat is never materialised -- conv1, the shortcut and their weight gradients read the two
        # parts in place (virtual-cat entry points; chunk order and arithmetic of the materialised cat: same bits)
        leaves = (w1, w2, ws)                        # (as passed: the tensors autograd accumulates into)
        cat = (xa.shape[1], xb.shape[1]) if xa is not None else None
        x, x2 = (nhwc(xa), nhwc(xb)) if x is None else (nhwc(x), None)
        w1, w2, ws = hwio(w1), hwio(w2), (hwio(ws) if ws is not None else None)
        p = ctx.plan = _block_plan(x, cat, x2 is not None, w1.shape[0], ws is not None, float(slope), bool(pool))
        st = _s()
        y1, p1, m1, r1, s, ps, ms, rs = _bb_conv1(p, x, x2, w1, ws, st)
        y2, a1, m2, r2, ms, rs = _bb_conv2(p, y1, p1, m1, r1, g1, b1, w2, ps, ms, rs, st)
        if p.has_sc and not p.fused_sc:
            s, ms, rs = _bb_shortcut(p, x, x2, ws, st)
        out, pooled, ctx.pool_idx = _bb_tail(p, y2, m2, r2, g2, b2, s if p.has_sc else x, ms, rs, gs, bs, st)
        ctx.pair_w = leaves if p.pair else None      # the leaves a parked set's gradient goes to if it never meets a partner
        # (pool: an output that brought no gradient reaches the backward as None, not as an NCHW tensor of zeros to convert and route)
        ctx.set_materialize_grads(False)
        # ONE layout for the virtual-cat, conv-shortcut and identity forms: what a form lacks is None (identity: s is x itself)
        ctx.save_for_backward(x, x2, w1, w2, ws, y1, a1, y2, s, out, m1, r1, m2, r2, ms, rs, g1, b1, g2,
                              *((gs, b2, bs) if p.has_sc else (None, None, None)))
        return (out, pooled) if pool else out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_pooled=None):
        p = ctx.plan
        x, x2, w1, w2, ws, y1, a1, y2, s, out, m1, r1, m2, r2, ms, rs, g1, b1, g2, gs, b2, bs = ctx.saved_tensors
        if p.pool and g_out is None:                     # (no skip gradient: the pooled path's alone, through the plain pooling backward)
            g_out = new_act(p.n, p.co, p.h, p.w, x)
            H.call("smsut_maxpool2_bwd", nhwc(g_pooled), out, g_out, p.n, p.h, p.w, p.co, _s())
            g_pooled = None
        g_out = nhwc(g_out)
        mp = p.pool and g_pooled is not None             # two gradients: routed together inside the tail backward's loads
        g_pooled = nhwc(g_pooled) if mp else None
        b = _block_bwd_plan(p, ctx.needs_input_grad, mp, lambda: _fin_available(x))
        st = _s()
        gy2, gs_t, gg2, gb2, ggs, gbs, amax = _bb_tail_bwd(p, b, g_out, g_pooled, ctx.pool_idx, out, y2, m2, r2, g2, b2,
                                                           s if p.has_sc else x, ms, rs, gs, bs, st)    # (identity: s is x itself)
        # (forking the three weight-gradient launches to a second stream inside this node was measured 1-3 % SLOWER
        #  than the single-stream order below -- profiles/r01_notes.md)
        gy1, gg1, gb1, sc2 = _bb_dgrad2(p, b, gy2, w2, y1, m1, r1, g1, b1, amax, st)
        gw2 = _bb_wgrad2(p, b, ctx.pair_w, y1, a1, gy2, w2, sc2, m1, r1, g1, b1, st)
        gw1, gws, sc1 = _bb_wgrad1(p, b, ctx.pair_w, x, x2, gy1, gs_t, w1, amax, st)
        gx, ga, gb = _bb_dgrad1(p, b, gy1, gs_t, w1, ws, sc1, st) if b.dx else (None, None, None)
        return gx, gw1, gg1, gb1, gw2, gg2, gb2, gws, ggs, gbs, None, ga, gb, None


class CatParts:
    """Deferred ``torch.cat([a, b], 1)`` (UpSampleAndConcat, network/blocks.py:49-50).  A fused BasicBlock reads the two parts in
    place (``basic_block_cat``) and never builds the cat; any other consumer calls ``tensor()``."""
    __slots__ = ("a", "b", "_t")

    def __init__(self, a, b):
        self.a, self.b, self._t = a, b, None

    @property
    def shape(self):
        return torch.Size((self.a.shape[0], self.a.shape[1] + self.b.shape[1], self.a.shape[2], self.a.shape[3]))

    def tensor(self):
        if self._t is None:
            self._t = concat_channels(self.a, self.b)
        return self._t


def concat_channels_deferred(a, b):
    """cat([a, b], 1) whose materialisation is left to the consumer (see CatParts); a plain tensor when the virtual-cat
    kernels cannot apply (unequal or non-16-multiple halves, CPU tensors, switches off)."""
    if (VIRTUAL_CAT and SPLIT_DGRAD and FUSED_BLOCK and a.is_cuda and a.shape[1] == b.shape[1]
            and a.shape[1] % 16 == 0 and a.shape[0] == b.shape[0] and a.shape[2:] == b.shape[2:]):
        return CatParts(a, b)
    return concat_channels(a, b)


def basic_block_cat_fusable(parts, w1, ws):
    """Every consumer of the cat has a virtual-cat kernel for this shape: persistent 3x3 forward (Kdim 32 / 64), streaming
    1x1 shortcut with statistics tiles, MFMA weight gradients."""
    n, ca, h, w = parts.a.shape
    ci, co = 2 * ca, w1.shape[0]
    return (ws is not None and w1.shape[1] == ci and co % 4 == 0
            and H.call("smsut_conv2d_mfma_cat_supported", n, h, w, ci, co)
            and H.call("smsut_conv1x1_supported", ci, co) and H.call("smsut_conv1x1_tiles", n, h * w, co) > 0
            and H.call("smsut_conv2d_wgrad_mfma_supported", 3, 1, 1, ci, co))


def basic_block_cat(parts, w1, g1, b1, w2, g2, b2, ws, gs, bs, slope):
    return BasicBlockFn.apply(None, w1, g1, b1, w2, g2, b2, ws, gs, bs, slope, cl(parts.a), cl(parts.b))


BLOCK_POOL = bool(int(_os.environ.get("SMSUT_BLOCK_POOL", "1")))     # encoder level: the block's tail and the level's max-pool as one pass


def basic_block_pool_fusable(x, w1, ws):
    """The fused block applies, it has a conv shortcut (two-IN tail), whole channel quads, an even plane -- and a gradient is wanted
    (the inference path keeps block + pooling)."""
    return (BLOCK_POOL and ws is not None and basic_block_fusable(x, w1, ws) and w1.shape[0] % 4 == 0
            and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and torch.is_grad_enabled() and (x.requires_grad or w1.requires_grad)
            and getattr(x, "_smsut_cat_parts", None) is None)


def basic_block_pool(x, w1, g1, b1, w2, g2, b2, ws, gs, bs, slope):
    """(skip, pooled) of an encoder level whose block is fused with its MaxPool2d(2, 2)."""
    return BasicBlockFn.apply(cl(x), w1, g1, b1, w2, g2, b2, ws, gs, bs, slope, None, None, True)


def basic_block(x, w1, g1, b1, w2, g2, b2, ws, gs, bs, slope):
    parts = getattr(x, "_smsut_cat_parts", None)
    if parts is not None and SPLIT_DGRAD and ws is not None and torch.is_grad_enabled():
        # x = cat([up, skip]) (UpSampleAndConcat): gradients go to the two parts directly, the ConcatFn node is bypassed
        return BasicBlockFn.apply(cl(x).detach(), w1, g1, b1, w2, g2, b2, ws, gs, bs, slope, parts[0], parts[1])
    return BasicBlockFn.apply(cl(x), w1, g1, b1, w2, g2, b2, ws, gs, bs, slope)


# ------------------------------------------------------------------------------------------- activations / add
class AddActFn(Function):
    """y = LeakyReLU(a + b) (residual tail, network/blocks.py:78-79); b may be None."""

    @staticmethod
    def forward(ctx, a, b, slope):
        a = nhwc(a)
        if b is not None:
            b = nhwc(b)
            assert a.shape == b.shape
        y = new_act(*a.shape, a)
        H.call("smsut_add_act", a, b, y, a.numel(), float(slope), _s())
        ctx.save_for_backward(y)
        ctx.slope = float(slope)
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        g = ActBwdFn.apply(gy, y, ctx.slope)
        return g, (g if ctx.has_b else None), None


class ActBwdFn(Function):
    """gx = gy * LeakyReLU'(y); linear in gy, so it is its own derivative."""

    @staticmethod
    def forward(ctx, gy, y, slope):
        gy = nhwc(gy)
        gx = new_act(*y.shape, y)
        H.call("smsut_act_bwd", gy, y, gx, y.numel(), slope, _s())
        ctx.save_for_backward(y)
        ctx.slope = slope
        return gx

    @staticmethod
    def backward(ctx, gg):
        (y,) = ctx.saved_tensors
        return ActBwdFn.apply(gg, y, ctx.slope), None, None


def add_act(a, b, slope):
    return AddActFn.apply(cl(a), cl(b), slope)


def leaky_relu(x, slope):
    return AddActFn.apply(cl(x), None, slope)


class TanhFn(Function):
    @staticmethod
    def forward(ctx, x):
        x = nhwc(x)
        y = new_act(*x.shape, x)
        H.call("smsut_tanh_fwd", x, y, x.numel(), _s())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gy = nhwc(gy)
        gx = new_act(*y.shape, y)
        H.call("smsut_tanh_bwd", gy, y, gx, y.numel(), _s())
        return gx


def tanh(x):
    return TanhFn.apply(x)


# ------------------------------------------------------------------------------------------- pooling / resampling
class MaxPool2Fn(Function):
    """nn.MaxPool2d(2, 2) (network/blocks.py:128-134)."""

    @staticmethod
    def forward(ctx, x):
        x = nhwc(x)
        n, c, h, w = x.shape
        y = new_act(n, c, h // 2, w // 2, x)
        H.call("smsut_maxpool2_fwd", x, y, n, h, w, c, _s())
        ctx.save_for_backward(x)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        gy = nhwc(gy)
        n, c, h, w = x.shape
        gx = new_act(n, c, h, w, x)
        H.call("smsut_maxpool2_bwd", gy, x, gx, n, h, w, c, _s())
        return gx


class MaxPool2SkipFn(Function):
    """An encoder level's two uses of its block output x (network/blocks.py:131-133, ugan.py:50-52): returns
    (max_pool2(x), x) and sums the two incoming gradients inside the pooling backward kernel -- autograd's separate
    accumulation kernel over the full-resolution tensor (read 2, write 1) disappears."""

    @staticmethod
    def forward(ctx, x):
        x = nhwc(x)
        n, c, h, w = x.shape
        y = new_act(n, c, h // 2, w // 2, x)
        H.call("smsut_maxpool2_fwd", x, y, n, h, w, c, _s())
        ctx.save_for_backward(x)
        return y, x.view_as(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gskip):
        (x,) = ctx.saved_tensors
        n, c, h, w = x.shape
        if gy is None:
            return gskip
        gy = nhwc(gy)
        gx = new_act(n, c, h, w, x)
        if gskip is None:
            H.call("smsut_maxpool2_bwd", gy, x, gx, n, h, w, c, _s())
        else:
            H.call("smsut_maxpool2_bwd_add", gy, x, nhwc(gskip), gx, n, h, w, c, _s())
        return gx


def max_pool2_skip(x):
    """(pooled, skip) of an encoder level; plain (max_pool2(x), x) off the GPU or when no gradient is wanted."""
    if x.is_cuda and x.requires_grad and torch.is_grad_enabled():
        return MaxPool2SkipFn.apply(x)
    return max_pool2(x), x


class AvgPool2Fn(Function):
    """F.avg_pool2d(x, 2) (network/blocks.py:101,107,112); linear, closed with AvgPool2BwdFn."""

    @staticmethod
    def forward(ctx, x):
        x = nhwc(x)
        n, c, h, w = x.shape
        y = new_act(n, c, h // 2, w // 2, x)
        H.call("smsut_avgpool2_fwd", x, y, n, h, w, c, _s())
        return y

    @staticmethod
    def backward(ctx, gy):
        return AvgPool2BwdFn.apply(gy)


class AvgPool2BwdFn(Function):
    @staticmethod
    def forward(ctx, gy):
        gy = nhwc(gy)
        n, c, ho, wo = gy.shape
        gx = new_act(n, c, 2 * ho, 2 * wo, gy)
        H.call("smsut_avgpool2_bwd", gy, gx, n, 2 * ho, 2 * wo, c, _s())
        return gx

    @staticmethod
    def backward(ctx, gg):
        return AvgPool2Fn.apply(gg)


class Bilinear2Fn(Function):
    """nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False) (network/blocks.py:44)."""

    @staticmethod
    def forward(ctx, x):
        x = nhwc(x)
        n, c, h, w = x.shape
        y = new_act(n, c, 2 * h, 2 * w, x)
        H.call("smsut_bilinear2_fwd", x, y, n, h, w, c, _s())
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        gy = nhwc(gy)
        n, c, ho, wo = gy.shape
        gx = new_act(n, c, ho // 2, wo // 2, gy)
        H.call("smsut_bilinear2_bwd", gy, gx, n, ho // 2, wo // 2, c, _s())
        return gx


def max_pool2(x):
    return MaxPool2Fn.apply(x)


def avg_pool2(x):
    return AvgPool2Fn.apply(cl(x))


def bilinear_up2(x):
    return Bilinear2Fn.apply(x)


class WindowFn(Function):
    """Padding (zero / reflect / replicate) or cropping as one window copy (networks.py:95-105,618,835-851)."""
    MODES = {"zero": 0, "reflect": 1, "refl": 1, "replicate": 2, "repl": 2}

    @staticmethod
    def forward(ctx, x, top, bottom, left, right, mode):
        x = nhwc(x)
        n, c, h, w = x.shape
        hd, wd = h + top + bottom, w + left + right
        y = new_act(n, c, hd, wd, x)
        H.call("smsut_window_fwd", x, y, n, h, w, hd, wd, c, top, left, mode, _s())
        ctx.geom = (h, w, hd, wd, top, left, mode)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        gy = nhwc(gy)
        h, w, hd, wd, top, left, mode = ctx.geom
        n, c = gy.shape[0], gy.shape[1]
        gx = new_act(n, c, h, w, gy)
        H.call("smsut_window_bwd", gy, gx, n, h, w, hd, wd, c, top, left, mode, _s())
        return gx, None, None, None, None, None


def pad2d(x, pads, mode="zero"):
    """``pads`` = (left, right, top, bottom) like torch.nn.functional.pad; negative values crop."""
    left, right, top, bottom = pads
    return WindowFn.apply(cl(x), top, bottom, left, right, WindowFn.MODES[mode])


class BlurDownFn(Function):
    """networks.Downsample(C, 'reflect', filt_size=3, stride=2) (networks.py:37-60)."""

    @staticmethod
    def forward(ctx, x):
        x = nhwc(x)
        n, c, h, w = x.shape
        y = new_act(n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1, x)
        H.call("smsut_blurdown_fwd", x, y, n, h, w, c, _s())
        ctx.shape = (n, c, h, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        gy = nhwc(gy)
        n, c, h, w = ctx.shape
        gx = new_act(n, c, h, w, gy)
        H.call("smsut_blurdown_bwd", gy, gx, n, h, w, c, _s())
        return gx


def blur_down2(x):
    return BlurDownFn.apply(cl(x))


class ConcatFn(Function):
    """torch.cat([a, b], dim=1) (network/blocks.py:50) on NHWC memory."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = nhwc(a), nhwc(b)
        n, ca, h, w = a.shape
        cb = b.shape[1]
        assert b.shape[0] == n and b.shape[2:] == a.shape[2:]
        y = new_act(n, ca + cb, h, w, a)
        p = n * h * w
        if ca % 4 == 0 and cb % 4 == 0:
            H.call("smsut_concat2", a, ca, b, cb, y, p, 0, _s())
        else:
            H.call("smsut_copy_channels", a, ca, 0, y, ca + cb, 0, ca, p, _s())
            H.call("smsut_copy_channels", b, cb, 0, y, ca + cb, ca, cb, p, _s())
        ctx.split = (ca, cb)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        gy = nhwc(gy)
        ca, cb = ctx.split
        n, _, h, w = gy.shape
        p = n * h * w
        ga = new_act(n, ca, h, w, gy) if ctx.needs_input_grad[0] else None
        gb = new_act(n, cb, h, w, gy) if ctx.needs_input_grad[1] else None
        if ca % 4 == 0 and cb % 4 == 0 and (ga is not None or gb is not None):
            H.call("smsut_concat2", ga, ca, gb, cb, gy, p, 1, _s())
        else:
            if ga is not None:
                H.call("smsut_copy_channels", gy, ca + cb, 0, ga, ca, 0, ca, p, _s())
            if gb is not None:
                H.call("smsut_copy_channels", gy, ca + cb, ca, gb, cb, 0, cb, p, _s())
        return ga, gb


def concat_channels(a, b):
    y = ConcatFn.apply(a, b)
    if SPLIT_DGRAD and torch.is_grad_enabled() and (a.requires_grad or b.requires_grad) and a.shape[1] % 16 == 0:
        y._smsut_cat_parts = (a, b)        # side channel: a fused BasicBlock consuming y writes d/da, d/db itself
    return y


class RowSegmentsFn(Function):
    """(y[a0:b0], y[a1:b1], ...) along the batch dimension as views, with ONE gradient buffer assembled in the backward (rows no
    segment covers are zero; a segment without a gradient too) -- instead of autograd's zeros + copy + add per slice and a layout
    conversion behind them.  The segments must not overlap."""

    @staticmethod
    def forward(ctx, y, *bounds):
        y = nhwc(y)
        ctx.shape, ctx.bounds = tuple(y.shape), tuple(int(b) for b in bounds)
        ctx.set_materialize_grads(False)
        return tuple(y[ctx.bounds[2 * i]:ctx.bounds[2 * i + 1]] for i in range(len(bounds) // 2))

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        n, c, h, w = ctx.shape
        ref = next(g for g in gs if g is not None)
        out = new_act(n, c, h, w, ref)
        pos = 0
        segs = sorted((ctx.bounds[2 * i], ctx.bounds[2 * i + 1], gs[i]) for i in range(len(gs)))
        for a, b, g in segs:
            if a > pos:
                out[pos:a].zero_()
            if g is None:
                out[a:b].zero_()
            else:
                out[a:b].copy_(g)
            pos = b
        if pos < n:
            out[pos:].zero_()
        return (out,) + (None,) * len(ctx.bounds)


def row_segments(y, *bounds):
    return RowSegmentsFn.apply(y, *bounds)


class ModalPlanesFn(Function):
    """cat([x, m.view(B,n,1,1).repeat(1,1,H,W)], 1) (network/ugan.py:156-159)."""

    @staticmethod
    def forward(ctx, x, m):
        x = nhwc(x)
        n, cx, h, w = x.shape
        m = m.to(torch.float32).contiguous()
        nm = m.shape[1]
        y = new_act(n, cx + nm, h, w, x)
        H.call("smsut_modal_planes", x, m, y, n, h * w, cx, nm, _s())
        ctx.dims = (cx, nm)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        gy = nhwc(gy)
        cx, nm = ctx.dims
        n, _, h, w = gy.shape
        gx = None
        if ctx.needs_input_grad[0]:
            gx = new_act(n, cx, h, w, gy)
            H.call("smsut_copy_channels", gy, cx + nm, 0, gx, cx, 0, cx, n * h * w, _s())
        return gx, None


def modal_planes(x, m):
    return ModalPlanesFn.apply(x, m)


# ------------------------------------------------------------------------------------------- losses
def dice_ce_stats(logits, labels, batch_dice):
    """Stage 1 of Dice+CE: one pass over the logits -> (stats [G, C, 3] = {tp, sum_p, count}, ce_sum [1]).  No autograd:
    the differentiable stage is ``DiceCEFromStatsFn``.  Under data parallelism the caller all-reduces both tensors
    between the stages, which is also where a captured step is split (no collective inside a hipGraph)."""
    logits = nhwc(logits.detach())
    n, c, h, w = logits.shape
    labels = labels.contiguous()
    if labels.dtype != torch.int64:
        raise TypeError("labels must be int64")
    g = 1 if batch_dice else n
    stats = torch.empty(g, c, 3, dtype=torch.float32, device=logits.device)
    ce_sum = torch.empty(1, dtype=torch.float32, device=logits.device)
    H.call("smsut_dicece_stats", logits, labels, stats, ce_sum, _ws(H.call("smsut_dicece_ws", n, h * w, c, g), logits),
           n, h * w, c, g, _s())
    return stats, ce_sum


class DiceCEFromStatsFn(Function):
    """Stage 2: loss value from (already global) statistics, and the gradient w.r.t. the local logits.

    ``world`` > 1: the statistics are sums over ``world`` ranks and ``npix`` is the global pixel count, so the value is the
    single-process global-batch loss on every rank and this rank's backward is ITS SHARE of that loss' gradient.  The
    gradient all-reduce that follows AVERAGES over ranks (parallel.GradAllReducer), which is right for the per-rank
    mean losses of the step but would divide this share by ``world`` once too often -- so the backward is scaled by
    ``world`` (r01 left that out: lambda_seg was effectively 10 / world)."""

    @staticmethod
    def forward(ctx, logits, labels, stats, ce_sum, w_ce, w_dc, world):
        logits = nhwc(logits)
        n, c, h, w = logits.shape
        g = stats.shape[0]
        npix = float(n * h * w) * world
        out = torch.empty(3, dtype=torch.float32, device=logits.device)
        H.call("smsut_dicece_final", stats, ce_sum, out, g, c, npix, float(w_dc), float(w_ce), _s())
        ctx.save_for_backward(logits, labels.contiguous(), stats)
        ctx.cfg = (g, npix, float(w_dc), float(w_ce), int(world))
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        logits, labels, stats = ctx.saved_tensors
        g, npix, w_dc, w_ce, world = ctx.cfg
        n, c, h, w = logits.shape
        gl = new_act(n, c, h, w, logits)
        gout = gout.contiguous()
        if world > 1:
            gout = gout * float(world)
        H.call("smsut_dicece_bwd", logits, labels, stats, gout, gl, n, h * w, c, g, npix, w_dc, w_ce, _s())
        return gl, None, None, None, None, None, None


def dice_ce_from_stats(logits, labels, stats, ce_sum, weight_ce, weight_dc, world=1):
    return DiceCEFromStatsFn.apply(logits, labels, stats, ce_sum, weight_ce, weight_dc, world)


def all_reduce_dice_stats(pairs, group):
    """ONE all-reduce for any number of (stats, ce_sum) pairs (16 floats each at 5 classes), in place.  Tensors that already sit
    back to back in one buffer (the trainers' persistent statistics buffer; a single flat tensor) are reduced where they are --
    one collective and nothing else on the critical path between two captured phases; anything else is packed, summed, unpacked."""
    import torch.distributed as dist
    from . import graphs
    graphs.assert_no_capture("all_reduce_dice_stats (Dice-statistics all-reduce)")
    ts = [t for pair in pairs for t in pair]
    adjacent = all(t.is_contiguous() for t in ts) and all(
        a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and a.storage_offset() + a.numel() == b.storage_offset()
        for a, b in zip(ts, ts[1:]))
    if adjacent:
        span = ts[0].as_strided((sum(t.numel() for t in ts),), (1,), ts[0].storage_offset())
        dist.all_reduce(span, group=group)
        return
    flat = torch.cat([t.reshape(-1) for t in ts])
    dist.all_reduce(flat, group=group)
    off = 0
    for t in ts:
        n = t.numel()
        t.copy_(flat[off:off + n].view_as(t))
        off += n


class DiceCEFn:
    """weight_dc * SoftDice + weight_ce * CE on logits [N,C,H,W] / int64 labels [N,H,W] (misc/loss.py:8-63): the two
    stages back to back.  ``group``: optional torch.distributed process group; when given, the Dice statistics and the CE
    sum are all-reduced between the stages so the loss equals the single-process global-batch value."""

    @staticmethod
    def apply(logits, labels, w_ce, w_dc, batch_dice, group):
        stats, ce_sum = dice_ce_stats(logits, labels, batch_dice)
        world = 1
        # per-sample Dice (batch_dice False) is a mean over samples like CE: the local loss + gradient averaging IS the
        # global-batch loss, nothing to exchange
        if group is not None and batch_dice:
            import torch.distributed as dist
            world = dist.get_world_size(group)
            if world > 1:
                all_reduce_dice_stats([(stats, ce_sum)], group)
        return DiceCEFromStatsFn.apply(logits, labels, stats, ce_sum, w_ce, w_dc, world)


def dice_ce(logits, labels, weight_ce=1.0, weight_dc=1.0, batch_dice=False, group=None):
    return DiceCEFn.apply(logits, labels, weight_ce, weight_dc, batch_dice, group)


class ScaledSumFn(Function):
    """out = scale * sum(x): the WGAN terms -/+mean(out_src) (uganConsisTrainer.py:130,136,154)."""

    @staticmethod
    def forward(ctx, x, scale):
        x = x.contiguous() if x.dim() != 4 else nhwc(x)
        out = torch.empty(1, dtype=torch.float32, device=x.device)
        n = x.numel()
        H.call("smsut_sum", x, out, _ws(H.call("smsut_sum_ws", n, 1), x), n, float(scale), _s())
        ctx.meta = (x.shape, x.stride(), float(scale))
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        shape, stride, scale = ctx.meta
        gx = torch.empty_strided(shape, stride, dtype=torch.float32, device=gout.device)
        H.call("smsut_fill", gx, 1.0, gx.numel(), _s())
        out = torch.empty_strided(shape, stride, dtype=torch.float32, device=gout.device)
        H.call("smsut_scale", gx, gout.contiguous(), scale, out, gx.numel(), _s())
        return out, None


def mean_all(x, sign=1.0):
    return ScaledSumFn.apply(x, sign / x.numel())


class L1MeanFn(Function):
    """mean(|a - b|) (uganConsisTrainer.py:162)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = nhwc(a), nhwc(b)
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        n = a.numel()
        H.call("smsut_l1_fwd", a, b, out, _ws(H.call("smsut_sum_ws", n, 1), a), n, _s())
        ctx.save_for_backward(a, b)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        ga = new_act(*a.shape, a) if ctx.needs_input_grad[0] else None
        gb = new_act(*b.shape, b) if ctx.needs_input_grad[1] else None
        if ga is not None or gb is not None:
            H.call("smsut_l1_bwd", a, b, gout.contiguous(), ga, gb, a.numel(), _s())
        return ga, gb


def l1_mean(a, b):
    return L1MeanFn.apply(a, b)


class SoftmaxMSEFn(Function):
    """mean((softmax(a, 1) - softmax(b, 1)) ** 2): the mean-teacher consistency term (reference
    trainer/meanTeacherTrainer.py:113-131); ``b`` is the EMA teacher's output and gets no gradient."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = nhwc(a), nhwc(b)
        assert a.shape == b.shape
        n, c, h, w = a.shape
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        H.call("smsut_softmax_mse_fwd", a, b, out, _ws(H.call("smsut_sum_ws", n * h * w, 1), a), n * h * w, c, _s())
        ctx.save_for_backward(a, b)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        a, b = ctx.saved_tensors
        n, c, h, w = a.shape
        ga = new_act(n, c, h, w, a)
        H.call("smsut_softmax_mse_bwd", a, b, gout.contiguous().reshape(1), ga, n * h * w, c, _s())
        return ga, None


def softmax_mse(a, b):
    return SoftmaxMSEFn.apply(cl(a), cl(b).detach())


def argmax_channels(logits):
    """``torch.argmax(logits, dim=1)`` on NHWC memory -> int64 [N, H, W] (no gradient)."""
    z = nhwc(logits.detach())
    n, c, h, w = z.shape
    out = torch.empty(n, h, w, dtype=torch.int64, device=z.device)
    H.call("smsut_argmax_channels", z, out, n * h * w, c, _s())
    return out


EVAL_MAX_CLASSES, EVAL_MAX_SLICES = 32, 65535      # the limits of smsut_eval_overlap (include/smsut_hip.h)


def eval_overlap(logits, labels, vol_ids, counts, classes=None, want_pred=True):
    """Validation in one pass (csrc/evaluate.hip): the argmax of channels ``0 .. classes-1`` of every pixel (``argmax_channels``'
    rule; ``classes`` defaults to all C channels, CoraNet passes L + 1: head 0 of its 3L+1) and the Dice overlap counts of the
    batch, ADDED into ``counts``: int64 ``[V, classes, 3]`` = {|P & G|, |P|, |G|} per (volume slot, class), contiguous, on the
    logits' device; the caller zeroes it once.  ``labels``: int64 ``[N, H, W]`` on the same device; a label outside
    ``0 .. classes-1`` counts nowhere.  ``vol_ids``: N Python ints, the volume slot of each slice, or -1 for a slice to skip (no
    count, its prediction bytes left as allocated); checked HERE, on the host, and uploaded as int32 -- no device value is read
    back.  Returns the prediction as uint8 ``[N, H, W]``, or None with ``want_pred=False``.  Wrong types raise ``TypeError``,
    wrong shapes or values ``ValueError``, before the device is touched."""
    for what, t, dt in (("logits", logits, torch.float32), ("labels", labels, torch.int64), ("counts", counts, torch.int64)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"eval_overlap: {what} must be a tensor, got {type(t).__name__}")
        if t.dtype != dt:
            raise TypeError(f"eval_overlap: {what} must be {dt}, got {t.dtype}")
        if not t.is_cuda or t.device != logits.device:
            raise TypeError(f"eval_overlap: {what} must be on the logits' HIP device, got {t.device} (no CPU fallback)")
    if logits.dim() != 4:
        raise ValueError(f"eval_overlap: expected NCHW logits, got shape {tuple(logits.shape)}")
    n, c, h, w = logits.shape
    k = c if classes is None else int(classes)
    if not 1 <= k <= min(c, EVAL_MAX_CLASSES):
        raise ValueError(f"eval_overlap: classes must lie in 1..min(C, {EVAL_MAX_CLASSES}), got {k} with C = {c}")
    if tuple(labels.shape) != (n, h, w):
        raise ValueError(f"eval_overlap: labels must be [N, H, W] = {(n, h, w)}, got {tuple(labels.shape)}")
    if counts.dim() != 3 or counts.shape[0] < 1 or tuple(counts.shape[1:]) != (k, 3) or not counts.is_contiguous():
        raise ValueError(f"eval_overlap: counts must be a contiguous [V >= 1, {k}, 3] tensor, got {tuple(counts.shape)}")
    if n > EVAL_MAX_SLICES or h * w < 1:
        raise ValueError(f"eval_overlap: needs at most {EVAL_MAX_SLICES} slices of at least one pixel, got {(n, h, w)}")
    ids = [int(i) for i in vol_ids]
    if len(ids) != n:
        raise ValueError(f"eval_overlap: {len(ids)} volume ids for {n} slices")
    n_vol = counts.shape[0]
    for i in ids:
        if not -1 <= i < n_vol:
            raise ValueError(f"eval_overlap: volume id {i} is neither -1 nor a slot of counts ({n_vol} slots)")
    pred = torch.empty(n, h, w, dtype=torch.uint8, device=logits.device) if want_pred else None
    if n == 0:
        return pred
    z = nhwc(logits.detach())
    # (pinned + non_blocking: a pageable upload would make the host wait for the stream; the pinned block is recycled by torch's
    #  host allocator only after the copy has run)
    vol = torch.tensor(ids, dtype=torch.int32).pin_memory().to(z.device, non_blocking=True)
    H.call("smsut_eval_overlap", z, labels.contiguous(), vol, counts, pred, n, h * w, c, k, n_vol, _s())
    return pred


# ------------------------------------------------------------------------------------------- CoraNet heads
# The 3L+1 channels of the CoraNet U-Net are three (L+1)-class heads sharing the background logit (channel 0; head k owns channels
# 1+kL .. (k+1)L, reference trainer/coraNetTrainer.py:288-295).  These ops take the network's NHWC output as it is -- no concatenated
# head copy anywhere (csrc/coranet.hip).
def _cora_heads(logits, what):
    c = logits.shape[1]
    if c < 4 or (c - 1) % 3:
        raise ValueError(f"{what}: expected 3L+1 channels, got {c}")
    return (c - 1) // 3


def _cora_weights(w, n_cls, like):
    if w.dtype != torch.float32 or w.numel() != n_cls or w.device != like.device:
        raise ValueError(f"class weights must be {n_cls} fp32 values on {like.device}")
    return w.contiguous()


def _cora_labels(t, logits, dtype, what):
    n, _, h, w = logits.shape
    if t.dtype != dtype or tuple(t.shape) != (n, h, w):
        raise TypeError(f"{what} must be {dtype} of shape {(n, h, w)}, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def cora_sup_stats(logits, labels, w_con, w_rad):
    """Stage 1 of the supervised head loss: one pass over the logits -> flat statistics [3(L+1)+3] of the three heads (batch sums:
    all-reduced by the caller under data parallelism, like the Dice statistics).  No autograd."""
    logits = nhwc(logits.detach())
    L = _cora_heads(logits, "cora_sup_stats")
    n, c, h, w = logits.shape
    labels = _cora_labels(labels, logits, torch.int64, "labels")
    stats = torch.empty(3 * (L + 1) + 3, dtype=torch.float32, device=logits.device)
    H.call("smsut_cora_sup_stats", logits, labels, _cora_weights(w_con, L + 1, logits), _cora_weights(w_rad, L + 1, logits), stats,
           _ws(H.call("smsut_cora_ws", n, h * w, L), logits), n, h * w, L, _s())
    return stats


class CoraSupFromStatsFn(Function):
    """Stage 2: [S, dice+ce of head 0, con, rad] from (already global) statistics; element 0 is the loss and the only one that carries
    a gradient (the backward reads d/dS alone).  ``world`` as in ``DiceCEFromStatsFn``: all three terms are ratios of global sums, so
    this rank's backward is its share of the global loss and is scaled by ``world`` ahead of the averaging gradient all-reduce."""

    @staticmethod
    def forward(ctx, logits, labels, stats, w_con, w_rad, w_ce, w_dc, world):
        logits = nhwc(logits)
        L = _cora_heads(logits, "cora_sup_loss")
        n, c, h, w = logits.shape
        npix = float(n * h * w) * world
        w_con, w_rad = _cora_weights(w_con, L + 1, logits), _cora_weights(w_rad, L + 1, logits)
        out = torch.empty(4, dtype=torch.float32, device=logits.device)
        H.call("smsut_cora_sup_final", stats, w_con, w_rad, out, L, npix, float(w_dc), float(w_ce), _s())
        ctx.save_for_backward(logits, _cora_labels(labels, logits, torch.int64, "labels"), stats, w_con, w_rad)
        ctx.cfg = (L, npix, float(w_dc), float(w_ce), int(world))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        logits, labels, stats, w_con, w_rad = ctx.saved_tensors
        L, npix, w_dc, w_ce, world = ctx.cfg
        n, c, h, w = logits.shape
        gl = new_act(n, c, h, w, logits)
        gout = gout.contiguous()
        if world > 1:
            gout = gout * float(world)
        H.call("smsut_cora_sup_bwd", logits, labels, stats, w_con, w_rad, gout, gl, n, h * w, L, npix, w_dc, w_ce, _s())
        return gl, None, None, None, None, None, None, None


def cora_sup_loss(logits, labels, w_con, w_rad, weight_ce, weight_dc, group=None):
    """Supervised CoraNet loss on logits [N, 3L+1, H, W] / int64 labels [N, H, W] (reference trainer/coraNetTrainer.py:288-301):
    returns the device tensor ``[S, dice+ce of head 0, con, rad]`` with
    ``S = ([weight_dc Dice_batch(h0) + weight_ce CE(h0)] + CE_{w_con}(h1) + CE_{w_rad}(h2)) / 4``; differentiate ``[0]``.
    ``w_con`` / ``w_rad``: fp32 device tensors of L+1 class weights.  ``group``: the statistics are all-reduced between the two stages
    (one collective, ``all_reduce_dice_stats``) so the value is the single-process global-batch loss."""
    stats = cora_sup_stats(logits, labels, w_con, w_rad)
    world = 1
    if group is not None:
        import torch.distributed as dist
        world = dist.get_world_size(group)
        if world > 1:
            all_reduce_dice_stats([(stats,)], group)
    return CoraSupFromStatsFn.apply(logits, labels, stats, w_con, w_rad, weight_ce, weight_dc, world)


class CoraSemiFn(Function):
    """[certain, uncertain] of the pseudo-labelled half (reference trainer/coraNetTrainer.py:304-341); gradient to the student logits."""

    @staticmethod
    def forward(ctx, z, e, plab, mask, cw):
        z, e = nhwc(z), nhwc(e)
        if z.shape != e.shape:
            raise ValueError(f"student / teacher logits differ in shape: {tuple(z.shape)} vs {tuple(e.shape)}")
        L = _cora_heads(z, "cora_semi_loss")
        n, c, h, w = z.shape
        plab = _cora_labels(plab, z, torch.int64, "pseudo labels")
        mask = _cora_labels(mask, z, torch.float32, "mask")
        stats = torch.empty(n, 3 * (L + 1) + 4, dtype=torch.float32, device=z.device)
        H.call("smsut_cora_semi_stats", z, e, plab, mask, stats, _ws(H.call("smsut_cora_ws", n, h * w, L), z), n, h * w, L, _s())
        out = torch.empty(2, dtype=torch.float32, device=z.device)
        H.call("smsut_cora_semi_final", stats, out, n, L, float(cw), _s())
        ctx.save_for_backward(z, e, plab, mask, stats)
        ctx.cfg = (L, float(cw))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        z, e, plab, mask, stats = ctx.saved_tensors
        L, cw = ctx.cfg
        n, c, h, w = z.shape
        gz = new_act(n, c, h, w, z)
        H.call("smsut_cora_semi_bwd", z, e, plab, mask, stats, gout.contiguous(), gz, n, h * w, L, cw, _s())
        return gz, None, None, None, None


def cora_semi_loss(logits, ema_logits, plab, mask, cw):
    """Pseudo-labelled CoraNet loss: the device tensor ``[certain, uncertain]`` of student logits against pseudo labels ``plab``
    (int64 [N, H, W]), certainty mask ``mask`` (fp32 0/1 [N, H, W]) and the teacher's logits (no gradient), consistency weight ``cw``:
    ``certain = (masked CE(h0, plab) + Dice_per_sample(h0, plab)) / 2``, ``uncertain = cw / 3 * sum_k`` softmax-MSE of head k over the
    pixels where the mask is 0 (both ratios count pixels).  The ratios are per rank under data parallelism, like ``softmax_mse``."""
    return CoraSemiFn.apply(cl(logits), cl(ema_logits).detach(), plab, mask, cw)


def cora_pseudo(logits):
    """Pseudo labels and certainty mask in one pass (reference trainer/coraNetTrainer.py:189-208, there through numpy on the host):
    ``(argmax(h0) int64 [N, H, W], (argmax(h1) == argmax(h2)) fp32 [N, H, W])``, first maximum wins as ``torch.argmax``."""
    z = nhwc(logits.detach())
    L = _cora_heads(z, "cora_pseudo")
    n, c, h, w = z.shape
    q = torch.empty(n, h, w, dtype=torch.int64, device=z.device)
    m = torch.empty(n, h, w, dtype=torch.float32, device=z.device)
    H.call("smsut_cora_pseudo", z, q, m, n * h * w, L, _s())
    return q, m


# ------------------------------------------------------------------------------------------- dual-task consistency (csrc/dtc.hip)
_SDF_STATUS = {}         # device -> one int32 that smsut_edt_sq sets when it meets a label outside [0, C); read by sdf_check() only
#                          (allocated by the first call on a device: make that call eagerly, NOT inside a graph capture, or the word
#                          would live in the capture's private pool)


def _sdf_status(dev):
    st = _SDF_STATUS.get(dev)
    if st is None:
        st = _SDF_STATUS[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return st


def _sdf_labels(labels, n_classes, what):
    if labels.dtype != torch.int64 or labels.dim() != 3:
        raise TypeError(f"{what}: labels must be torch.int64 of shape [B, H, W], got {labels.dtype} {tuple(labels.shape)}")
    b, h, w = labels.shape
    n_classes = int(n_classes)
    ws = H.call("smsut_sdf_ws", b, n_classes, h, w)
    if ws < 0:
        raise ValueError(f"{what}: needs 1 <= H, W <= 512 and 1 <= n_classes <= 16, got H = {h}, W = {w}, n_classes = {n_classes}")
    return labels.contiguous(), n_classes, ws


def _edt_launch(labels, n_classes, ws):
    b, h, w = labels.shape
    d2 = torch.empty(b, n_classes, h, w, dtype=torch.int32, device=labels.device)
    work = _ws(ws, labels)
    H.call("smsut_edt_sq", labels, d2, work, _sdf_status(labels.device), b, n_classes, h, w, _s())
    return d2, work


def sdf_check(device=None):
    """Raise ``ValueError`` if an ``edt_sq`` / ``signed_distance_map`` call on ``device`` since the last check met a label outside
    ``[0, n_classes)``.  The kernels only SET a device word (such a pixel counts as a member of no class); this reads it, so it
    synchronises: call it where the host waits anyway (the trainer does after reading the iteration's scalars), never inside a capture."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    st = _SDF_STATUS.get(dev)
    if st is not None and st.item() != 0:
        st.zero_()
        raise ValueError("signed_distance_map / edt_sq: a label lies outside [0, n_classes)")


def edt_sq(labels, n_classes, validate=False):
    """Exact squared Euclidean distance transform of every class of every label slice: int64 labels ``[B, H, W]`` -> int32
    ``[B, n_classes, H, W]``.  With ``P = (labels == c)`` a member of P gets the squared distance to the nearest non-member
    (``scipy.ndimage.distance_transform_edt(P) ** 2``) and a non-member the squared distance to the nearest member
    (``distance_transform_edt(~P) ** 2``); outside the image is nothing, and the result is 0 everywhere where P is empty or full.
    Two launches on the current stream, nothing read back; ``validate=True`` adds ``sdf_check()`` (one synchronisation).  Capturable into
    a graph after one eager call on the device (the first call allocates the status word and sets a kernel attribute)."""
    labels, n_classes, ws = _sdf_labels(labels, n_classes, "edt_sq")
    d2, _ = _edt_launch(labels, n_classes, ws)
    if validate:
        sdf_check(labels.device)
    return d2


def signed_distance_map(labels, n_classes, validate=False):
    """The DTC supervision target: fp32 ``[B, n_classes, H, W]`` in channels-last memory (the layout of the tanh head), per class
    ``+sqrt(d2) / sqrt(max d2 over the non-members)`` on non-members and ``-sqrt(d2) / sqrt(max d2 over the members)`` on members with
    ``d2 = edt_sq``; exactly 0 on the inner boundary (members with ``d2 == 1``), exactly +1 everywhere where the class is absent from the
    slice and -1 where it fills it.  No autograd; three launches on the current stream, nothing read back (``validate`` as ``edt_sq``)."""
    labels, n_classes, ws = _sdf_labels(labels, n_classes, "signed_distance_map")
    b, h, w = labels.shape
    d2, work = _edt_launch(labels, n_classes, ws)
    sdf = torch.empty(b, h, w, n_classes, dtype=torch.float32, device=labels.device).permute(0, 3, 1, 2)
    H.call("smsut_sdf_final", labels, d2, work, sdf, b, n_classes, h, w, _s())
    if validate:
        sdf_check(labels.device)
    return sdf


class DtcLossFn(Function):
    """[mean((t[:B] - sdf) ** 2), mean((sigmoid(-k t) - softmax(z, 1)) ** 2)]; one backward launch writes d/dt and d/dz."""

    @staticmethod
    def forward(ctx, t, z, sdf, k):
        t, z, sdf = nhwc(t), nhwc(z), nhwc(sdf)
        if t.shape != z.shape:
            raise ValueError(f"dtc_loss: the two heads differ in shape: {tuple(t.shape)} vs {tuple(z.shape)}")
        n, c, h, w = t.shape
        b = sdf.shape[0]
        if tuple(sdf.shape[1:]) != (c, h, w) or not 1 <= b <= n or sdf.dtype != torch.float32:
            raise ValueError(f"dtc_loss: sdf must be fp32 [B <= {n}, {c}, {h}, {w}], got {sdf.dtype} {tuple(sdf.shape)}")
        out = torch.empty(2, dtype=torch.float32, device=t.device)
        H.call("smsut_dtc_loss_fwd", t, z, sdf, out, _ws(H.call("smsut_dtc_ws", n, h * w), t), n, b, h * w, c, float(k), _s())
        ctx.save_for_backward(t, z, sdf)
        ctx.k = float(k)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        t, z, sdf = ctx.saved_tensors
        n, c, h, w = t.shape
        gt, gz = new_act(n, c, h, w, t), new_act(n, c, h, w, z)
        H.call("smsut_dtc_loss_bwd", t, z, sdf, gout.contiguous(), gt, gz, n, sdf.shape[0], h * w, c, ctx.k, _s())
        return gt, gz, None, None


def dtc_loss(t, z, sdf, k=1500.0):
    """The two DTC terms as the device tensor ``[L_sdf, L_cons]``: ``t`` the tanh head and ``z`` the logits, both ``[N, C, H, W]``;
    ``sdf`` ``[B, C, H, W]`` (``signed_distance_map``; no gradient) pairs with the first ``B <= N`` slices.
    ``L_sdf = mean((t[:B] - sdf) ** 2)``, ``L_cons = mean((sigmoid(-k * t) - softmax(z, 1)) ** 2)`` over all N slices.  Both are local
    means (per rank under data parallelism, like ``softmax_mse``), bit-identical from run to run, finite for every t in [-1, 1]."""
    return DtcLossFn.apply(cl(t), cl(z), cl(sdf).detach(), k)


def _dense(t):
    """Every element of the storage span belongs to exactly one index (any dimension order)."""
    exp = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s > 1), key=lambda x: x[1]):
        if stride != exp:
            return False
        exp *= size
    return True


_EMA_TABLE = {}          # device -> (key, entries, blk_ent, blk_chunk, nblocks): the pointer table of the last parameter set


def ema_update(ema_params, params, alpha):
    """``ema = alpha * ema + (1 - alpha) * p`` over all parameter tensors in ONE launch (reference trainer/coraNetTrainer.py:168-174).
    Each pair must be fp32, dense and of one layout (the weights' HWIO strides on both sides).  The device pointer table is rebuilt
    only when a pointer changes."""
    ema_params, params = list(ema_params), [p.detach() for p in params]
    if len(ema_params) != len(params) or not params:
        raise ValueError("ema_update needs two parameter lists of equal, non-zero length")
    for e, p in zip(ema_params, params):
        if (e.dtype != torch.float32 or p.dtype != torch.float32 or e.shape != p.shape or e.device != p.device
                or any(a != b for a, b, s in zip(e.stride(), p.stride(), e.shape) if s > 1) or not _dense(e)):
            raise ValueError(f"ema_update: tensors of shape {tuple(e.shape)} / {tuple(p.shape)} differ in dtype, device or layout")
    dev = params[0].device
    key = tuple((H.ptr(e), H.ptr(p), e.numel()) for e, p in zip(ema_params, params))
    tab = _EMA_TABLE.get(dev)
    if tab is None or tab[0] != key:
        chunk = H.call("smsut_ema_chunk")
        blk_ent, blk_chunk = [], []
        for i, ent in enumerate(key):
            nb = (ent[2] + chunk - 1) // chunk
            blk_ent += [i] * nb
            blk_chunk += list(range(nb))
        tab = (key, torch.tensor(key, dtype=torch.int64, device=dev), torch.tensor(blk_ent, dtype=torch.int32, device=dev),
               torch.tensor(blk_chunk, dtype=torch.int32, device=dev), len(blk_ent))
        _EMA_TABLE[dev] = tab
    H.call("smsut_ema_multi", tab[1], tab[2], tab[3], tab[4], float(alpha), float(1 - alpha), _s())


class CERowsFn(Function):
    """F.cross_entropy(logits[B,C], target[B]) (modality classification, uganConsisTrainer.py:131,155)."""

    @staticmethod
    def forward(ctx, z, tgt):
        z = z.contiguous()
        tgt = tgt.contiguous().to(torch.int64)
        out = torch.empty(1, dtype=torch.float32, device=z.device)
        H.call("smsut_ce_rows_fwd", z, tgt, out, z.shape[0], z.shape[1], _s())
        ctx.save_for_backward(z, tgt)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        z, tgt = ctx.saved_tensors
        gz = torch.empty_like(z)
        H.call("smsut_ce_rows_bwd", z, tgt, gout.contiguous(), gz, z.shape[0], z.shape[1], _s())
        return gz, None


def cross_entropy_rows(z, tgt):
    return CERowsFn.apply(z, tgt)


class GradPenaltyFn(Function):
    """mean((||dydx_b||_2 - 1)^2) over samples (uganShp0Trainer.py:131-134)."""

    @staticmethod
    def forward(ctx, dydx):
        d = nhwc(dydx) if dydx.dim() == 4 else dydx.contiguous()
        rows = d.shape[0]
        n = d.numel() // rows
        out = torch.empty(1, dtype=torch.float32, device=d.device)
        norms = torch.empty(rows, dtype=torch.float32, device=d.device)
        H.call("smsut_gp_fwd", d, out, norms, _ws(H.call("smsut_sum_ws", n, rows), d), rows, n, _s())
        ctx.save_for_backward(d, norms)
        return out[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        d, norms = ctx.saved_tensors
        rows = d.shape[0]
        g = torch.empty_strided(d.shape, d.stride(), dtype=torch.float32, device=d.device)
        H.call("smsut_gp_bwd", d, norms, gout.contiguous(), g, rows, d.numel() // rows, _s())
        return g


def grad_penalty(dydx):
    return GradPenaltyFn.apply(dydx)


class GatherPatchesFn(Function):
    """feat.permute(0,2,3,1).flatten(1,2)[:, ids, :].flatten(0,1) (network/ugan.py:318-327)."""

    @staticmethod
    def forward(ctx, feat, ids):
        feat = nhwc(feat)
        n, c, h, w = feat.shape
        ids = ids.contiguous().to(torch.int64)
        p = ids.numel()
        out = torch.empty(n * p, c, dtype=torch.float32, device=feat.device)
        H.call("smsut_gather_rows", feat, ids, out, n, h * w, c, p, _s())
        ctx.save_for_backward(ids)
        ctx.shape = (n, c, h, w)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        (ids,) = ctx.saved_tensors
        n, c, h, w = ctx.shape
        gfeat = new_act(n, c, h, w, gout)
        H.call("smsut_scatter_rows", gout.contiguous(), ids, gfeat, n, h * w, c, ids.numel(), _s())
        return gfeat, None


def gather_patches(feat, ids):
    return GatherPatchesFn.apply(feat, ids)


class L2NormFn(Function):
    """x / (||x||_2 + 1e-7) per row (network/networks.py:234-243)."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        norms = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        H.call("smsut_l2norm_fwd", x, y, norms, x.shape[0], x.shape[1], _s())
        ctx.save_for_backward(x, norms)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, norms = ctx.saved_tensors
        gx = torch.empty_like(x)
        H.call("smsut_l2norm_bwd", gy.contiguous(), x, norms, gx, x.shape[0], x.shape[1], _s())
        return gx


def l2_normalize(x):
    return L2NormFn.apply(x)


class PatchNCEFn(Function):
    """Per-row PatchNCE loss (network/patchnce.py:13-51); ``k`` is detached as in the reference (:16)."""

    @staticmethod
    def forward(ctx, q, k, npatches, T):
        q, k = q.contiguous(), k.detach().contiguous()
        rows, dim = q.shape
        loss = torch.empty(rows, dtype=torch.float32, device=q.device)
        probs = torch.empty(rows, npatches + 1, dtype=torch.float32, device=q.device)
        H.call("smsut_patchnce_fwd", q, k, loss, probs, rows, npatches, dim, float(T), _s())
        ctx.save_for_backward(probs, k)
        ctx.cfg = (npatches, float(T))
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss):
        probs, k = ctx.saved_tensors
        npatches, T = ctx.cfg
        rows, dim = k.shape
        gq = torch.empty(rows, dim, dtype=torch.float32, device=k.device)
        H.call("smsut_patchnce_bwd", gloss.contiguous(), probs, k, gq, rows, npatches, dim, T, _s())
        return gq, None, None, None


def patch_nce(q, k, npatches, T=0.07):
    return PatchNCEFn.apply(q, k, npatches, T)


def row_lerp(a, b, alpha):
    """alpha*a + (1-alpha)*b with one alpha per sample (x_hat of WGAN-GP, uganConsisTrainer.py:138-139); no grad."""
    a, b = nhwc(a.detach()), nhwc(b.detach())
    out = new_act(*a.shape, a)
    rows = a.shape[0]
    H.call("smsut_row_lerp", a, b, alpha.detach().reshape(-1).contiguous().to(torch.float32), out, rows,
           a.numel() // rows, _s())
    return out


# ------------------------------------------------------------------------------------------- test-phase metrics
def _dhw(vol: torch.Tensor):
    """(D, H, W, planar) of a dense uint8 volume [D, H, W] or image [H, W] on the device."""
    if vol.dtype != torch.uint8 or vol.dim() not in (2, 3):
        raise ValueError(f"expected a uint8 [H, W] or [D, H, W] tensor, got {vol.dtype} {tuple(vol.shape)}")
    return (1, *vol.shape, 1) if vol.dim() == 2 else (*vol.shape, 0)


def _byte_ws(nbytes: int, like: torch.Tensor) -> torch.Tensor:
    if nbytes < 0:
        raise H.SmsutHipError("invalid metrics arguments (workspace query returned -1)")
    return torch.empty(max(int(nbytes), 4), dtype=torch.uint8, device=like.device)


def cc_filter(vol_u8, n_cls, per_slice):
    """Connected-component cleanup of classes 1..n_cls (reference misc/utils.py:18-36): components of at most a tenth of their
    class's voxels are dropped, everything else above n_cls becomes 0.  ``per_slice``: 8-neighbour labelling of each z slice
    alone; else 18-neighbour 3-D labelling.  Returns a new uint8 tensor; raises ``SmsutHipError`` if the labelling reported
    its loop bound (waits for the device to read the error word)."""
    vol = vol_u8.contiguous()
    d, h, w, _ = _dhw(vol)
    per_slice = int(bool(per_slice))
    ws = _byte_ws(H.call("smsut_cc_ws", d, h, w, int(n_cls), per_slice), vol)
    out = torch.empty_like(vol)
    H.call("smsut_cc_filter", vol, out, ws, d, h, w, int(n_cls), per_slice, _s())
    err = int(ws[:4].view(torch.int32).item())
    if err:
        raise H.SmsutHipError(f"smsut_cc_filter: union-find loop bound reached (error word {err})")
    return out


SPACING_MIN, SPACING_MAX = 1e-100, 1e100      # the range of the *_sp entry points (include/smsut_hip.h)


def check_spacing(spacing, ndim):
    """A voxel spacing for an ``ndim``-axis array as a tuple of floats, ordered like the axes.  Pure host code.  A sequence of
    another length raises ``RuntimeError`` (what scipy's ``_normalize_sequence`` raises through medpy); an entry that is not
    finite, not positive or outside [1e-100, 1e100] raises ``ValueError``."""
    try:
        sp = tuple(float(v) for v in spacing)
    except TypeError:
        raise RuntimeError("spacing must be a sequence with one entry per array axis") from None
    if len(sp) != ndim:
        raise RuntimeError("sequence argument must have length equal to input rank")
    for v in sp:
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"voxel spacing must be finite and positive, got {sp}")
        if not SPACING_MIN <= v <= SPACING_MAX:
            raise ValueError(f"voxel spacing must lie in [{SPACING_MIN:g}, {SPACING_MAX:g}], got {sp}")
    return sp


def _zyx(spacing, ndim):
    sp = check_spacing(spacing, ndim)
    return (1.0, *sp) if ndim == 2 else sp


def surface_stats(pred_u8, gt_u8, n_cls, spacing=None):
    """Per label 1..n_cls: float64 host array [n_cls, 7] = {|P&G|, |P|, |G|, border(P), sum dist(border P -> border G),
    border(G), sum dist(border G -> border P)} (medpy's dc / assd ingredients, erosion connectivity 1).  ``spacing``: None for
    distances in voxels, else one positive finite float per array axis, ``(sz, sy, sx)`` or ``(sy, sx)`` (medpy's
    ``voxelspacing``): the distances are then in the spacing's unit."""
    pred, gt = pred_u8.contiguous(), gt_u8.contiguous()
    if pred.shape != gt.shape:
        raise ValueError(f"shape mismatch {tuple(pred.shape)} vs {tuple(gt.shape)}")
    d, h, w, planar = _dhw(pred)
    _dhw(gt)
    if spacing is not None:
        sp = _zyx(spacing, pred.dim())
        ws = _byte_ws(H.call("smsut_surface_sp_ws", d, h, w, int(n_cls), planar), pred)
        out = torch.empty(int(n_cls), 7, dtype=torch.float64, device=pred.device)
        H.call("smsut_surface_stats_sp", pred, gt, out, ws, d, h, w, int(n_cls), planar, *sp, _s())
        return out.cpu().numpy()
    ws = _byte_ws(H.call("smsut_surface_ws", d, h, w, int(n_cls), planar), pred)
    out = torch.empty(int(n_cls), 7, dtype=torch.float64, device=pred.device)
    H.call("smsut_surface_stats", pred, gt, out, ws, d, h, w, int(n_cls), planar, _s())
    return out.cpu().numpy()


def surface_hd(pred_u8, gt_u8, n_cls, q=95.0, spacing=None):
    """Per label 1..n_cls: float64 host array [n_cls, 6] = {border(P), border(G), max d^2(border P -> border G),
    max d^2(border G -> border P), lo2, hi2}: the squared distances of both directions pooled (n values), lo2 the one at
    sorted rank lo = floor((n - 1) * q / 100) and hi2 the one at rank min(lo + 1, n - 1) -- medpy's hd / hd95 ingredients
    (erosion connectivity 1), selected exactly on the device.  The four distance entries are -1 when either mask is empty.
    ``spacing``: None for voxels (the four distance entries are then integers), else one positive finite float per array
    axis, ``(sz, sy, sx)`` or ``(sy, sx)``: the four distance columns are then fp64 SQUARED physical distances, each exactly
    one of the values the device computed."""
    pred, gt = pred_u8.contiguous(), gt_u8.contiguous()
    if pred.shape != gt.shape:
        raise ValueError(f"shape mismatch {tuple(pred.shape)} vs {tuple(gt.shape)}")
    d, h, w, planar = _dhw(pred)
    _dhw(gt)
    if spacing is not None:
        sp = _zyx(spacing, pred.dim())
        ws = _byte_ws(H.call("smsut_surface_hd_sp_ws", d, h, w, int(n_cls), planar), pred)
        out = torch.empty(int(n_cls), 6, dtype=torch.float64, device=pred.device)
        H.call("smsut_surface_hd_sp", pred, gt, out, ws, d, h, w, int(n_cls), planar, float(q) / 100.0, *sp, _s())
        return out.cpu().numpy()
    ws = _byte_ws(H.call("smsut_surface_hd_ws", d, h, w, int(n_cls), planar), pred)
    out = torch.empty(int(n_cls), 6, dtype=torch.float64, device=pred.device)
    H.call("smsut_surface_hd", pred, gt, out, ws, d, h, w, int(n_cls), planar, float(q) / 100.0, _s())
    return out.cpu().numpy()


SIM_MIN_SIDE, SIM_MAX_SIDE, SIM_MAX_SLICES = 11, 4096, 65535      # the limits of smsut_image_similarity (include/smsut_hip.h)


def image_similarity(a, b, data_range=1.0):
    """Per slice of two image batches: float64 device tensor ``[N, 3]`` = {sum of SSIM over the slice's (H-10)(W-10) window
    centres, SE = sum (a-b)^2 over all H W pixels, AE = sum |a-b|} (csrc/similarity.hip: 11x11 Gaussian window, sigma 1.5,
    population moments, C1 = (0.01 L)^2, C2 = (0.03 L)^2 with L = ``data_range``; fixed-order fp64 sums, bitwise reproducible).
    ``a``, ``b``: fp32 ``[N, H, W]`` or ``[N, 1, H, W]`` on the device, made contiguous here; 1 <= N <= 65535,
    11 <= H, W <= 4096.  A shape or dtype mismatch, a size outside the limits or a ``data_range`` that is not finite and positive
    raises ``ValueError`` before the device is touched.  Nothing is read back."""
    for what, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"image_similarity: {what} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise ValueError(f"image_similarity: {what} must be float32, got {t.dtype}")
    if a.shape != b.shape:
        raise ValueError(f"image_similarity: shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    if a.dim() == 4 and a.shape[1] == 1:
        n, _, h, w = a.shape
    elif a.dim() == 3:
        n, h, w = a.shape
    else:
        raise ValueError(f"image_similarity: expected [N, H, W] or [N, 1, H, W], got {tuple(a.shape)}")
    if not (1 <= n <= SIM_MAX_SLICES and SIM_MIN_SIDE <= h <= SIM_MAX_SIDE and SIM_MIN_SIDE <= w <= SIM_MAX_SIDE):
        raise ValueError(f"image_similarity: needs 1..{SIM_MAX_SLICES} slices of {SIM_MIN_SIDE}..{SIM_MAX_SIDE} pixels a side, "
                         f"got {(n, h, w)}")
    try:
        data_range = float(data_range)
    except (TypeError, ValueError):
        raise ValueError(f"image_similarity: data_range must be a number, got {data_range!r}") from None
    if not (math.isfinite(data_range) and data_range > 0.0):
        raise ValueError(f"image_similarity: data_range must be finite and positive, got {data_range}")
    if a.device != b.device:
        raise ValueError(f"image_similarity: a is on {a.device}, b on {b.device}")
    a, b = a.detach().reshape(n, h, w).contiguous(), b.detach().reshape(n, h, w).contiguous()
    H.ptr(a)                                                       # (a CPU tensor is refused here: no fallback)
    ws = _byte_ws(H.call("smsut_image_similarity_ws", n, h, w), a)
    out = torch.empty(n, 3, dtype=torch.float64, device=a.device)
    H.call("smsut_image_similarity", a, b, out, ws, n, h, w, data_range, _s())
    return out


# ------------------------------------------------------------------------------------------- volume preparation (csrc/volume.hip)
VOL_MAX_DIM, VOL_MAX_VOXELS, ORDER_MAX_RANKS = 4096, 2 ** 31 - 1, 8      # the limits of the volume entry points (include/smsut_hip.h)


def _vol_size(what, size):
    try:
        size = tuple(int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: expected three integers (z, y, x), got {size!r}") from None
    if len(size) != 3 or not all(1 <= v <= VOL_MAX_DIM for v in size) or size[0] * size[1] * size[2] > VOL_MAX_VOXELS:
        raise ValueError(f"{what}: needs three axes of 1..{VOL_MAX_DIM} and at most 2^31 - 1 voxels, got {size}")
    return size


def _vol_tensor(what, t, dtype):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: expected a tensor, got {type(t).__name__}")
    if t.dtype != dtype or t.dim() != 3:
        raise ValueError(f"{what}: expected a {dtype} [D, H, W] tensor, got {t.dtype} {tuple(t.shape)}")
    _vol_size(what, t.shape)
    return t.detach().contiguous()


def _axis_ints(what, name, v, lo):
    try:
        v = tuple(int(k) for k in v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {name} must be three integers (z, y, x), got {v!r}") from None
    if len(v) != 3 or not all(lo <= k <= VOL_MAX_DIM for k in v):
        raise ValueError(f"{what}: {name} must be three integers in {lo}..{VOL_MAX_DIM}, got {v}")
    return v


def _resample_args(what, out_size, num, den, start, offset):
    return (_vol_size(what + " out_size", out_size), _axis_ints(what, "num", num, 1), _axis_ints(what, "den", den, 1),
            _axis_ints(what, "start", start, 0), _axis_ints(what, "offset", offset, 0))


def bspline_coefficients(vol):
    """The cubic B-spline interpolation coefficients of ``vol`` (fp32 ``[D, H, W]`` on the device) with whole-sample mirror
    boundaries on every axis (index -1 -> 1, n -> n - 2; an axis of length 1 is copied): ITK's BSplineDecompositionImageFilter,
    scipy's ``spline_filter(order=3, mode='mirror')``.  A new fp32 tensor of the same shape; nothing is read back."""
    vol = _vol_tensor("bspline_coefficients", vol, torch.float32)
    H.ptr(vol)
    d, h, w = vol.shape
    ws = _byte_ws(H.call("smsut_bspline_ws", d, h, w), vol)
    out = torch.empty_like(vol)
    H.call("smsut_bspline_coefficients", vol, out, ws, d, h, w, _s())
    return out


def resample_volume(coeff, out_size, num, den, start, offset=(0, 0, 0)):
    """Evaluate the cubic B-spline with coefficients ``coeff`` (fp32 ``[D, H, W]``, from ``bspline_coefficients``) on the window
    ``out_size = (oz, oy, ox)``: output index i of an axis reads the continuous index ``x = ((i + start) * num) / den - offset``
    (fp64), and a point with ``x < -0.5`` or ``x >= n - 0.5`` on any axis is 0.  ``num``, ``den``, ``start``, ``offset``: three
    integers each, ordered (z, y, x).  Only the window is written; returns fp32 ``[oz, oy, ox]``."""
    coeff = _vol_tensor("resample_volume", coeff, torch.float32)
    out_size, num, den, start, offset = _resample_args("resample_volume", out_size, num, den, start, offset)
    H.ptr(coeff)
    ws = _byte_ws(H.call("smsut_resample_ws", *out_size), coeff)
    out = torch.empty(out_size, dtype=torch.float32, device=coeff.device)
    H.call("smsut_resample_volume", coeff, out, ws, *coeff.shape, *out_size, *num, *den, *start, *offset, _s())
    return out


def resample_labels(lab_u8, out_size, num, den, start, offset=(0, 0, 0), lut=None):
    """Nearest-neighbour resampling of a uint8 label volume ``[D, H, W]`` by ``resample_volume``'s index map: source index
    ``floor(x + 0.5)`` (halves round up), 0 outside.  ``lut``: an optional 256-entry uint8 device tensor applied to the SOURCE value
    (a grey-range -> class remap in the same pass).  Returns uint8 ``[oz, oy, ox]``."""
    lab = _vol_tensor("resample_labels", lab_u8, torch.uint8)
    out_size, num, den, start, offset = _resample_args("resample_labels", out_size, num, den, start, offset)
    if lut is not None:
        if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or lut.numel() != 256:
            raise ValueError("resample_labels: lut must be a uint8 tensor of 256 entries")
        if lut.device != lab.device:
            raise ValueError(f"resample_labels: lab is on {lab.device}, lut on {lut.device}")
        lut = lut.contiguous()
    H.ptr(lab)
    ws = _byte_ws(H.call("smsut_resample_ws", *out_size), lab)
    out = torch.empty(out_size, dtype=torch.uint8, device=lab.device)
    H.call("smsut_resample_labels", lab, out, ws, lut, *lab.shape, *out_size, *num, *den, *start, *offset, _s())
    return out


def order_statistics(vol, ranks):
    """The values ``np.partition`` would leave at the sorted positions ``ranks`` (1..8 integers in ``[0, n)``) of the ``n`` values of
    the fp32 device tensor ``vol`` (any shape): an fp32 device tensor ``[len(ranks)]``, exact (an MSD radix select over
    order-preserving integer keys; -0.0 and +0.0 compare equal as floats).  Every value must be FINITE: NaN and Inf are outside the
    contract.  Nothing is read back."""
    if not isinstance(vol, torch.Tensor) or vol.dtype != torch.float32:
        raise ValueError("order_statistics: expected a float32 tensor")
    n = vol.numel()
    try:
        ranks = [int(r) for r in ranks]
    except (TypeError, ValueError):
        raise ValueError(f"order_statistics: ranks must be integers, got {ranks!r}") from None
    if not 1 <= n <= VOL_MAX_VOXELS:
        raise ValueError(f"order_statistics: needs 1..2^31 - 1 values, got {n}")
    if not 1 <= len(ranks) <= ORDER_MAX_RANKS or not all(0 <= r < n for r in ranks):
        raise ValueError(f"order_statistics: needs 1..{ORDER_MAX_RANKS} ranks in [0, {n}), got {ranks}")
    v = vol.detach().contiguous()
    H.ptr(v)
    ws = _byte_ws(H.call("smsut_order_statistics_ws", n, len(ranks)), v)
    out = torch.empty(len(ranks), dtype=torch.float32, device=v.device)
    H.call("smsut_order_statistics", v, out, ws, n, len(ranks), *(ranks + [0] * (ORDER_MAX_RANKS - len(ranks))), _s())
    return out


def window_u8(vol, bounds):
    """``(uint8)((min(max(x, lo), hi) - lo) / (hi - lo) * 255.0f)`` of every value of the fp32 device tensor ``vol``, with
    ``(lo, hi) = bounds``, a 2-float device tensor read on the device: fp32 in this order, IEEE division, truncation; all zeros when
    ``hi == lo``.  Returns a uint8 tensor of ``vol``'s shape."""
    if not isinstance(vol, torch.Tensor) or vol.dtype != torch.float32:
        raise ValueError("window_u8: expected a float32 tensor")
    if not isinstance(bounds, torch.Tensor) or bounds.dtype != torch.float32 or bounds.numel() != 2:
        raise ValueError("window_u8: bounds must be a float32 tensor (lo, hi)")
    if not 1 <= vol.numel() <= VOL_MAX_VOXELS:
        raise ValueError(f"window_u8: needs 1..2^31 - 1 values, got {vol.numel()}")
    if bounds.device != vol.device:
        raise ValueError(f"window_u8: vol is on {vol.device}, bounds on {bounds.device}")
    v, b = vol.detach().contiguous(), bounds.detach().contiguous()
    H.ptr(v)
    out = torch.empty(v.shape, dtype=torch.uint8, device=v.device)
    H.call("smsut_window_u8", v, b, out, v.numel(), _s())
    return out


# ------------------------------------------------------------------------------------------- test-time augmentation (csrc/tta.hip)
# Transform g = r + 4 f (r in 0..3 quarter turns, f in 0..1) acts on the last two axes of a slice:
#   F_g(x) = torch.rot90(torch.flip(x, [-1]) if f else x, k=r, dims=(-2, -1)),   F_g^-1(y) = flip_if_f(torch.rot90(y, k=-r, dims=(-2, -1)))
# Odd r needs H == W.  The kernels, tests/tta_ref.py and predict.py all use this one definition.
TTA_MAX_MEMBERS, TTA_MAX_CLASSES, TTA_MAX_SLICES, TTA_MAX_DIM = 16, 32, 65535, 16384     # the limits of smsut_tta_* (include/smsut_hip.h)
TTA_SETS = {"none": (0,), "flips": (0, 4, 6, 2), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}          # flips: identity, left-right, up-down, both


def tta_transforms(name_or_list):
    """A named transform set (``'none'``, ``'flips'``, ``'d4'``) or a sequence of integers ``g = r + 4 f`` in 0..7 (repeats allowed:
    one entry per ensemble member) as a tuple of ints.  Pure host code; ``ValueError`` for an unknown name, an empty or over-long
    list or an entry outside 0..7, ``TypeError`` for anything that is neither a name nor a sequence of integers."""
    if isinstance(name_or_list, str):
        if name_or_list not in TTA_SETS:
            raise ValueError(f"tta_transforms: unknown set {name_or_list!r}; expected one of {sorted(TTA_SETS)}")
        return TTA_SETS[name_or_list]
    try:
        items = list(name_or_list)
    except TypeError:
        raise TypeError(f"tta_transforms: expected a set name or a sequence of integers, got {type(name_or_list).__name__}") from None
    for g in items:
        if isinstance(g, bool) or not isinstance(g, int):
            raise TypeError(f"tta_transforms: entries must be integers, got {g!r}")
    if not 1 <= len(items) <= TTA_MAX_MEMBERS:
        raise ValueError(f"tta_transforms: needs 1..{TTA_MAX_MEMBERS} transforms, got {len(items)}")
    if not all(0 <= g <= 7 for g in items):
        raise ValueError(f"tta_transforms: entries must lie in 0..7 (g = r + 4 f), got {items}")
    return tuple(items)


def _tta_check_plane(what, transforms, h, w):
    if not (1 <= h <= TTA_MAX_DIM and 1 <= w <= TTA_MAX_DIM):
        raise ValueError(f"{what}: H and W must lie in 1..{TTA_MAX_DIM}, got {(h, w)}")
    if h != w and any(g & 1 for g in transforms):
        raise ValueError(f"{what}: a quarter turn (odd r, transforms {[g for g in transforms if g & 1]}) needs a square slice, got {h} x {w}")


def _tta_host_ints(values):
    import ctypes
    arr = (ctypes.c_int * len(values))(*values)
    return arr, ctypes.addressof(arr)


def tta_expand(img_u8, transforms):
    """The augmented network inputs of a group of slices in one launch: ``img_u8`` uint8 ``[N, H, W]`` on the device ->
    fp32 ``[T, N, 1, H, W]``; member ``t`` is ``F_g`` of every slice for ``g = transforms[t]``, converted exactly as the loader
    converts a PNG slice on the device (bitwise ``u8.float().div(255).sub(.5).div(.5)`` of a device tensor).  ``TypeError`` for wrong types or devices, ``ValueError`` for
    shapes, values or a quarter turn of a non-square slice, before the device is touched.  No CPU fallback."""
    tr = tta_transforms(transforms)
    if not isinstance(img_u8, torch.Tensor):
        raise TypeError(f"tta_expand: img_u8 must be a tensor, got {type(img_u8).__name__}")
    if img_u8.dtype != torch.uint8:
        raise TypeError(f"tta_expand: img_u8 must be uint8, got {img_u8.dtype}")
    if not img_u8.is_cuda:
        raise TypeError(f"tta_expand: img_u8 must be on a HIP device, got {img_u8.device} (no CPU fallback)")
    if img_u8.dim() != 3:
        raise ValueError(f"tta_expand: expected [N, H, W] slices, got shape {tuple(img_u8.shape)}")
    n, h, w = img_u8.shape
    _tta_check_plane("tta_expand", tr, h, w)
    if n > TTA_MAX_SLICES:
        raise ValueError(f"tta_expand: at most {TTA_MAX_SLICES} slices, got {n}")
    out = torch.empty(len(tr), n, 1, h, w, dtype=torch.float32, device=img_u8.device)
    if n == 0:
        return out
    keep, addr = _tta_host_ints(tr)
    H.call("smsut_tta_expand", img_u8.contiguous(), out, addr, len(tr), n, h, w, _s())
    del keep                                                   # (the entry point has copied the list into the kernel arguments)
    return out


def _tta_members(what, members, transforms, classes):
    """The checks ``tta_merge`` and ``tta_uncertainty`` share, all on the host: ``(members as a list, transforms, n, c, h, w, k)``."""
    tr = tta_transforms(transforms)
    try:
        members = list(members)
    except TypeError:
        raise TypeError(f"{what}: members must be a sequence of tensors, got {type(members).__name__}") from None
    for i, m in enumerate(members):
        if not isinstance(m, torch.Tensor):
            raise TypeError(f"{what}: member {i} must be a tensor, got {type(m).__name__}")
        if m.dtype != torch.float32:
            raise TypeError(f"{what}: member {i} must be float32, got {m.dtype}")
    if not 1 <= len(members) <= TTA_MAX_MEMBERS:
        raise ValueError(f"{what}: needs 1..{TTA_MAX_MEMBERS} members, got {len(members)}")
    for i, m in enumerate(members):
        if not m.is_cuda or m.device != members[0].device:
            raise TypeError(f"{what}: member {i} must be on the first member's HIP device, got {m.device} (no CPU fallback)")
    if len(tr) != len(members):
        raise ValueError(f"{what}: {len(members)} members but {len(tr)} transforms")
    if members[0].dim() != 4:
        raise ValueError(f"{what}: expected NCHW logits, got shape {tuple(members[0].shape)}")
    n, c, h, w = members[0].shape
    for i, m in enumerate(members):
        if tuple(m.shape) != (n, c, h, w):
            raise ValueError(f"{what}: member {i} has shape {tuple(m.shape)}, member 0 {(n, c, h, w)}")
    k = c if classes is None else int(classes)
    if not 1 <= k <= min(c, TTA_MAX_CLASSES):
        raise ValueError(f"{what}: classes must lie in 1..min(C, {TTA_MAX_CLASSES}), got {k} with C = {c}")
    _tta_check_plane(what, tr, h, w)
    if n > TTA_MAX_SLICES:
        raise ValueError(f"{what}: at most {TTA_MAX_SLICES} slices, got {n}")
    return members, tr, n, c, h, w, k


def tta_merge(members, transforms, classes=None, want_conf=False, want_prob=False):
    """Test-time augmentation / ensembling in one pass (csrc/tta.hip).  ``members``: T logit tensors, logical NCHW ``[N, C, H, W]``
    fp32 in the NHWC memory the networks leave them in (read in place, each logit once; they are not stacked), member ``t`` being
    a network's output on ``tta_expand(...)[t]``; ``transforms``: their T transforms (a set name or integers, repeats allowed:
    two networks x four flips is T = 8).  The softmax of channels ``0 .. classes-1`` of every member (``classes`` defaults to C;
    CoraNet passes L + 1: head 0) is averaged on the un-transformed grid.  Returns ``(pred, conf, prob)``: ``pred`` uint8
    ``[N, H, W]``, the first maximum of the mean by ``argmax_channels``' rule; ``conf`` fp32 ``[N, H, W]``, the mean probability
    of that class, or None; ``prob`` fp32 ``[N, H, W, classes]`` or None.  Bitwise reproducible.  ``TypeError`` for wrong types
    or devices, ``ValueError`` for shapes, values or a quarter turn of a non-square slice, before the device is touched."""
    import ctypes
    members, tr, n, c, h, w, k = _tta_members("tta_merge", members, transforms, classes)
    dev = members[0].device
    pred = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
    conf = torch.empty(n, h, w, dtype=torch.float32, device=dev) if want_conf else None
    prob = torch.empty(n, h, w, k, dtype=torch.float32, device=dev) if want_prob else None
    if n == 0:
        return pred, conf, prob
    zs = [nhwc(m.detach()) for m in members]                  # (a network's output already is NHWC: no copy)
    ptrs = (ctypes.c_void_p * len(zs))(*[z.data_ptr() for z in zs])
    keep, addr = _tta_host_ints(tr)
    H.call("smsut_tta_merge", ctypes.addressof(ptrs), addr, pred, conf, prob, len(zs), n, h, w, c, k, _s())
    del keep, ptrs
    return pred, conf, prob


# ------------------------------------------------------------------------------------------- sliding windows (csrc/window.hip)
WINDOW_MAX_TILES = 64                                          # smsut_window_blend: ny * nx <= 64 (include/smsut_hip.h)
WINDOW_BLENDS = ("gaussian", "constant")


def window_plan(size, window, overlap=0.5):
    """The origins of the windows of length ``window`` along an axis of length ``size``, as a tuple of ints: ``target = max(1,
    int(window * (1 - overlap)))`` is the largest step, ``n = ceil((size - window) / target) + 1`` windows, origin ``i`` at
    ``(i * (size - window)) // (n - 1)`` (``(0,)`` for ``n == 1``).  The first origin is 0, the last ``size - window``, they increase
    strictly and consecutive ones are at most ``target <= window`` apart: every index is covered.  Pure host code, integer
    arithmetic; ``ValueError`` unless ``1 <= window <= size`` and ``0 <= overlap < 1``."""
    for name, v in (("size", size), ("window", window)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise TypeError(f"window_plan: {name} must be an integer, got {v!r}")
    if isinstance(overlap, bool) or not isinstance(overlap, numbers.Real):
        raise TypeError(f"window_plan: overlap must be a number, got {overlap!r}")
    size, window = int(size), int(window)
    if not 1 <= window <= size:
        raise ValueError(f"window_plan: needs 1 <= window <= size, got window {window}, size {size}")
    if not 0 <= overlap < 1:
        raise ValueError(f"window_plan: needs 0 <= overlap < 1, got {overlap}")
    target = max(1, int(window * (1 - overlap)))
    span = size - window
    n = (span + target - 1) // target + 1
    return (0,) if n == 1 else tuple((i * span) // (n - 1) for i in range(n))


def window_weights(n, blend="gaussian", device=None):
    """One axis of the separable importance map of a window of length ``n``, fp32 ``[n]`` on ``device``.  ``'gaussian'``:
    ``exp(-0.5 * ((i - (n - 1) / 2) / (n / 8))**2)``, sigma = n / 8 (the nnU-Net and MONAI default), computed in fp64 on the host
    and rounded once; ``'constant'``: ones.  Every value is finite and positive (at n = 256 the smallest is 3.6e-4, the corner
    product 1.3e-7: a normal fp32 number)."""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral):
        raise TypeError(f"window_weights: n must be an integer, got {n!r}")
    if not 1 <= n <= TTA_MAX_DIM:
        raise ValueError(f"window_weights: n must lie in 1..{TTA_MAX_DIM}, got {n}")
    if blend not in WINDOW_BLENDS:
        raise ValueError(f"window_weights: unknown blend {blend!r}; expected one of {list(WINDOW_BLENDS)}")
    n = int(n)
    if blend == "constant":
        w = [1.0] * n
    else:
        w = [math.exp(-0.5 * ((i - (n - 1) / 2) / (n / 8)) ** 2) for i in range(n)]
    return torch.tensor(w, dtype=torch.float64).to(torch.float32).to(device)


def _window_origins(what, name, origins, window, size):
    """One axis of a plan: integers, strictly increasing, every window inside ``[0, size)`` and every index under one."""
    try:
        origins = list(origins)
    except TypeError:
        raise TypeError(f"{what}: {name} must be a sequence of integers, got {type(origins).__name__}") from None
    for o in origins:
        if isinstance(o, bool) or not isinstance(o, numbers.Integral):
            raise TypeError(f"{what}: {name} must be integers, got {o!r}")
    origins = [int(o) for o in origins]
    if not origins:
        raise ValueError(f"{what}: {name} is empty")
    if any(b <= a for a, b in zip(origins, origins[1:])):
        raise ValueError(f"{what}: {name} must increase strictly, got {origins}")
    if origins[0] < 0 or origins[-1] + window > size:
        raise ValueError(f"{what}: a window of {window} at {name} {origins} leaves the grid's axis of {size}")
    if origins[0] > 0 or origins[-1] + window < size or any(b > a + window for a, b in zip(origins, origins[1:])):
        raise ValueError(f"{what}: windows of {window} at {name} {origins} leave an index of the axis of {size} uncovered")
    return origins


def window_blend(tiles, ys, xs, grid_hw, wy, wx, want_conf=False, want_prob=False):
    """Blend the windows of a sliding-window prediction in one pass (csrc/window.hip).  ``tiles``: ``len(ys) * len(xs)`` tensors in
    row-major (iy, ix) order, each the mean class probabilities of one window as contiguous fp32 ``[N, wh, ww, K]`` (what
    ``tta_merge(..., want_prob=True)`` returns; read in place, they are not stacked), window (iy, ix) lying at ``ys[iy], xs[ix]`` of
    the grid ``grid_hw = (H, W)``; ``wy [wh]``, ``wx [ww]``: the two axes of the importance map on the device
    (``window_weights``).  Per pixel the covering windows' weights ``wy * wx`` are normalised by their sum and the probabilities
    averaged with them, in row-major window order, in fp32.  Returns ``(pred, conf, prob)``: ``pred`` uint8 ``[N, H, W]``, the
    first maximum by ``argmax_channels``' rule; ``conf`` fp32 ``[N, H, W]``, the blended probability of that class, or None;
    ``prob`` fp32 ``[N, H, W, K]`` or None.  Under one window a pixel's probabilities pass through bit for bit.  Bitwise
    reproducible.  All checks run on the host before the device is touched: ``TypeError`` for what is no fp32 tensor or is on the CPU,
    ``ValueError`` for a tile that is not contiguous ``[N, wh, ww, K]`` (it is not copied silently), a tile count other than
    ``len(ys) * len(xs)`` or above 64, origins that do not increase strictly, leave the grid or leave an index uncovered, and
    weight tables of another length or device."""
    import ctypes
    what = "window_blend"
    try:
        tiles = list(tiles)
    except TypeError:
        raise TypeError(f"{what}: tiles must be a sequence of tensors, got {type(tiles).__name__}") from None
    for name, t in [(f"tile {i}", t) for i, t in enumerate(tiles)] + [("wy", wy), ("wx", wx)]:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")
    if not tiles:
        raise ValueError(f"{what}: needs at least one tile")
    if tiles[0].dim() != 4:
        raise ValueError(f"{what}: expected tiles [N, wh, ww, K], got shape {tuple(tiles[0].shape)}")
    n, wh, ww, k = tiles[0].shape
    try:
        h, w = (int(v) for v in grid_hw)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: grid_hw must be two integers (H, W), got {grid_hw!r}") from None
    if not (1 <= wh <= h <= TTA_MAX_DIM and 1 <= ww <= w <= TTA_MAX_DIM):
        raise ValueError(f"{what}: needs 1 <= window <= grid <= {TTA_MAX_DIM} on both axes, got window {(wh, ww)}, grid {(h, w)}")
    ys = _window_origins(what, "ys", ys, wh, h)
    xs = _window_origins(what, "xs", xs, ww, w)
    if len(tiles) != len(ys) * len(xs):
        raise ValueError(f"{what}: {len(tiles)} tiles for {len(ys)} x {len(xs)} origins")
    if len(tiles) > WINDOW_MAX_TILES:
        raise ValueError(f"{what}: at most {WINDOW_MAX_TILES} tiles, got {len(tiles)}")
    if not 1 <= k <= TTA_MAX_CLASSES:
        raise ValueError(f"{what}: classes must lie in 1..{TTA_MAX_CLASSES}, got {k}")
    if n > TTA_MAX_SLICES:
        raise ValueError(f"{what}: at most {TTA_MAX_SLICES} slices, got {n}")
    for i, t in enumerate(tiles):
        if tuple(t.shape) != (n, wh, ww, k):
            raise ValueError(f"{what}: tile {i} has shape {tuple(t.shape)}, tile 0 {(n, wh, ww, k)}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: tile {i} is not contiguous [N, wh, ww, K] (strides {t.stride()}); it is not copied silently")
    for name, t, length in (("wy", wy, wh), ("wx", wx, ww)):
        if tuple(t.shape) != (length,) or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous [{length}] table, got shape {tuple(t.shape)}")
    for i, t in enumerate(tiles):
        if not t.is_cuda or t.device != tiles[0].device:
            raise TypeError(f"{what}: tile {i} must be on the first tile's HIP device, got {t.device} (no CPU fallback)")
    dev = tiles[0].device
    for name, t in (("wy", wy), ("wx", wx)):
        if t.device != dev:
            raise ValueError(f"{what}: the tiles are on {dev}, {name} on {t.device}")
    pred = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
    conf = torch.empty(n, h, w, dtype=torch.float32, device=dev) if want_conf else None
    prob = torch.empty(n, h, w, k, dtype=torch.float32, device=dev) if want_prob else None
    if n == 0:
        return pred, conf, prob
    zs = [t.detach() for t in tiles]
    ptrs = (ctypes.c_void_p * len(zs))(*[z.data_ptr() for z in zs])
    keep_y, addr_y = _tta_host_ints(ys)
    keep_x, addr_x = _tta_host_ints(xs)
    H.call("smsut_window_blend", ctypes.addressof(ptrs), addr_y, addr_x, wy.detach(), wx.detach(), pred, conf, prob, len(ys), len(xs),
           n, h, w, wh, ww, k, _s())
    del keep_y, keep_x, ptrs                                   # (the entry point has copied the tables into the kernel arguments)
    return pred, conf, prob


# ------------------------------------------------------------------------------------------- uncertainty (csrc/uncertainty.hip)
UNCERTAIN_ENTROPY_SCALE = 1 << 20                              # HSUM counts entropy in units of 2^-20 nat (csrc/uncertainty.hip)


class UncertaintyLayout:
    """Where ``tta_uncertainty`` keeps what in a row of its int64 ``counts [classes, 2 T + 4]`` (include/smsut_hip.h): columns
    ``V`` (pixels predicted k), ``ALL`` (every member chose k), ``ANY`` (some member chose k), ``HSUM`` (the entropy of the pixels
    predicted k, summed in units of 2^-20 nat); ``member_voxels`` (``V_t``: member t chose k) and ``member_overlap`` (``I_t``:
    member t chose k and so did the prediction) are ``[classes, T]`` views of an array or tensor.  Pure host code."""
    V, ALL, ANY, HSUM, FIXED = 0, 1, 2, 3, 4

    def __init__(self, members):
        if isinstance(members, bool) or not isinstance(members, int):
            raise TypeError(f"UncertaintyLayout: members must be an int, got {type(members).__name__}")
        if not 1 <= members <= TTA_MAX_MEMBERS:
            raise ValueError(f"UncertaintyLayout: members must lie in 1..{TTA_MAX_MEMBERS}, got {members}")
        self.members = members
        self.slots = 2 * members + self.FIXED

    def member_voxels(self, counts):
        return counts[:, self.FIXED:self.FIXED + self.members]

    def member_overlap(self, counts):
        return counts[:, self.FIXED + self.members:self.slots]


class Uncertainty(NamedTuple):
    pred: torch.Tensor                         # uint8 [N, H, W]: tta_merge's prediction, bit for bit
    conf: torch.Tensor                         # fp32 [N, H, W]: tta_merge's confidence, bit for bit
    entropy: Optional[torch.Tensor]            # fp32 [N, H, W]: the entropy of the mean probabilities (nat)
    mutual_info: Optional[torch.Tensor]        # fp32 [N, H, W]: that entropy minus the members' mean entropy, clamped at 0
    votes: Optional[torch.Tensor]              # uint8 [N, H, W]: the members whose own label is the prediction


def tta_uncertainty(members, transforms, classes=None, counts=None, want_maps=True):
    """``tta_merge``'s pass with the uncertainty of its prediction (csrc/uncertainty.hip): the same members, transforms and
    ``classes``, read the same way, once.  Returns ``Uncertainty(pred, conf, entropy, mutual_info, votes)``: ``pred`` / ``conf`` are
    bitwise ``tta_merge``'s; ``entropy`` is H = -sum_k mean_k log(mean_k + 1e-6) of the averaged probabilities; ``mutual_info`` is
    H minus the mean of the members' own entropies (BALD: large where the members contradict each other, not where all are unsure),
    clamped at 0; ``votes`` counts the members whose own label -- the first maximum of their logits -- is ``pred``.  With
    ``want_maps=False`` these three are None.  ``counts``: an int64 contiguous ``[classes, 2 T + 4]`` tensor on the members' device
    that the call ADDS the per-class agreement counts into (``UncertaintyLayout``; ``misc.utils.structure_agreement`` turns them
    into scores); the caller zeroes it once per volume.  Integers and per-pixel arithmetic only: bitwise reproducible.
    ``TypeError`` for wrong types or devices, ``ValueError`` for shapes and values, before the device is touched."""
    import ctypes
    if counts is not None:
        if not isinstance(counts, torch.Tensor):
            raise TypeError(f"tta_uncertainty: counts must be a tensor, got {type(counts).__name__}")
        if counts.dtype != torch.int64:
            raise TypeError(f"tta_uncertainty: counts must be int64, got {counts.dtype}")
    members, tr, n, c, h, w, k = _tta_members("tta_uncertainty", members, transforms, classes)
    dev = members[0].device
    if counts is not None:
        if counts.device != dev:
            raise TypeError(f"tta_uncertainty: counts must be on the members' device {dev}, got {counts.device}")
        slots = UncertaintyLayout(len(tr)).slots
        if tuple(counts.shape) != (k, slots) or not counts.is_contiguous():
            raise ValueError(f"tta_uncertainty: counts must be a contiguous [{k}, {slots}] tensor ([classes, 2 T + 4]), got shape "
                             f"{tuple(counts.shape)}, strides {tuple(counts.stride())}")
    pred = torch.empty(n, h, w, dtype=torch.uint8, device=dev)
    conf = torch.empty(n, h, w, dtype=torch.float32, device=dev)
    entropy = torch.empty(n, h, w, dtype=torch.float32, device=dev) if want_maps else None
    mutual = torch.empty(n, h, w, dtype=torch.float32, device=dev) if want_maps else None
    votes = torch.empty(n, h, w, dtype=torch.uint8, device=dev) if want_maps else None
    if n == 0:
        return Uncertainty(pred, conf, entropy, mutual, votes)
    zs = [nhwc(m.detach()) for m in members]                  # (a network's output already is NHWC: no copy)
    ptrs = (ctypes.c_void_p * len(zs))(*[z.data_ptr() for z in zs])
    keep, addr = _tta_host_ints(tr)
    H.call("smsut_tta_uncertain", ctypes.addressof(ptrs), addr, pred, conf, entropy, mutual, votes, counts, len(zs), n, h, w, c, k,
           _s())
    del keep, ptrs
    return Uncertainty(pred, conf, entropy, mutual, votes)


# ------------------------------------------------------------------------------------------- calibration (test phase)
CALIB_MAX_CLASSES, CALIB_MAX_BINS, CALIB_MAX_SLICES, CALIB_MAX_DIM = 32, 64, 65535, 16384   # include/smsut_hip.h: SMSUT_CALIB_*


class CalibrationLayout:
    """Where ``calibration_stats`` keeps what in its fp64 vector of ``size = 3 bins + 4 classes + 4`` (include/smsut_hip.h).
    Each accessor takes such a vector -- a NumPy array or a tensor, anything that slices -- and returns a view:
    ``bins`` ``[bins, 3]`` = {pixels, sum of conf, correct pixels}; ``classes`` ``[classes, 4]`` = {pixels, correct pixels, sum of
    nll, sum of brier} per true class; ``grad``, ``curv`` (the first and second derivative of the summed NLL by 1 / temperature),
    ``skipped`` and ``nonfinite``: the element itself.  Pure host code."""

    def __init__(self, classes, bins):
        self.n_classes, self.n_bins = int(classes), int(bins)
        if not 1 <= self.n_classes <= CALIB_MAX_CLASSES:
            raise ValueError(f"CalibrationLayout: classes must lie in 1..{CALIB_MAX_CLASSES}, got {classes}")
        if not 1 <= self.n_bins <= CALIB_MAX_BINS:
            raise ValueError(f"CalibrationLayout: bins must lie in 1..{CALIB_MAX_BINS}, got {bins}")
        self.size = 3 * self.n_bins + 4 * self.n_classes + 4
        self._tail = 3 * self.n_bins + 4 * self.n_classes

    def bins(self, v):
        return v[:3 * self.n_bins].reshape(self.n_bins, 3)

    def classes(self, v):
        return v[3 * self.n_bins:self._tail].reshape(self.n_classes, 4)

    def grad(self, v):
        return v[self._tail]

    def curv(self, v):
        return v[self._tail + 1]

    def skipped(self, v):
        return v[self._tail + 2]

    def nonfinite(self, v):
        return v[self._tail + 3]


def calibration_stats(logits, labels, out, classes=None, bins=15, temperature=1.0):
    """Calibration statistics of one batch in one pass (csrc/calibration.hip), ADDED into ``out``: fp64, contiguous,
    ``CalibrationLayout(classes, bins).size`` elements on the logits' device; the caller zeroes it once.  ``logits``: logical NCHW
    fp32 in the NHWC memory a network leaves it in (read in place, no copy); ``labels``: int64 ``[N, H, W]``; ``classes``: the
    leading channels that are classes (default: all; CoraNet passes L + 1); the softmax is taken of ``logits / temperature``
    (the kernel multiplies by the fp32 value of ``1 / temperature``).  A label outside ``0 .. classes-1`` counts in ``skipped``
    only.  Two launches, nothing is read back; bitwise reproducible.  Returns ``out``.  Wrong types raise ``TypeError``, wrong
    shapes or values ``ValueError``, before the device is touched.  No CPU fallback."""
    for what, t, dt in (("logits", logits, torch.float32), ("labels", labels, torch.int64), ("out", out, torch.float64)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"calibration_stats: {what} must be a tensor, got {type(t).__name__}")
        if t.dtype != dt:
            raise TypeError(f"calibration_stats: {what} must be {dt}, got {t.dtype}")
        if not t.is_cuda or t.device != logits.device:
            raise TypeError(f"calibration_stats: {what} must be on the logits' HIP device, got {t.device} (no CPU fallback)")
    for what, v in (("bins", bins), ("classes", classes)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int)):
            raise TypeError(f"calibration_stats: {what} must be an int, got {type(v).__name__}")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)):
        raise TypeError(f"calibration_stats: temperature must be a number, got {type(temperature).__name__}")
    if logits.dim() != 4:
        raise ValueError(f"calibration_stats: expected NCHW logits, got shape {tuple(logits.shape)}")
    n, c, h, w = logits.shape
    k = c if classes is None else classes
    if not 1 <= k <= min(c, CALIB_MAX_CLASSES):
        raise ValueError(f"calibration_stats: classes must lie in 1..min(C, {CALIB_MAX_CLASSES}), got {k} with C = {c}")
    if not 1 <= bins <= CALIB_MAX_BINS:
        raise ValueError(f"calibration_stats: bins must lie in 1..{CALIB_MAX_BINS}, got {bins}")
    beta = calibration_beta(temperature)
    if tuple(labels.shape) != (n, h, w):
        raise ValueError(f"calibration_stats: labels must be [N, H, W] = {(n, h, w)}, got {tuple(labels.shape)}")
    size = CalibrationLayout(k, bins).size
    if out.dim() != 1 or out.shape[0] != size or not out.is_contiguous():
        raise ValueError(f"calibration_stats: out must be a contiguous vector of {size} elements, got {tuple(out.shape)}")
    if n > CALIB_MAX_SLICES or not (1 <= h <= CALIB_MAX_DIM and 1 <= w <= CALIB_MAX_DIM):
        raise ValueError(f"calibration_stats: needs at most {CALIB_MAX_SLICES} slices with H, W in 1..{CALIB_MAX_DIM}, got {(n, h, w)}")
    if n == 0:
        return out
    z = nhwc(logits.detach())                                  # (a network's output already is NHWC: no copy)
    nbytes = H.call("smsut_calibration_ws", n, h, w, c, k, bins)
    ws = _byte_ws(nbytes, z)
    H.call("smsut_calibration_stats", z, labels.contiguous(), out, ws, n, h, w, c, k, bins, beta, _s())
    return out


def calibration_beta(temperature):
    """The fp32 inverse temperature the kernel multiplies by: ``float32(1 / temperature)``; ``ValueError`` unless the temperature
    and that value are finite and positive."""
    import math
    import numpy as _np
    t = float(temperature)
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError(f"calibration: temperature must be finite and positive, got {temperature}")
    with _np.errstate(over="ignore"):
        beta = float(_np.float32(1.0 / t))
    if not (math.isfinite(beta) and beta > 0.0):
        raise ValueError(f"calibration: 1 / temperature = {1.0 / t} is not a positive finite float32")
    return beta
