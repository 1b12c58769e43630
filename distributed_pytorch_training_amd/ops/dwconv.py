"""Depthwise KxK "same" convolution (ConvNeXt's 7x7) on the gfx950 kernels of
csrc/kernels/dwconv_kernels.hip: channels_last, 16-bit operands, fp32 accumulation.

forward   y = dwconv(x, w) + bias in the weight's type.  x may be fp32 (a ConvNeXt block's input
          is the fp32 residual stream under autocast): the kernel rounds each element to the
          operand type as it loads it, bit for bit what autocast's cast would have written, so
          there is no cast pass and no 16-bit copy of x.
backward  input gradient: the same kernel with flipped taps, written directly in x's type;
          weight and bias gradient: fp32 partials per pixel slice summed in a fixed order
          (the ``colsum_rows`` kernel), in the weight's type: no atomics, bit-reproducible.

``DPT_NATIVE_DWCONV=0`` sends depthwise convs to ``F.conv2d`` instead (bench/dwconv_ab.py;
measured in profiles/dwconv.md).
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import native, native_available

_CL = torch.channels_last
_KIND = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
KERNEL_SIZES = (3, 5, 7)
# process-wide switch, read once at import
ENABLED = os.environ.get("DPT_NATIVE_DWCONV", "1") != "0"
# forward calls that took the native kernels (tests read it to check a model's routing)
CALLS = 0


def supported(x: torch.Tensor, w: torch.Tensor, stride, padding, dilation, groups) -> bool:
    if not (ENABLED and x.is_cuda and native_available() and x.dim() == 4 and w.dim() == 4):
        return False
    if w.dtype not in (torch.bfloat16, torch.float16) or x.dtype not in (w.dtype, torch.float32):
        return False
    c, k = x.shape[1], w.shape[2]
    if not (groups == c == w.shape[0] and w.shape[1] == 1 and w.shape[3] == k and k in KERNEL_SIZES and c % 8 == 0):
        return False
    return (tuple(stride) == (1, 1) and tuple(dilation) == (1, 1) and tuple(padding) == ((k - 1) // 2,) * 2
            and x.is_contiguous(memory_format=_CL))


def reference_dwconv(x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """The PyTorch composition (and the CPU path)."""
    return F.conv2d(x, w, bias, 1, (w.shape[2] - 1) // 2, 1, x.shape[1])


def _cl(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous(memory_format=_CL) else t.contiguous(memory_format=_CL)


class _DwConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias):
        ctx.save_for_backward(x, w)
        ctx.bias_dtype = None if bias is None else bias.dtype
        return native().dwconv_fwd(x, w, bias)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _cl(dy if dy.dtype == w.dtype else dy.to(w.dtype))
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = native().dwconv_dgrad(dy, w, x.dtype == torch.float32)
        if ctx.needs_input_grad[1] or (ctx.bias_dtype is not None and ctx.needs_input_grad[2]):
            dw, db = native().dwconv_wgrad(dy, x, w.shape[2], _KIND[w.dtype])
            db = None if ctx.bias_dtype is None else db.to(ctx.bias_dtype)
        return dx, dw, db


def dwconv2d(x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """Depthwise stride-1 "same" conv of a channels_last x [N, C, H, W] with w [C, 1, K, K].  GPU
    tensors run the native kernels (an unsupported shape or type raises: no quiet fallback)."""
    if not x.is_cuda:
        return reference_dwconv(x, w, bias)
    global CALLS
    CALLS += 1
    return _DwConv.apply(_cl(x), w.contiguous(), bias)
