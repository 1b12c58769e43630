"""Patchify convolution with bias (kernel == stride, no padding: ConvNeXt's 4x4 stride-4 stem and
2x2 stride-2 downsamples) on the gfx950 kernels of csrc/kernels/patchconv_kernels.hip:
channels_last, 16-bit operands, fp32 accumulation on the matrix cores.

forward   y = conv(x, w) + bias in the weight's type, the bias added in fp32 before the single
          rounding.  The stem's x may be fp32 (the input image under autocast): the kernel rounds
          each element to the operand type as it loads it, bit for bit autocast's cast.
backward  input gradient (2x2 only; the stem's input needs none): one GEMM scattered back to
          the patches, every element of dx written once; weight and bias gradient: fp32 partials
          per row slice summed in a fixed order (``sum_partials``), in the weight's type: no
          atomics, bit-reproducible.

Supported: k = 2 with C % 32 == 0, k = 4 with C == 3; Cout % 32 == 0.
``DPT_NATIVE_PATCHCONV=0`` sends these convs to ``F.conv2d`` instead (bench/patchconv_ab.py;
measured in profiles/patchconv.md).
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import native, native_available

_CL = torch.channels_last
_KIND = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
# process-wide switch, read once at import
ENABLED = os.environ.get("DPT_NATIVE_PATCHCONV", "1") != "0"
# forward calls that took the native kernels (tests read it to check a model's routing)
CALLS = 0


def _shape_ok(c: int, cout: int, k: int) -> bool:
    return cout > 0 and cout % 32 == 0 and ((k == 2 and c > 0 and c % 32 == 0) or (k == 4 and c == 3))


def supported(x: torch.Tensor, w: torch.Tensor, bias, stride, padding, dilation, groups) -> bool:
    if not (ENABLED and x.is_cuda and native_available() and x.dim() == 4 and w.dim() == 4 and bias is not None):
        return False
    if w.dtype not in (torch.bfloat16, torch.float16) or x.dtype not in (w.dtype, torch.float32):
        return False
    if bias.dtype not in (w.dtype, torch.float32):
        return False
    k = w.shape[2]
    if not (groups == 1 and w.shape[3] == k and x.shape[1] == w.shape[1] and _shape_ok(w.shape[1], w.shape[0], k)):
        return False
    return (tuple(stride) == (k, k) and tuple(dilation) == (1, 1) and tuple(padding) == (0, 0)
            and x.is_contiguous(memory_format=_CL))


def reference_patchconv(x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """The PyTorch composition (and the CPU path)."""
    return F.conv2d(x, w, bias, w.shape[2])


def _cl(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous(memory_format=_CL) else t.contiguous(memory_format=_CL)


class _PatchConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias):
        ctx.save_for_backward(x, w)
        ctx.bias_dtype = None if bias is None else bias.dtype
        return native().patchconv_fwd(x, w, bias)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _cl(dy if dy.dtype == w.dtype else dy.to(w.dtype))
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = native().patchconv_dgrad(dy, w, x.shape[2], x.shape[3])
        if ctx.needs_input_grad[1] or (ctx.bias_dtype is not None and ctx.needs_input_grad[2]):
            dw, db = native().patchconv_wgrad(dy, x, w.shape[2], _KIND[w.dtype])
            db = None if ctx.bias_dtype is None else db.to(ctx.bias_dtype)
        return dx, dw, db


def patch_conv2d(x: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """Conv of a channels_last x [N, C, H, W] with w [Cout, C, k, k] at stride k, no padding.  GPU
    tensors run the native kernels (an unsupported shape or type raises: no quiet fallback)."""
    if not x.is_cuda:
        return reference_patchconv(x, w, bias)
    k = w.shape[2]
    if not (w.dim() == 4 and x.dim() == 4 and w.shape[3] == k and _shape_ok(w.shape[1], w.shape[0], k)):
        raise ValueError(f"patch_conv2d: unsupported weight {tuple(w.shape)} (k = 2 with C % 32 == 0 or k = 4 with "
                         "C == 3; Cout % 32 == 0)")
    if x.dtype != w.dtype and not (k == 4 and x.dtype == torch.float32):
        x = x.to(w.dtype)      # only the stem kernel reads fp32
    global CALLS
    CALLS += 1
    return _PatchConv.apply(_cl(x), w, bias)
