"""ConvNeXt block ops on the gfx950 kernels of csrc/kernels/cnx_kernels.hip.

* ``channel_layer_norm16(y, weight, bias, eps, dtype)``  LayerNorm over the last (channel) dim of
  a channels-last activation viewed as [.., C], written directly in ``dtype`` (bf16 / fp16): y is
  16-bit (a depthwise conv's output) or fp32 (the residual stream in front of a downsample).  The
  backward gives the input gradient in y's type and dgamma / dbeta in one pass.
* ``scale_residual(x, z, b2, ls)``  out = x + ls * (z + b2) in fp32: z is fc2's output WITHOUT its
  bias (16-bit), x the residual stream (fp32; 16-bit directly after a stem / downsample conv).
  The backward writes dz = ls * dout and the column sums for dls and db2 in one pass; the
  residual gradient is dout itself.

Semantics equal the PyTorch composition under autocast up to rounding order.  CPU tensors run
that composition through the same signatures; an unsupported GPU input raises (no quiet
fallback).  ``DPT_NATIVE_CNBLOCK=0`` keeps models/convnext.py on the module-by-module path
(bench/cnblock_ab.py; measured in profiles/convnext_block.md).
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import native, native_available

_KIND = {torch.bfloat16: 1, torch.float16: 2}
# process-wide switch, read once at import
ENABLED = os.environ.get("DPT_NATIVE_CNBLOCK", "1") != "0"
# forward calls that took the native kernels (tests read it to check a model's routing)
CALLS = 0


def ln_supported(x: torch.Tensor, dim: int) -> bool:
    return x.is_cuda and native_available() and native().cnx_ln_supported(dim)


class _ChannelLayerNorm16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, weight, bias, eps, kind):
        h, mean, rstd = native().cnx_ln_fwd(y, weight, bias, float(eps), int(kind))
        ctx.save_for_backward(y, weight, mean, rstd)
        return h

    @staticmethod
    def backward(ctx, gh):
        y, weight, mean, rstd = ctx.saved_tensors
        gy, dg, db = native().cnx_ln_bwd(gh.contiguous(), y, mean, rstd, weight)
        return gy, dg, db, None, None


class _ScaleResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, z, b2, ls):
        ctx.save_for_backward(z, b2, ls)
        return native().cnx_scale_residual_fwd(x, z, b2, ls)

    @staticmethod
    def backward(ctx, dout):
        z, b2, ls = ctx.saved_tensors
        dz, dls, db2 = native().cnx_scale_residual_bwd(dout.contiguous(), z, b2, ls)
        return dout, dz, db2, dls


def channel_layer_norm16(y: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float,
                         dtype: torch.dtype) -> torch.Tensor:
    """LayerNorm over the last dim of y [.., C] (fp32 or ``dtype``) returned in ``dtype``."""
    if not y.is_cuda:
        return F.layer_norm(y.float(), (y.shape[-1],), weight, bias, eps).to(dtype)
    global CALLS
    CALLS += 1
    return _ChannelLayerNorm16.apply(y.contiguous(), weight, bias, eps, _KIND[dtype])


def scale_residual(x: torch.Tensor, z: torch.Tensor, b2: torch.Tensor, ls: torch.Tensor) -> torch.Tensor:
    """x + ls * (z + b2) in fp32 for x, z [.., C] and per-channel b2, ls [C]."""
    if not x.is_cuda:
        return x.float() + ls.float() * (z.float() + b2.float())
    global CALLS
    CALLS += 1
    return _ScaleResidual.apply(x.contiguous(), z.contiguous(), b2.contiguous(), ls.contiguous())
