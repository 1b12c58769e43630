"""ConvNeXt block ops on the gfx950 kernels of csrc/kernels/cnx_kernels.hip and grn_kernels.hip.

* ``channel_layer_norm16(y, weight, bias, eps, dtype)``  LayerNorm over the last (channel) dim of
  a channels-last activation viewed as [.., C], written directly in ``dtype`` (bf16 / fp16): y is
  16-bit (a depthwise conv's output) or fp32 (the residual stream in front of a downsample).  The
  backward gives the input gradient in y's type and dgamma / dbeta in one pass.
* ``scale_residual(x, z, b2, ls)``  out = x + ls * (z + b2) in fp32: z is fc2's output WITHOUT its
  bias (16-bit), x the residual stream (fp32; 16-bit directly after a stem / downsample conv).
  The backward writes dz = ls * dout and the column sums for dls and db2 in one pass; the
  residual gradient is dout itself.
* ``gelu_grn16(u, b1, gamma, beta, rows_per_sample, eps)``  ConvNeXt V2's bias + GELU + Global
  Response Normalization between fc1 and fc2: y = GELU(u + b1), G = ||y||_2 over the
  ``rows_per_sample`` rows of a sample, Nx = G / (mean over D of G + eps), g = gamma * (y * Nx) +
  beta + y in u's 16-bit type.  u [.., D] is fc1's output WITHOUT its bias.  y is not stored: the
  backward recomputes it from u and keeps only the per-(sample, channel) statistics.

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


class _GeluGrn16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, b1, gamma, beta, rows_per_sample, eps):
        g, G, inv, s = native().cnx_grn_fwd(u, b1, gamma, beta, int(rows_per_sample), float(eps))
        ctx.save_for_backward(u, b1, gamma, G, inv, s)
        ctx.rows_per_sample = int(rows_per_sample)
        return g

    @staticmethod
    def backward(ctx, dg):
        u, b1, gamma, G, inv, s = ctx.saved_tensors
        du, db1, dgamma, dbeta = native().cnx_grn_bwd(dg.contiguous(), u, b1, gamma, G, inv, s, ctx.rows_per_sample)
        return du, db1, dgamma, dbeta, None, None


def grn_supported(x: torch.Tensor, dim: int) -> bool:
    return x.is_cuda and native_available() and native().cnx_grn_supported(dim)


def gelu_grn16(u: torch.Tensor, b1: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, rows_per_sample: int,
               eps: float = 1e-6) -> torch.Tensor:
    """GRN(GELU(u + b1)) in u's dtype for u [.., D] whose rows come in samples of ``rows_per_sample``;
    b1, gamma, beta [D] (gamma / beta fp32 on the GPU)."""
    D = u.shape[-1]
    if not u.is_cuda:
        ct = torch.promote_types(u.dtype, torch.float32)     # 16-bit operands compute in fp32
        y = F.gelu(u.to(ct) + b1.to(ct)).reshape(-1, rows_per_sample, D)
        G = torch.linalg.vector_norm(y, ord=2, dim=1, keepdim=True)
        Nx = G / (G.mean(dim=-1, keepdim=True) + eps)
        return (gamma.to(ct) * (y * Nx) + beta.to(ct) + y).reshape(u.shape).to(u.dtype)
    global CALLS
    CALLS += 1
    return _GeluGrn16.apply(u.contiguous(), b1.contiguous(), gamma.contiguous(), beta.contiguous(),
                            rows_per_sample, eps)
