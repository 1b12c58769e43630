"""ConvNeXt-T/S/B with torchvision-identical parameter names, shapes and init
(ConvNeXt-T: 28,589,128 parameters at 1000 classes).

Layout: ``features.0`` the stem (4x4 stride-4 conv + channels-first LayerNorm), ``features.{1,3,5,7}``
the four stages of blocks, ``features.{2,4,6}`` the downsamples (LayerNorm + 2x2 stride-2 conv),
``classifier`` = LayerNorm, Flatten, Linear.  A block is ``x + layer_scale * block(x)`` with
``block`` = depthwise 7x7 conv (0), permute to NHWC, LayerNorm (2), Linear (3), GELU, Linear (5),
permute back.

Stochastic depth is not implemented: its rate defaults to 0 and any other value raises (the
published recipe's 0.1 needs device-side RNG).

MI355X notes
------------
* Under bf16 / fp16 autocast with weight shadows and channels_last activations the depthwise
  convs run csrc/kernels/dwconv_kernels.hip (ops/dwconv.py, routed by parallel/shadow.py): the
  block's input is the fp32 residual stream, which the kernels read as it is.
* In the native engine (``set_native``; a freshly built model and the stock engine stay module by
  module) a block under bf16 / fp16 autocast on channels_last GPU activations runs the
  depthwise conv, ``channel_layer_norm16`` (ops/convnext.py,
  csrc/kernels/cnx_kernels.hip: LayerNorm over the channels of the conv's 16-bit output, several
  rows per wave, written as the 16-bit GEMM operand), ``linear16`` and ``gelu_linear16`` of
  ops/vit.py (bias-free fc1, bias + GELU, fc2 with the fused backward where ``dim % 64 == 0``),
  and ``scale_residual`` (``x + layer_scale * (fc2 + bias)`` in one fp32 pass whose backward
  also gives the layer-scale and bias gradients).  ``LayerNorm2d`` (stem, downsamples,
  classifier) takes ``channel_layer_norm16`` too and hands 16 bits to the conv / Linear that
  follows.  Widths: 96 / 192 / 384 / 768 and 128 / 256 / 512 / 1024; ``DPT_NATIVE_CNBLOCK=0``
  switches the route off (profiles/convnext_block.md).
* The stem (4x4 stride 4, reading the fp32 image) and the downsample convs (2x2 stride 2), all with
  a bias, run csrc/kernels/patchconv_kernels.hip under the same conditions (ops/patchconv.py,
  routed by parallel/shadow.py): bias and bias gradient in the epilogues, no MIOpen kernel left in
  the step; ``DPT_NATIVE_PATCHCONV=0`` sends them back to ``F.conv2d`` (profiles/patchconv.md).

ConvNeXt V2 (``convnextv2_tiny`` 28,635,496 parameters at 1000 classes, ``convnextv2_base``) keeps this
layout and swaps the block: no layer scale, and Global Response Normalization between the MLP's
GELU and fc2.  ``CNBlockV2`` names its parameters as the official checkpoints do (``dwconv``,
``norm``, ``pwconv1``, ``grn.gamma`` / ``grn.beta`` of shape [1, 1, 1, 4 dim], ``pwconv2``); the
containers around the blocks are the V1 ones above.  Its native route, under the same conditions, is
the depthwise conv, ``channel_layer_norm16``, ``linear16`` (bias-free fc1), ``gelu_grn16``
(ops/convnext.py, csrc/kernels/grn_kernels.hip: bias + GELU + GRN without storing the GELU's
output), ``linear16`` (fc2) and ``scale_residual`` with a unit scale (profiles/convnext_v2_grn.md).
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import convnext as cnx
from ..ops.vit import gelu_linear16, linear16
from ..parallel.shadow import shadow_param
from .vit import _bias16


def _native_route(mod: nn.Module, x: torch.Tensor, dim: int) -> bool:
    """The conditions of the native block / LayerNorm route (module docstring)."""
    if not (mod.dpt_native and cnx.ENABLED and x.is_cuda and x.dim() == 4):
        return False
    if not (torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") in (torch.bfloat16, torch.float16)):
        return False
    return x.is_contiguous(memory_format=torch.channels_last) and cnx.ln_supported(x, dim)


class LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an [N, C, H, W] tensor (a view change for channels_last)."""
    dpt_native = False   # set_native: channel_layer_norm16, 16-bit output

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if _native_route(self, x, self.normalized_shape[0]):
            dt = torch.get_autocast_dtype("cuda")
            rows = x.permute(0, 2, 3, 1)
            if rows.dtype not in (dt, torch.float32):
                rows = rows.float()
            return cnx.channel_layer_norm16(rows, self.weight, self.bias, self.eps, dt).permute(0, 3, 1, 2)
        x = F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps)
        return x.permute(0, 3, 1, 2)


class Permute(nn.Module):
    def __init__(self, dims: Sequence[int]) -> None:
        super().__init__()
        self.dims = list(dims)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x.permute(self.dims)


class CNBlock(nn.Module):
    dpt_native = False   # set_native: the fused route of _forward_native

    def __init__(self, dim: int, layer_scale: float) -> None:
        super().__init__()
        self.block = nn.Sequential(
            nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim, bias=True),
            Permute([0, 2, 3, 1]),
            nn.LayerNorm(dim, eps=1e-6),
            nn.Linear(dim, 4 * dim),
            nn.GELU(),
            nn.Linear(4 * dim, dim),
            Permute([0, 3, 1, 2]),
        )
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * layer_scale)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if _native_route(self, x, self.layer_scale.shape[0]):
            return self._forward_native(x)
        return x + self.layer_scale * self.block(x)

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        dt = torch.get_autocast_dtype("cuda")
        ln, fc1, fc2 = self.block[2], self.block[3], self.block[5]
        y = self.block[0](x)                              # depthwise conv: 16-bit, channels_last
        h = cnx.channel_layer_norm16(y.permute(0, 2, 3, 1), ln.weight, ln.bias, ln.eps, dt)
        u = linear16(h, shadow_param(fc1, "weight", h))   # biases move into the next kernels
        z = gelu_linear16(u, _bias16(fc1, "bias", h), shadow_param(fc2, "weight", h))
        xr = x.permute(0, 2, 3, 1)
        if xr.dtype not in (dt, torch.float32):
            xr = xr.float()
        out = cnx.scale_residual(xr, z, _bias16(fc2, "bias", h), self.layer_scale.flatten())
        return out.permute(0, 3, 1, 2)


class ConvNeXt(nn.Module):
    @staticmethod
    def make_block(dim: int, layer_scale: float) -> nn.Module:
        return CNBlock(dim, layer_scale)

    def __init__(self, depths: Sequence[int], dims: Sequence[int], num_classes: int = 1000,
                 layer_scale: float = 1e-6, stochastic_depth_prob: float = 0.0) -> None:
        super().__init__()
        if stochastic_depth_prob != 0.0:
            raise NotImplementedError("stochastic depth is not implemented (rate must be 0)")
        layers = [nn.Sequential(nn.Conv2d(3, dims[0], kernel_size=4, stride=4), LayerNorm2d(dims[0], eps=1e-6))]
        for i, (depth, dim) in enumerate(zip(depths, dims)):
            layers.append(nn.Sequential(*[self.make_block(dim, layer_scale) for _ in range(depth)]))
            if i + 1 < len(dims):
                layers.append(nn.Sequential(LayerNorm2d(dim, eps=1e-6),
                                            nn.Conv2d(dim, dims[i + 1], kernel_size=2, stride=2)))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(LayerNorm2d(dims[-1], eps=1e-6), nn.Flatten(1),
                                        nn.Linear(dims[-1], num_classes))
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.classifier(self.avgpool(self.features(x)))


class GRN(nn.Module):
    """Global Response Normalization over an [N, H, W, D] activation (ConvNeXt V2): parameters
    ``gamma`` / ``beta`` [1, 1, 1, D] start at zero, so a fresh layer is the identity."""

    def __init__(self, dim: int, eps: float = 1e-6) -> None:
        super().__init__()
        self.gamma = nn.Parameter(torch.zeros(1, 1, 1, dim))
        self.beta = nn.Parameter(torch.zeros(1, 1, 1, dim))
        self.eps = eps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        gx = torch.linalg.vector_norm(x, ord=2, dim=(1, 2), keepdim=True)
        nx = gx / (gx.mean(dim=-1, keepdim=True) + self.eps)
        return self.gamma * (x * nx) + self.beta + x


_ONES = {}   # (device, dim) -> fp32 ones: the unit layer scale of a V2 block's tail


def _ones(dim: int, device: torch.device) -> torch.Tensor:
    key = (device, dim)
    if key not in _ONES:
        _ONES[key] = torch.ones(dim, device=device)
    return _ONES[key]


class CNBlockV2(nn.Module):
    """A ConvNeXt V2 block with the official checkpoint's parameter names: ``dwconv``, ``norm``,
    ``pwconv1``, ``grn.gamma`` / ``grn.beta``, ``pwconv2``; no layer scale."""
    dpt_native = False   # set_native: the fused route of _forward_native

    def __init__(self, dim: int) -> None:
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim, bias=True)
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.grn = GRN(4 * dim)
        self.pwconv2 = nn.Linear(4 * dim, dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        dim = self.norm.normalized_shape[0]
        if _native_route(self, x, dim) and cnx.grn_supported(x, 4 * dim):
            return self._forward_native(x)
        y = self.norm(self.dwconv(x).permute(0, 2, 3, 1))
        y = self.pwconv2(self.grn(self.act(self.pwconv1(y))))
        return x + y.permute(0, 3, 1, 2)

    def _forward_native(self, x: torch.Tensor) -> torch.Tensor:
        dt = torch.get_autocast_dtype("cuda")
        ln, fc1, fc2 = self.norm, self.pwconv1, self.pwconv2
        y = self.dwconv(x)                                # depthwise conv: 16-bit, channels_last
        h = cnx.channel_layer_norm16(y.permute(0, 2, 3, 1), ln.weight, ln.bias, ln.eps, dt)
        u = linear16(h, shadow_param(fc1, "weight", h))   # biases move into the next kernels
        g = cnx.gelu_grn16(u, _bias16(fc1, "bias", h), self.grn.gamma.flatten(), self.grn.beta.flatten(),
                           u.shape[1] * u.shape[2], self.grn.eps)
        z = linear16(g, shadow_param(fc2, "weight", h))
        xr = x.permute(0, 2, 3, 1)
        if xr.dtype not in (dt, torch.float32):
            xr = xr.float()
        out = cnx.scale_residual(xr, z, _bias16(fc2, "bias", h), _ones(z.shape[-1], z.device))
        return out.permute(0, 3, 1, 2)


class ConvNeXtV2(ConvNeXt):
    """ConvNeXt V2: the V1 layout (``features`` / ``classifier``) with CNBlockV2 blocks."""
    @staticmethod
    def make_block(dim: int, layer_scale: float) -> nn.Module:
        return CNBlockV2(dim)

    def __init__(self, depths: Sequence[int], dims: Sequence[int], num_classes: int = 1000,
                 stochastic_depth_prob: float = 0.0) -> None:
        super().__init__(depths, dims, num_classes, 0.0, stochastic_depth_prob)


def set_native(model: nn.Module, on: bool = True) -> int:
    """Route a ConvNeXt's blocks and channel LayerNorms through the native kernels (on) or the
    modules they are built from (off, the default of a freshly built model); returns how many
    modules were switched."""
    n = 0
    for m in model.modules():
        if isinstance(m, (CNBlock, CNBlockV2, LayerNorm2d)):
            m.dpt_native = bool(on)
            n += 1
    return n


def convnext_tiny(num_classes: int = 1000, **kw) -> ConvNeXt:
    return ConvNeXt([3, 3, 9, 3], [96, 192, 384, 768], num_classes, **kw)


def convnext_small(num_classes: int = 1000, **kw) -> ConvNeXt:
    return ConvNeXt([3, 3, 27, 3], [96, 192, 384, 768], num_classes, **kw)


def convnext_base(num_classes: int = 1000, **kw) -> ConvNeXt:
    return ConvNeXt([3, 3, 27, 3], [128, 256, 512, 1024], num_classes, **kw)


def convnextv2_tiny(num_classes: int = 1000, **kw) -> ConvNeXtV2:
    return ConvNeXtV2([3, 3, 9, 3], [96, 192, 384, 768], num_classes, **kw)


def convnextv2_base(num_classes: int = 1000, **kw) -> ConvNeXtV2:
    return ConvNeXtV2([3, 3, 27, 3], [128, 256, 512, 1024], num_classes, **kw)
