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
* Everything else stays on the modules it is built from (``nn.LayerNorm``, ``nn.Linear``,
  ``nn.GELU``, the stem and downsample ``nn.Conv2d``).
"""
from __future__ import annotations

from typing import Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F


class LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an [N, C, H, W] tensor (a view change for channels_last)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = F.layer_norm(x.permute(0, 2, 3, 1), self.normalized_shape, self.weight, self.bias, self.eps)
        return x.permute(0, 3, 1, 2)


class Permute(nn.Module):
    def __init__(self, dims: Sequence[int]) -> None:
        super().__init__()
        self.dims = list(dims)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x.permute(self.dims)


class CNBlock(nn.Module):
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
        return x + self.layer_scale * self.block(x)


class ConvNeXt(nn.Module):
    def __init__(self, depths: Sequence[int], dims: Sequence[int], num_classes: int = 1000,
                 layer_scale: float = 1e-6, stochastic_depth_prob: float = 0.0) -> None:
        super().__init__()
        if stochastic_depth_prob != 0.0:
            raise NotImplementedError("stochastic depth is not implemented (rate must be 0)")
        layers = [nn.Sequential(nn.Conv2d(3, dims[0], kernel_size=4, stride=4), LayerNorm2d(dims[0], eps=1e-6))]
        for i, (depth, dim) in enumerate(zip(depths, dims)):
            layers.append(nn.Sequential(*[CNBlock(dim, layer_scale) for _ in range(depth)]))
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


def convnext_tiny(num_classes: int = 1000, **kw) -> ConvNeXt:
    return ConvNeXt([3, 3, 9, 3], [96, 192, 384, 768], num_classes, **kw)


def convnext_small(num_classes: int = 1000, **kw) -> ConvNeXt:
    return ConvNeXt([3, 3, 27, 3], [96, 192, 384, 768], num_classes, **kw)


def convnext_base(num_classes: int = 1000, **kw) -> ConvNeXt:
    return ConvNeXt([3, 3, 27, 3], [128, 256, 512, 1024], num_classes, **kw)
