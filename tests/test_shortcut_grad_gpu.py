"""Compact identity-path gradient of the 1x1 / stride-2 downsample convs (ops/conv.py
S2_COMPACT_DRES).

With the switch on, the downsample conv on a block tail's identity alias writes its input gradient
as [N, C, ceil(H/2), ceil(W/2)] and the tail's conv-path consumer reads it with a strided
residual in its BNR epilogue; with it off, the gradient is the full-resolution tensor with
explicit zeros at three pixels of every 2x2 cell.  Same GEMMs, same adds (+0.0 where there is no
identity gradient): every comparison is bit for bit.  No placeholder tensor exists in the compact
path (the downsample conv returns None to autograd), so there is nothing to poison.
"""
import copy

import pytest
import torch
import torch.nn as nn

from distributed_pytorch_training_amd import ops
from distributed_pytorch_training_amd.models import layers
from distributed_pytorch_training_amd.models.resnet import BasicBlock, Bottleneck
from distributed_pytorch_training_amd.ops import conv as native_conv

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _rand(shape, dtype, dev, g, scale=1.0):
    t = (torch.randn(shape, device=dev, generator=g) * scale).to(dtype)
    return t.contiguous(memory_format=CL) if len(shape) == 4 else t


def _expand(compact, H, W):
    """The zero-expanded [N, C, H, W] form of a compact stride-2 gradient (+0.0 elsewhere)."""
    n, c = compact.shape[:2]
    full = torch.zeros((n, c, H, W), dtype=compact.dtype, device=compact.device).contiguous(memory_format=CL)
    full[:, :, ::2, ::2] = compact
    return full


# ---- kernel level ------------------------------------------------------------------------------
@pytest.mark.parametrize("splitk", [1, 2], ids=["in-kernel", "split-epilogue"])
@pytest.mark.parametrize("mask", [True, False], ids=["mask", "bny"])
@pytest.mark.parametrize("mid", [64, 256])  # 256: four K-steps, the fewest the split-K path takes
@pytest.mark.parametrize("hw", [10, 7])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_strided_residual_epilogue_is_bitwise_the_zero_expanded_one(cuda, dtype, hw, mid, mask, splitk):
    """conv_dgrad_bnstats of a 1x1 conv (mid <- 128 tail channels) on a tail source.  N = 3,
    H = W = 10: M = 300 is three 128-row tiles, the last partial, tiles straddle image borders and
    even and odd rows share a tile; H = W = 7: odd sizes (compact 4 x 4)."""
    C_ = ops.native()
    N, C, H, W = 3, 128, hw, hw
    M = N * H * W
    g = torch.Generator(device=cuda).manual_seed(1000 + hw + mid)
    w = _rand((mid, C, 1, 1), dtype, cuda, g, 0.1)
    gy = _rand((N, mid, H, W), dtype, cuda, g)
    bnx = _rand((N, C, H, W), dtype, cuda, g)
    bny = torch.relu(_rand((N, C, H, W), dtype, cuda, g))
    mean = torch.randn(C, device=cuda, generator=g) * 0.1
    compact = _rand((N, C, (H + 1) // 2, (W + 1) // 2), dtype, cuda, g)
    compact[0, :8, 0, 0] = -0.0  # a signed zero in the gradient itself survives both ways
    full = _expand(compact, H, W)
    bits = None
    if mask:
        pos = (bny.permute(0, 2, 3, 1).reshape(M, C // 8, 8) > 0).to(torch.int32)
        bits = (pos << torch.arange(8, device=cuda, dtype=torch.int32)).sum(-1).to(torch.uint8).contiguous()
    wt = C_.conv_wt_flip_multi([w])[0]
    split = C_.conv_fwd_splits(M, C, mid, True) > 1
    assert split == (mid >= 256)
    C_.conv_set_splitk(splitk)
    try:
        ref = C_.conv_dgrad_bnstats(gy, w, 0, bnx, mean, None, bny, full, wt, bn_mask=bits)
        out = C_.conv_dgrad_bnstats(gy, w, 0, bnx, mean, None, bny, compact, wt, bn_mask=bits, bn_res_s2=True)
    finally:
        C_.conv_set_splitk(1)
    if splitk == 2 and split:  # partial columns per 16-row slab: the split epilogue ran
        assert ref[1].shape[1] == (M + 15) // 16
    for name, a, b in zip(("dz", "p1", "p2"), ref, out):
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert torch.isfinite(a.float()).all() and a.float().abs().max() > 0, name
        assert torch.equal(_bits(a), _bits(b)), f"{name}: {(_bits(a) != _bits(b)).sum().item()} elements differ"


@pytest.mark.parametrize("splitk", [1, 2], ids=["in-kernel", "split-epilogue"])
@pytest.mark.parametrize("hw", [10, 7])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_compact_downsample_gradient_is_the_even_pixels_of_the_full_one(cuda, dtype, hw, splitk):
    C_ = ops.native()
    N, C, Cout = 3, 256, 512
    ho = (hw + 1) // 2
    g = torch.Generator(device=cuda).manual_seed(2000 + hw)
    w = _rand((Cout, C, 1, 1), dtype, cuda, g, 0.1)
    gy = _rand((N, Cout, ho, ho), dtype, cuda, g)
    C_.conv_set_splitk(splitk)
    try:
        full = C_.conv_dgrad_s2(gy, w, 0, hw, hw)[0]
        compact = C_.conv_dgrad_s2(gy, w, 0, hw, hw, compact=True)[0]
    finally:
        C_.conv_set_splitk(1)
    assert compact.shape == (N, C, ho, ho) and compact.is_contiguous(memory_format=CL)
    assert compact.float().abs().max() > 0
    assert torch.equal(_bits(full), _bits(_expand(compact, hw, hw)))


# ---- block level -------------------------------------------------------------------------------
class _Conv(nn.Module):
    """A bias-free conv on the MFMA kernels with a 16-bit weight parameter (what the shadow
    weights of the training engine give the model's convs)."""

    def __init__(self, ref: nn.Conv2d, dtype, g):
        super().__init__()
        w = torch.randn(ref.weight.shape, device="cuda", generator=g) * (2.0 / ref.weight[0].numel()) ** 0.5
        self.weight = nn.Parameter(w.to(dtype).contiguous(memory_format=CL))
        self.stride, self.pad = ref.stride[0], ref.padding[0]

    def forward(self, x):
        return native_conv.conv2d(x, self.weight, self.stride, self.pad, bn_stats=True)


def _two_blocks(kind, dtype, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    if kind == "bottleneck":  # 256 -> 64 -> 256 (a fused tail), then 256 -> 128 -> 512 / stride 2
        ds = nn.Sequential(nn.Conv2d(256, 512, 1, 2, bias=False), nn.BatchNorm2d(512))
        net = nn.Sequential(Bottleneck(256, 64), Bottleneck(256, 128, 2, ds))
        cin = 256
    else:                     # 64 -> 64, then 64 -> 128 / stride 2
        ds = nn.Sequential(nn.Conv2d(64, 128, 1, 2, bias=False), nn.BatchNorm2d(128))
        net = nn.Sequential(BasicBlock(64, 64), BasicBlock(64, 128, 2, ds))
        cin = 64
    net = net.to(dev)
    for parent in list(net.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, nn.Conv2d):
                setattr(parent, name, _Conv(child, dtype, g))
    layers.fuse_batchnorm(net)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, device=dev, generator=g) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, device=dev, generator=g) - 0.5)
    x = _rand((2, cin, 8, 8), dtype, dev, g)
    return net.train(), x


def _block_grads(net0, x0, compact, monkeypatch, fuse_fwd=True, fuse_bwd=True):
    monkeypatch.setattr(native_conv, "S2_COMPACT_DRES", compact)
    monkeypatch.setattr(native_conv, "BN_BWD_FUSE", fuse_fwd)
    native_conv.reset_side_channels()
    net = copy.deepcopy(net0)
    x = x0.detach().clone().requires_grad_(True)
    y = net(x)
    y = y[0] if isinstance(y, tuple) else y
    g = torch.Generator(device=x.device).manual_seed(8)
    gy = _rand(tuple(y.shape), y.dtype, x.device, g)
    monkeypatch.setattr(native_conv, "BN_BWD_FUSE", fuse_bwd)
    y.backward(gy)
    assert not native_conv._BNB_PARTIALS
    out = {"x": x.grad}
    out.update({n: p.grad for n, p in net.named_parameters()})
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert a[name] is not None and b[name] is not None, name
        assert torch.isfinite(a[name].float()).all(), name
        assert torch.equal(_bits(a[name]), _bits(b[name])), \
            f"{name}: {(_bits(a[name]) != _bits(b[name])).sum().item()} elements differ"


@pytest.mark.parametrize("kind", ["bottleneck", "basic"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_blocks_switch_on_is_bitwise_switch_off(cuda, dtype, kind, monkeypatch):
    net, x = _two_blocks(kind, dtype, cuda)
    calls = []
    real = ops.native().conv_dgrad_bnstats
    off = _block_grads(net, x, False, monkeypatch)

    class _Spy:
        def __getattr__(self, name):
            if name == "conv_dgrad_bnstats":
                def f(*a, **k):
                    calls.append(bool(k.get("bn_res_s2", False)))
                    return real(*a, **k)
                return f
            return getattr(ops.native(), name)

    spy = _Spy()
    monkeypatch.setattr(native_conv, "native", lambda: spy)
    on = _block_grads(net, x, True, monkeypatch)
    # the Bottleneck's stride-1 1x1 conv1 folds the compact gradient; the BasicBlock's 3x3 / stride-2
    # conv1 folds nothing, so its downsample conv keeps the full gradient
    assert any(calls) == (kind == "bottleneck")
    _same(off, on)


@pytest.mark.parametrize("kind", ["bottleneck", "basic"])
@pytest.mark.parametrize("fuse_fwd", [False, True], ids=["never-fused", "unfused-before-backward"])
def test_blocks_when_the_consumer_cannot_fold(cuda, kind, fuse_fwd, monkeypatch):
    """BN_BWD_FUSE off (for the whole step, or switched off between forward and backward): the
    conv-path consumer folds nothing, so the downsample conv must hand autograd the full gradient."""
    net, x = _two_blocks(kind, torch.bfloat16, cuda)
    off = _block_grads(net, x, False, monkeypatch, fuse_fwd, False)
    on = _block_grads(net, x, True, monkeypatch, fuse_fwd, False)
    _same(off, on)
