"""Patchify conv kernels (csrc/kernels/patchconv_kernels.hip) against fp64 ``F.conv2d`` on the CPU.

The reference reads the already rounded operands (``x.to(dt)``, w, b, dy as fp64).  Bounds, with
u = 2^-8 (bf16) / 2^-11 (fp16): one output rounding plus fp32 accumulation of n terms in any order,
evaluated on the absolute-value operands:
  forward        |y - ref|  <= u |ref| + (K + 2) 2^-24 (|A| |W| + |b|),   K = k k C
  backward-data  |dx - ref| <= u |ref| + (Cout + 2) 2^-24 |dy| |W|
  dW / db        |dw - ref| <= u |ref| + (M + 2) 2^-24 sum |dy| |A|,      M = N (H/k) (W/k)
Below the output type's normal range the rounding is absolute, so every bound also carries half the
smallest subnormal (2^-25 for fp16): an fp16 dW of a single product (M = 1) below 2^-14 cannot meet
a purely relative bound.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from distributed_pytorch_training_amd import ops
from distributed_pytorch_training_amd.ops import patchconv

pytestmark = pytest.mark.gpu

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
KIND = {torch.bfloat16: 1, torch.float16: 2}
# name: (k, N, C, Cout, H, W, x is fp32); the row tile is 128 (asserted below)
SHAPES = {
    "tiny": (2, 1, 32, 64, 2, 2, False),         # M = 1
    "odd": (2, 2, 96, 192, 5, 7, False),         # floor drops a row and a column; K = 384; partial column tile
    "edge": (2, 3, 128, 256, 2, 86, False),      # M = TM + 1: a tile spans three images, the next holds one row
    "slices": (2, 2, 96, 192, 34, 32, False),    # M = 544: two row slices of 5 and 4 K-steps, the last one short
    "stem": (4, 2, 3, 96, 8, 12, False),
    "stem-f32": (4, 2, 3, 96, 8, 12, True),
    "stem-odd": (4, 2, 3, 96, 9, 14, False),     # floor, and rows of x that are not 8 / 16-byte aligned
    "stem-odd-f32": (4, 2, 3, 96, 9, 14, True),
    "stem-slices": (4, 2, 3, 96, 64, 62, True),  # M = 480: two row slices through the stem's column-sum reduction
}


def _inputs(shape, dt, cuda, seed=0):
    k, n, c, cout, h, w_, f32 = SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    cl = torch.channels_last
    x = torch.randn(n, c, h, w_, generator=g).to(torch.float32 if f32 else dt).to(cuda).contiguous(memory_format=cl)
    w = (torch.randn(cout, c, k, k, generator=g) / (k * k * c) ** 0.5).to(dt).to(cuda).contiguous(memory_format=cl)
    b = torch.randn(cout, generator=g).to(dt).to(cuda)
    dy = torch.randn(n, cout, h // k, w_ // k, generator=g).to(dt).to(cuda).contiguous(memory_format=cl)
    return x, w, b, dy


def _ref(x, w, b, dy):
    """fp64 (y, dx, dw, db) of the conv on the CPU."""
    x, w, b = (t.detach().double().cpu().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(x, w, b, stride=w.shape[2])
    dx, dw, db = torch.autograd.grad(y, (x, w, b), dy.double().cpu())
    return y.detach(), dx, dw, db


def _within(out, ref, u, slack, what):
    err = (out.double().cpu() - ref).abs()
    fi = torch.finfo(out.dtype)
    bound = u * ref.abs() + slack + fi.smallest_normal * fi.eps / 2   # half the smallest subnormal
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max err/bound {worst:.3f}")
    assert out.shape == ref.shape and bool((err <= bound).all()), (what, err.max().item(), worst)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_three_passes_against_fp64(cuda, dt, shape):
    nat = ops.native()
    assert nat.patchconv_tiles() == (128, 128)
    k, n, c, cout, h, w_, _ = SHAPES[shape]
    x, w, b, dy = _inputs(shape, dt, cuda)
    M = n * (h // k) * (w_ // k)
    if shape.endswith("slices"):
        assert nat.patchconv_wgrad_slices(M, cout, c, k) == 2
    y = nat.patchconv_fwd(x, w, b)
    dw, db = nat.patchconv_wgrad(dy, x, k, KIND[dt])
    assert y.dtype == dt and dw.dtype == dt and db.dtype == dt and y.is_contiguous(memory_format=torch.channels_last)
    x16 = x.to(dt)
    ry, rdx, rdw, rdb = _ref(x16, w, b, dy)
    ay, adx, adw, adb = _ref(x16.abs(), w.abs(), b.abs(), dy.abs())
    e = 2.0 ** -24
    _within(y, ry, U[dt], (k * k * c + 2) * e * ay, "y")
    _within(dw, rdw, U[dt], (M + 2) * e * adw, "dw")
    _within(db, rdb, U[dt], (M + 2) * e * adb, "db")
    if k == 2:   # the stem's input needs no gradient
        dx = nat.patchconv_dgrad(dy, w, h, w_)
        assert dx.dtype == dt and dx.is_contiguous(memory_format=torch.channels_last)
        _within(dx, rdx, U[dt], (cout + 2) * e * adx, "dx")
        assert not dx[:, :, 2 * (h // 2):, :].any() and not dx[:, :, :, 2 * (w_ // 2):].any()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_fp32_stem_input_rounds_like_the_cast(cuda, dt):
    nat = ops.native()
    x, w, b, dy = _inputs("stem-odd-f32", dt, cuda, seed=1)
    x16 = x.to(dt)
    assert torch.equal(nat.patchconv_fwd(x, w, b), nat.patchconv_fwd(x16, w, b))
    assert torch.equal(nat.patchconv_wgrad(dy, x, 4, KIND[dt])[0], nat.patchconv_wgrad(dy, x16, 4, KIND[dt])[0])


def test_backward_weight_is_deterministic(cuda):
    x, w, b, dy = _inputs("slices", torch.bfloat16, cuda, seed=2)
    (dw1, db1), (dw2, db2) = (ops.native().patchconv_wgrad(dy, x, 2, 0) for _ in range(2))
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)


def test_convnext_routes_patchify_convs_to_the_native_kernels(cuda, monkeypatch):
    """One bf16-autocast forward + backward of ConvNeXt-T (32 px, batch 4; M = 4 rows at the last
    downsample) through the native engine's model: the stem and the three downsamples take the
    native kernels, none with the switch off, and the native logits are no further from the fp32
    forward than twice the F.conv2d route's (+1e-6): the routes differ only in where the conv
    output is rounded."""
    from distributed_pytorch_training_amd.config import parse_args
    from distributed_pytorch_training_amd.engine.trainer import Trainer
    from distributed_pytorch_training_amd.models import build_model

    torch.manual_seed(0)
    base = build_model("convnext_tiny", 10, cuda, channels_last=True)
    args = parse_args(["--model", "convnext_tiny", "--dataset", "synthetic", "--amp", "--amp-dtype", "bf16",
                       "--channels-last", "--no-cuda-graph"])
    tr = Trainer(copy.deepcopy(base), args, 0, 1, cuda, log=lambda s: None)
    assert tr.ddp.shadow_flat is not None
    x = torch.randn(4, 3, 32, 32, device=cuda).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        ref = base(x).double()
    err = {}
    for route, calls in (("native", 4), ("stock", 0)):
        monkeypatch.setattr(patchconv, "ENABLED", route == "native")
        monkeypatch.setattr(patchconv, "CALLS", 0)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = tr.module(x)
        logits.float().sum().backward()
        assert patchconv.CALLS == calls, (route, patchconv.CALLS)
        err[route] = (logits.detach().double() - ref).abs().max().item()
    print("max |logits - fp32|:", err)
    assert err["native"] <= 2 * err["stock"] + 1e-6, err
