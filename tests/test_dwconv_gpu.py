"""Depthwise conv kernels (csrc/kernels/dwconv_kernels.hip) against fp64 ``F.conv2d`` on the CPU.

The reference reads the already rounded operands (``x.to(dt)``, w, b, dy as fp64).  Bounds, with
u = 2^-8 (bf16), 2^-11 (fp16), 2^-24 (fp32):
  forward / backward-data  |out - ref| <= u_out |ref| + (K^2 + 2) 2^-24 (|x| (*) |w| + |b|)
  backward-weight / bias   |dw - ref|  <= u_w |ref| + (P + 2) 2^-24 sum |dy| |x|,  P = N H W
(one output rounding plus fp32 accumulation of K^2 resp. P terms, in any order).
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from distributed_pytorch_training_amd import ops
from distributed_pytorch_training_amd.ops import dwconv

pytestmark = pytest.mark.gpu

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
KIND = {torch.bfloat16: 1, torch.float16: 2}
# (N, C, H, W) as functions of T, the larger pixel tile edge of the forward kernel
SHAPES = {
    "tiny": lambda T: (1, 8, 2, 3),            # smaller than the halo: every tap row meets padding
    "edges": lambda T: (2, 72, T - 1, T + 1),  # partial last channel block, tile edge -1 / +1
    "exact": lambda T: (3, 64, T, 2 * T + 1),  # exact tile; the pixel slices do not divide evenly
    "small": lambda T: (2, 96, 7, 7),          # the small-tile geometry
}


def _ref(x, w, b, dy):
    """fp64 (y, dx, dw, db) of the depthwise conv on the CPU."""
    x, w, b = (t.detach().double().cpu().requires_grad_(True) for t in (x, w, b))
    y = F.conv2d(x, w, b, padding=(w.shape[2] - 1) // 2, groups=x.shape[1])
    dx, dw, db = torch.autograd.grad(y, (x, w, b), dy.double().cpu())
    return y.detach(), dx, dw, db


def _inputs(shape, K, dt, act, cuda, seed=0):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w_ = shape
    x = torch.randn(shape, generator=g).to(act).to(cuda).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(c, 1, K, K, generator=g) / K).to(dt).to(cuda)
    b = torch.randn(c, generator=g).to(dt).to(cuda)
    dy = torch.randn(shape, generator=g).to(dt).to(cuda).contiguous(memory_format=torch.channels_last)
    return x, w, b, dy


def _run(x, w, b, dy):
    nat = ops.native()
    y = nat.dwconv_fwd(x, w, b)
    dx = nat.dwconv_dgrad(dy, w, x.dtype == torch.float32)
    dw, db = nat.dwconv_wgrad(dy, x, w.shape[2], KIND[w.dtype])
    return y, dx, dw, db


def _within(out, ref, u, slack, what):
    err = (out.double().cpu() - ref).abs()
    bound = u * ref.abs() + slack
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max err/bound {worst:.3f}")
    assert out.shape == ref.shape and bool((err <= bound).all()), (what, err.max().item(), worst)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("act_f32", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [3, 7])
def test_three_passes_against_fp64(cuda, K, dt, act_f32, shape):
    shp = SHAPES[shape](ops.native().dwconv_tiles()[0])
    act = torch.float32 if act_f32 else dt
    x, w, b, dy = _inputs(shp, K, dt, act, cuda)
    y, dx, dw, db = _run(x, w, b, dy)
    assert y.dtype == dt and dx.dtype == act and dw.dtype == dt and db.dtype == dt
    assert y.is_contiguous(memory_format=torch.channels_last) and dx.is_contiguous(memory_format=torch.channels_last)
    x16 = x.to(dt)
    ry, rdx, rdw, rdb = _ref(x16, w, b, dy)
    ay, adx, adw, adb = _ref(x16.abs(), w.abs(), b.abs(), dy.abs())   # |x| (*) |w| + |b| and its kin
    e = 2.0 ** -24
    P = shp[0] * shp[2] * shp[3]
    _within(y, ry, U[dt], (K * K + 2) * e * ay, "y")
    _within(dx, rdx, U[act], (K * K + 2) * e * adx, "dx")
    _within(dw, rdw, U[dt], (P + 2) * e * adw, "dw")
    _within(db, rdb, U[dt], (P + 2) * e * adb, "db")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_fp32_activations_round_like_the_cast(cuda, dt):
    T = ops.native().dwconv_tiles()[0]
    x, w, b, dy = _inputs(SHAPES["edges"](T), 7, dt, torch.float32, cuda, seed=1)
    y32, dx32, dw32, db32 = _run(x, w, b, dy)
    y16, dx16, dw16, db16 = _run(x.to(dt), w, b, dy)
    assert torch.equal(y32, y16) and torch.equal(dw32, dw16) and torch.equal(db32, db16)
    assert torch.equal(dx32.to(dt), dx16)


def test_backward_weight_is_deterministic(cuda):
    T = ops.native().dwconv_tiles()[0]
    x, w, b, dy = _inputs(SHAPES["exact"](T), 7, torch.bfloat16, torch.float32, cuda, seed=2)
    (dw1, db1), (dw2, db2) = (ops.native().dwconv_wgrad(dy, x, 7, 0) for _ in range(2))
    assert torch.equal(dw1, dw2) and torch.equal(db1, db2)


def test_convnext_routes_depthwise_convs_to_the_native_kernels(cuda, monkeypatch):
    """One bf16-autocast forward of ConvNeXt-T (32 px, batch 4) through the native engine's model:
    18 depthwise convs take the native kernels, none with the switch off, and the native logits are
    no further from the fp32 forward than twice the F.conv2d route's (+1e-6): the two routes
    differ only in where each depthwise output is rounded."""
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
    err = {}
    with torch.no_grad():
        ref = base(x).double()
        for route, calls in (("native", 18), ("stock", 0)):
            monkeypatch.setattr(dwconv, "ENABLED", route == "native")
            monkeypatch.setattr(dwconv, "CALLS", 0)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = tr.module(x)
            assert dwconv.CALLS == calls, (route, dwconv.CALLS)
            err[route] = (logits.double() - ref).abs().max().item()
    print("max |logits - fp32|:", err)
    assert err["native"] <= 2 * err["stock"] + 1e-6, err
