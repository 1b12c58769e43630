"""The split-bf16 fp32 convolution mode without a GPU: its plain-torch contract
(ops/reference.py ``conv2d_split_bf16`` / ``conv2d_split_bf16_grads``) against an fp64 convolution
and against a 10-bit-mantissa (TF32-like) convolution, and the ``--fp32-conv`` flag down to the
per-conv routing of ``set_conv_routing``."""
import pytest
import torch
import torch.nn.functional as F

# (N, C, H, W, Co, k, stride, pad): tests/test_conv_f32_gpu.py SHAPES
SHAPES = [
    (8, 64, 8, 8, 64, 3, 1, 1),
    (8, 64, 8, 8, 128, 3, 2, 1),
    (8, 64, 8, 8, 128, 1, 2, 0),
    (8, 256, 2, 2, 512, 3, 2, 1),
    (8, 512, 1, 1, 512, 3, 1, 1),
    (4, 3, 32, 32, 64, 7, 2, 3),
    (2, 64, 14, 14, 256, 1, 1, 0),
    (2, 256, 14, 14, 64, 1, 1, 0),
    (2, 128, 15, 13, 96, 3, 2, 1),
    (3, 12, 9, 7, 20, 3, 1, 0),
    (2, 36, 11, 11, 44, 5, 2, 2),
    (64, 512, 2, 2, 512, 3, 1, 1),
]


def make_case(shape, device="cpu"):
    """x, w, dy of the exact-mode test's data recipe (randn, weights / sqrt(K), seed sum(shape))."""
    n, c, h, w_, co, k, st, p = shape
    g = torch.Generator(device=device).manual_seed(sum(shape))
    x = torch.randn(n, c, h, w_, device=device, generator=g)
    w = torch.randn(co, c, k, k, device=device, generator=g) / (c * k * k) ** 0.5
    ho, wo = (h + 2 * p - k) // st + 1, (w_ + 2 * p - k) // st + 1
    dy = torch.randn(n, co, ho, wo, device=device, generator=g)
    return x, w, dy


def fp64_conv(x, w, dy, stride, pad):
    xd = x.detach().double().cpu().requires_grad_(True)
    wd = w.detach().double().cpu().requires_grad_(True)
    y = F.conv2d(xd, wd, stride=stride, padding=pad)
    dx, dw = torch.autograd.grad(y, (xd, wd), dy.detach().double().cpu())
    return y.detach(), dx, dw


def rel(a, b):
    return ((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-30)).item()


def _round_mantissa10(v):
    """fp32 rounded to a 10-bit mantissa, nearest even (what a TF32 matrix core reads)."""
    u = v.detach().float().cpu().contiguous().view(torch.int32)
    u = (u + 0xFFF + ((u >> 13) & 1)) & ~0x1FFF
    return u.view(torch.float32)


def test_mantissa_rounding_helper():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -10), 0.0])
    assert _round_mantissa10(v).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -10), 0.0]


def test_split_bf16_is_hi_plus_lo():
    from distributed_pytorch_training_amd.ops import reference
    v = torch.randn(4096, generator=torch.Generator().manual_seed(0))
    hi, lo = reference.split_bf16(v)
    assert torch.equal(hi.float().to(torch.bfloat16).double(), hi)      # both are bf16 values
    assert torch.equal(lo.float().to(torch.bfloat16).double(), lo)
    assert torch.equal(hi, v.to(torch.bfloat16).double())               # hi is the nearest bf16
    # 8 + 8 mantissa bits (and lo's sign): the remainder is below 2^-17 of the value
    assert ((v.double() - hi - lo).abs() <= v.double().abs() * 2.0 ** -17).all()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_split_bf16_against_fp64_and_tf32(shape):
    from distributed_pytorch_training_amd.ops import reference
    st, p = shape[6], shape[7]
    x, w, dy = make_case(shape)
    ry, rdx, rdw = fp64_conv(x, w, dy, st, p)
    y = reference.conv2d_split_bf16(x, w, st, p)
    dx, dw = reference.conv2d_split_bf16_grads(x, w, dy, st, p)
    assert y.shape == ry.shape and dx.shape == rdx.shape and dw.shape == rdw.shape
    xt, wt, dyt = _round_mantissa10(x), _round_mantissa10(w), _round_mantissa10(dy)
    ty = fp64_conv(xt, wt, dyt, st, p)[0]
    tdx = fp64_conv(x, wt, dyt, st, p)[1]      # dx is linear in (dy, w): only those are rounded
    tdw = fp64_conv(xt, w, dyt, st, p)[2]      # dw in (dy, x)
    for name, got, want, tf in (("y", y, ry, ty), ("dx", dx, rdx, tdx), ("dw", dw, rdw, tdw)):
        e, et = rel(got, want), rel(tf, want)
        print(f"{name}: split-bf16 {e:.3e}  10-bit mantissa {et:.3e}  ratio {et / e:.1f}")
        assert e < 1e-5, (name, e)
        assert 16 * e <= et, (name, e, et)


# ---- the flag ---------------------------------------------------------------------------------
BASE = ["--dataset", "synthetic", "--image-size", "32", "--num-classes", "10"]


def _routing(model):
    from distributed_pytorch_training_amd.ops import conv_f32
    return [(m.dpt_native_conv, m.dpt_native_conv_f32,
             conv_f32.MODE if m.dpt_conv_f32_mode is None else m.dpt_conv_f32_mode)
            for m in model.modules() if isinstance(m, torch.nn.Conv2d)]


def _routed_resnet18(argv):
    from distributed_pytorch_training_amd.config import fp32_conv_routing, parse_args
    from distributed_pytorch_training_amd.models import build_model
    from distributed_pytorch_training_amd.models.layers import set_conv_routing
    args = parse_args(BASE + argv)
    model = build_model("resnet18", 10, torch.device("cpu"), image_size=32)
    f32, mode = fp32_conv_routing(args)
    set_conv_routing(model, True, None, f32, mode)
    return model


def test_fp32_conv_flag_parses():
    from distributed_pytorch_training_amd.config import fp32_conv_routing, parse_args
    assert parse_args(BASE).fp32_conv is None
    assert fp32_conv_routing(parse_args(BASE)) == (None, None)
    for choice in ("miopen", "exact", "split-bf16"):
        assert parse_args(BASE + ["--fp32-conv", choice]).fp32_conv == choice
    assert fp32_conv_routing(parse_args(BASE + ["--fp32-conv", "miopen"])) == (False, None)
    assert fp32_conv_routing(parse_args(BASE + ["--fp32-conv", "split-bf16"])) == (True, "split-bf16")
    assert fp32_conv_routing(parse_args(BASE + ["--native-conv-fp32"])) == (True, None)
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--fp32-conv", "tf32"])


@pytest.mark.parametrize("choice", ["split-bf16", "miopen"])
def test_native_conv_fp32_contradicting_fp32_conv_exits(choice):
    from distributed_pytorch_training_amd.config import parse_args
    with pytest.raises(SystemExit):
        parse_args(BASE + ["--native-conv-fp32", "--fp32-conv", choice])
    assert parse_args(BASE + ["--native-conv-fp32", "--fp32-conv", "exact"]).fp32_conv == "exact"


def test_fp32_conv_exact_routes_like_native_conv_fp32(monkeypatch):
    from distributed_pytorch_training_amd.ops import conv_f32
    monkeypatch.setattr(conv_f32, "MODE", "exact")      # the default, whatever the environment says
    a = _routing(_routed_resnet18(["--fp32-conv", "exact"]))
    b = _routing(_routed_resnet18(["--native-conv-fp32"]))
    assert len(a) == 20 and a == b
    assert all(r == (True, True, "exact") for r in a)


def test_fp32_conv_split_bf16_is_per_model():
    split = _routed_resnet18(["--fp32-conv", "split-bf16"])
    convs = [m for m in split.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 20
    assert all(m.dpt_conv_f32_mode == "split-bf16" and m.dpt_native_conv_f32 is True for m in convs)
    other = _routed_resnet18([])                        # a second model, built without the flag
    assert all(m.dpt_conv_f32_mode is None and m.dpt_native_conv_f32 is None
               for m in other.modules() if isinstance(m, torch.nn.Conv2d))
    assert all(m.dpt_conv_f32_mode == "split-bf16" for m in convs)
    miopen = _routed_resnet18(["--fp32-conv", "miopen"])
    assert all(m.dpt_native_conv_f32 is False for m in miopen.modules() if isinstance(m, torch.nn.Conv2d))


def test_conv2d_rejects_an_unknown_mode():
    from distributed_pytorch_training_amd.ops import conv_f32
    from distributed_pytorch_training_amd.models.layers import set_conv_routing
    with pytest.raises(ValueError):
        conv_f32.conv2d(torch.zeros(1, 4, 4, 4), torch.zeros(4, 4, 1, 1), 1, 0, mode="tf32")
    with pytest.raises(ValueError):
        set_conv_routing(torch.nn.Conv2d(4, 4, 1), f32_mode="tf32")
