"""CPU path of gelu_grn16 (ops/convnext.py) and the ConvNeXt V2 model zoo entries."""
import torch
import torch.nn.functional as F

from distributed_pytorch_training_amd.models import build_model, count_params
from distributed_pytorch_training_amd.ops import convnext as cnx


def test_cpu_path_equals_the_official_formula_in_fp64():
    g = torch.Generator().manual_seed(0)
    N, H, W, D = 2, 3, 5, 24
    u = torch.randn(N, H, W, D, generator=g, dtype=torch.float64)
    b1, gamma, beta = (torch.randn(D, generator=g, dtype=torch.float64) for _ in range(3))
    dout = torch.randn(N, H, W, D, generator=g, dtype=torch.float64)
    leaves = [t.requires_grad_(True) for t in (u, b1, gamma, beta)]

    x = F.gelu(u + b1)                                            # the official GRN.forward on [N, H, W, D]
    Gx = torch.linalg.vector_norm(x, ord=2, dim=(1, 2), keepdim=True)
    want = gamma * (x * (Gx / (Gx.mean(dim=-1, keepdim=True) + 1e-6))) + beta + x
    got = cnx.gelu_grn16(u, b1, gamma, beta, H * W)
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=1e-13, atol=1e-13)
    for a, b in zip(torch.autograd.grad(got, leaves, dout), torch.autograd.grad(want, leaves, dout)):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)


def test_convnextv2_tiny_parameters_and_gradients():
    m = build_model("convnextv2_tiny", 1000)
    assert count_params(m) == 28_635_496
    sd = m.state_dict()
    assert tuple(sd["features.1.0.grn.gamma"].shape) == (1, 1, 1, 384) and "features.7.2.pwconv2.bias" in sd
    assert not any("layer_scale" in k for k in sd)
    assert all(bool((v == 0).all()) for k, v in sd.items() if ".grn." in k)
    m = build_model("convnextv2_tiny", 10, channels_last=True)
    y = m(torch.randn(2, 3, 64, 64).contiguous(memory_format=torch.channels_last))
    assert y.shape == (2, 10)
    y.sum().backward()
    assert all(p.grad is not None for p in m.parameters())
