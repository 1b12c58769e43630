"""ConvNeXt model zoo entries and the depthwise conv op's CPU path."""
import pytest
import torch
import torch.nn.functional as F

from distributed_pytorch_training_amd.models import build_model, count_params
from distributed_pytorch_training_amd.ops.dwconv import dwconv2d, reference_dwconv


def test_convnext_tiny_param_count_and_keys():
    m = build_model("convnext_tiny", 1000)
    assert count_params(m) == 28_589_128
    sd = m.state_dict()
    for k in ["features.0.0.weight", "features.1.0.block.0.weight", "features.1.0.layer_scale", "features.2.1.weight",
              "features.7.2.block.5.bias", "classifier.2.weight"]:
        assert k in sd, k
    assert tuple(sd["features.1.0.block.0.weight"].shape) == (96, 1, 7, 7)
    assert tuple(sd["features.1.0.layer_scale"].shape) == (96, 1, 1)
    assert torch.all(sd["features.1.0.layer_scale"] == 1e-6)


def test_forward_backward_channels_last():
    m = build_model("convnext_tiny", 10, channels_last=True)
    x = torch.randn(2, 3, 64, 64).contiguous(memory_format=torch.channels_last)
    y = m(x)
    assert y.shape == (2, 10)
    y.sum().backward()
    assert all(p.grad is not None for p in m.parameters())


@pytest.mark.parametrize("K", [3, 5, 7])
def test_reference_dwconv_is_grouped_conv2d(K):
    g = torch.Generator().manual_seed(K)
    x, w, b = torch.randn(2, 16, 9, 11, generator=g), torch.randn(16, 1, K, K, generator=g), torch.randn(16, generator=g)
    want = F.conv2d(x, w, b, stride=1, padding=(K - 1) // 2, groups=16)
    assert want.shape == x.shape
    assert torch.equal(reference_dwconv(x, w, b), want) and torch.equal(dwconv2d(x, w, b), want)


@pytest.mark.parametrize("name", ["convnext_tiny", "convnext_small", "convnext_base"])
def test_state_dict_round_trip_with_torchvision(name):
    tv = pytest.importorskip("torchvision")
    ours, theirs = build_model(name, 1000), getattr(tv.models, name)(weights=None)
    theirs.load_state_dict(ours.state_dict(), strict=True)
    ours.load_state_dict(theirs.state_dict(), strict=True)
