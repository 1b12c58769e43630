"""CPU paths of the ConvNeXt block ops (ops/convnext.py) and of set_native."""
import copy

import pytest
import torch
import torch.nn.functional as F

from distributed_pytorch_training_amd.ops import convnext as cnx


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_cpu_paths_equal_the_pytorch_composition(dt):
    g = torch.Generator().manual_seed(0)
    y = torch.randn(2, 3, 5, 96, generator=g)
    w, b, ls = (torch.randn(96, generator=g) for _ in range(3))
    h = cnx.channel_layer_norm16(y.to(dt), w, b, 1e-6, dt)
    assert h.dtype == dt and torch.equal(h, F.layer_norm(y.to(dt).float(), (96,), w, b, 1e-6).to(dt))
    z, b2 = torch.randn(2, 3, 5, 96, generator=g).to(dt), b.to(dt)
    out = cnx.scale_residual(y, z, b2, ls)
    assert out.dtype == torch.float32 and torch.equal(out, y + ls * (z.float() + b2.float()))


def test_set_native_leaves_a_cpu_model_unchanged():
    from distributed_pytorch_training_amd.models import build_model
    from distributed_pytorch_training_amd.models.convnext import set_native

    torch.manual_seed(0)
    m = build_model("convnext_tiny", 10)
    x = torch.randn(2, 3, 32, 32)
    with torch.no_grad():
        ref = m(x)
        sd = copy.deepcopy(m.state_dict())
        assert set_native(m) == 18 + 5          # blocks + stem, three downsample and classifier LayerNorms
        assert torch.equal(m(x), ref)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            a = m(x)
            set_native(m, False)
            assert torch.equal(m(x), a)
    assert list(m.state_dict()) == list(sd)
