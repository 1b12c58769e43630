"""ops/patchconv.py without a GPU: the CPU path is ``F.conv2d``, and ``supported`` is a GPU-only route."""
import pytest
import torch
import torch.nn.functional as F

from distributed_pytorch_training_amd.ops import patchconv


@pytest.mark.parametrize("k, c, cout, h, w_", [(2, 32, 64, 5, 6), (4, 3, 96, 9, 14)])
def test_cpu_path_is_conv2d_forward_and_backward(k, c, cout, h, w_):
    g = torch.Generator().manual_seed(0)
    x, w, b = torch.randn(2, c, h, w_, generator=g), torch.randn(cout, c, k, k, generator=g), torch.randn(cout, generator=g)
    got, want = [], []
    for fn, out in ((patchconv.patch_conv2d, got), (lambda x, w, b: F.conv2d(x, w, b, stride=k), want)):
        leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
        y = fn(*leaves)
        out += [y.detach(), *torch.autograd.grad(y.square().sum(), leaves)]
    assert all(torch.equal(a, b_) for a, b_ in zip(got, want))
    assert torch.equal(patchconv.reference_patchconv(x, w, b), want[0])


@pytest.mark.parametrize("stride, padding, groups, wshape", [
    ((2, 2), (0, 0), 1, (64, 32, 2, 2)),    # a CPU tensor
    ((2, 2), (1, 1), 1, (64, 32, 2, 2)),    # padding
    ((1, 1), (0, 0), 1, (64, 32, 2, 2)),    # kernel != stride
    ((2, 2), (0, 0), 2, (64, 16, 2, 2)),    # grouped
])
def test_supported_is_false_off_the_route(stride, padding, groups, wshape):
    x = torch.randn(1, 32, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    w, b = torch.randn(wshape).bfloat16(), torch.zeros(wshape[0], dtype=torch.bfloat16)
    assert not patchconv.supported(x, w, b, stride, padding, (1, 1), groups)
