"""The split-bf16 mode of the fp32 convolutions (csrc/kernels/conv_f32_kernels.hip SPLIT = true,
ops/conv_f32.py ``conv2d(..., mode="split-bf16")``) on the GPU: the kernels against the contract
in plain torch (ops/reference.py ``conv2d_split_bf16``), bitwise determinism, exactness under
power-of-two scaling, non-finite inputs, the ``--fp32-conv split-bf16`` routing of the native
engine, and the accuracy of a whole ResNet-18 step."""
import pytest
import torch
import torch.nn.functional as F

from test_conv_f32_split import SHAPES, fp64_conv, make_case, rel

pytestmark = pytest.mark.gpu

CL = torch.channels_last
SPLIT_K = (64, 512, 2, 2, 512, 3, 1, 1)
NARROW = (3, 12, 9, 7, 20, 3, 1, 0)


def _gpu_case(shape, cuda):
    x, w, dy = make_case(shape, cuda)
    return (x.contiguous(memory_format=CL).requires_grad_(True), w.contiguous(memory_format=CL).requires_grad_(True),
            dy.contiguous(memory_format=CL))


def _run(x, w, dy, stride, pad, mode):
    from distributed_pytorch_training_amd.ops import conv_f32
    y = conv_f32.conv2d(x, w, stride, pad, mode=mode)
    dx, dw = torch.autograd.grad(y, (x, w), dy)
    return y.detach(), dx, dw


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_bf16_matches_the_contract(cuda, shape):
    """y, dx and dw against the contract computed in fp64 from identically split operands (what is
    left is the kernels' fp32 accumulation: the exact-mode test's 2e-6) and against the plain
    fp64 convolution (the contract's own 4.5e-6 error: 1e-5).  A missing term is 1.7e-3 away from
    the contract, a truncated hi 1.3e-5, a misplaced K group O(1)."""
    from distributed_pytorch_training_amd.ops import reference
    st, p = shape[6], shape[7]
    x, w, dy = _gpu_case(shape, cuda)
    y, dx, dw = _run(x, w, dy, st, p, "split-bf16")
    assert y.dtype == torch.float32 and y.is_contiguous(memory_format=CL)
    cy = reference.conv2d_split_bf16(x, w, st, p)
    cdx, cdw = reference.conv2d_split_bf16_grads(x, w, dy, st, p)
    ry, rdx, rdw = fp64_conv(x, w, dy, st, p)
    assert y.shape == cy.shape and dx.shape == cdx.shape and dw.shape == cdw.shape
    for name, got, contract, exact in (("y", y, cy, ry), ("dx", dx, cdx, rdx), ("dw", dw, cdw, rdw)):
        ec, ee = rel(got, contract), rel(got, exact)
        print(f"{name}: against the contract {ec:.3e}, against fp64 {ee:.3e}")
        assert ec < 2e-6, (name, ec)
        assert ee < 1e-5, (name, ee)


def test_split_bf16_is_bitwise_deterministic_and_shares_no_state_with_exact(cuda):
    x, w, dy = _gpu_case(SPLIT_K, cuda)
    before = _run(x, w, dy, 1, 1, "exact")
    outs = [_run(x, w, dy, 1, 1, "split-bf16") for _ in range(3)]
    after = _run(x, w, dy, 1, 1, "exact")
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert torch.equal(a, b)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert not torch.equal(before[0], outs[0][0])    # the two modes are different arithmetic


@pytest.mark.parametrize("shape", [NARROW, SPLIT_K], ids=lambda s: "x".join(map(str, s)))
def test_split_bf16_is_exact_under_power_of_two_scaling(cuda, shape):
    """x * 2^40 and w * 2^-40: the split commutes with a power of two and so do the MFMA's products
    and sums (no overflow or denormal in range), so y is the same bits; dx and dw, scaled back."""
    st, p = shape[6], shape[7]
    x, w, dy = _gpu_case(shape, cuda)
    y, dx, dw = _run(x, w, dy, st, p, "split-bf16")
    xs = (x.detach() * 2.0 ** 40).requires_grad_(True)
    ws = (w.detach() * 2.0 ** -40).requires_grad_(True)
    ys, dxs, dws = _run(xs, ws, dy, st, p, "split-bf16")
    assert torch.equal(ys, y)
    assert torch.equal(dxs * 2.0 ** 40, dx)
    assert torch.equal(dws * 2.0 ** -40, dw)


def test_split_bf16_non_finite_input_reaches_exactly_its_window(cuda):
    n, c, h, w_, co, k, st, p = NARROW
    x, w, dy = _gpu_case(NARROW, cuda)
    from distributed_pytorch_training_amd.ops import conv_f32
    clean = conv_f32.conv2d(x, w, st, p, mode="split-bf16").detach()
    assert torch.isfinite(clean).all()
    xi = x.detach().clone()
    n0, c0, h0, w0 = 1, 5, 4, 3
    xi[n0, c0, h0, w0] = float("inf")
    y = conv_f32.conv2d(xi, w, st, p, mode="split-bf16").detach()
    # outputs (ho, wo) whose k x k window (stride 1, no padding) holds (h0, w0)
    hit = torch.zeros_like(clean, dtype=torch.bool)
    hit[n0, :, max(0, h0 - k + 1):h0 + 1, max(0, w0 - k + 1):w0 + 1] = True
    assert hit.sum().item() == co * k * k
    assert not torch.isfinite(y[hit]).any()
    assert torch.equal(y[~hit], clean[~hit])


def _args(extra):
    from distributed_pytorch_training_amd.config import parse_args
    return parse_args(["--dataset", "synthetic", "--image-size", "32", "--num-classes", "10", "--no-cuda-graph"]
                      + extra)


def test_fp32_conv_split_bf16_routes_every_conv_to_the_split_function(cuda, monkeypatch):
    from distributed_pytorch_training_amd.engine.trainer import Trainer
    from distributed_pytorch_training_amd.models import build_model
    from distributed_pytorch_training_amd.ops import conv_f32
    split_calls, exact_calls = [], []
    orig_split, orig_exact = conv_f32._ConvF32Split.forward, conv_f32._ConvF32.forward

    def spy_split(ctx, x, w, stride, pad):
        split_calls.append(tuple(w.shape))
        return orig_split(ctx, x, w, stride, pad)

    def spy_exact(ctx, x, w, stride, pad):
        exact_calls.append(tuple(w.shape))
        return orig_exact(ctx, x, w, stride, pad)

    monkeypatch.setattr(conv_f32._ConvF32Split, "forward", staticmethod(spy_split))
    monkeypatch.setattr(conv_f32._ConvF32, "forward", staticmethod(spy_exact))
    torch.manual_seed(0)
    model = build_model("resnet18", 10, cuda, image_size=32, channels_last=True)
    tr = Trainer(model, _args(["--fp32-conv", "split-bf16"]), 0, 1, cuda, log=lambda s: None)
    x = torch.randn(16, 3, 32, 32, device=cuda).contiguous(memory_format=CL)
    y = torch.randint(0, 10, (16,), device=cuda)
    _, loss = tr.train_step(x, y)
    torch.cuda.synchronize()
    assert len(split_calls) == 20 and len(exact_calls) == 0, (len(split_calls), len(exact_calls))
    assert torch.isfinite(loss).item()


def test_fp32_resnet18_step_split_bf16_gradient_error(cuda):
    """One fp32 ResNet-18 / 32 px step from one state and batch; the gradients of the native engine
    in exact mode (e_exact), of stock torch modules on MIOpen (e_stock) and of the native engine in
    split-bf16 mode (e_split) against an fp64 CPU model, relative L2 over all parameters.  The
    per-conv error ratio of the CPU emulation is about 22 (4.4e-6 / 2e-7) and ReLU-mask flips scale
    with it; the bound is that ratio with about 1.5x headroom:
    e_split <= 32 * max(e_exact, e_stock) + 1e-5.
    Measured on an MI355X: e_exact 3.74e-6, e_stock 9.43e-4, e_split 7.62e-3 (bound 3.0e-2).  The
    bound holds through e_stock; e_split / e_exact is about 2000, not 22: at this batch a 4.4e-6
    perturbation flips the ReLU mask of a handful of units and one flipped layer4 unit moves the
    gradient by ~1e-2, while exact mode's 2e-7 flips none (profiles/conv_f32_split.md)."""
    from distributed_pytorch_training_amd.engine.trainer import Trainer
    from distributed_pytorch_training_amd.models import build_model
    torch.manual_seed(0)
    ref = build_model("resnet18", 10, torch.device("cpu"), image_size=32).double()
    state = {k: v.float() for k, v in ref.state_dict().items()}
    g = torch.Generator().manual_seed(1)
    x = torch.randn(32, 3, 32, 32, generator=g)
    y = torch.randint(0, 10, (32,), generator=g)
    F.cross_entropy(ref(x.double()), y).backward()
    r = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])

    def native_error(choice):
        model = build_model("resnet18", 10, cuda, image_size=32, channels_last=True)
        model.load_state_dict(state)
        tr = Trainer(model, _args(["--lr", "0", "--fp32-conv", choice]), 0, 1, cuda, log=lambda s: None)
        tr.train_step(x.to(cuda).contiguous(memory_format=CL), y.to(cuda))
        torch.cuda.synchronize()
        pos = {id(p): i for i, p in enumerate(tr.ddp.arena.params)}
        ag = tr.ddp.averaged_grads()
        nat = torch.cat([ag[pos[id(p)]].double().cpu().reshape(-1) for p in model.parameters()])
        return ((nat - r).norm() / r.norm()).item()

    stock = build_model("resnet18", 10, cuda, image_size=32)
    stock.load_state_dict(state)
    F.cross_entropy(stock(x.to(cuda)), y.to(cuda)).backward()
    torch.cuda.synchronize()
    sto = torch.cat([p.grad.double().cpu().reshape(-1) for p in stock.parameters()])
    e_stock = ((sto - r).norm() / r.norm()).item()
    e_exact = native_error("exact")
    e_split = native_error("split-bf16")
    print(f"e_exact {e_exact:.3e}  e_stock {e_stock:.3e}  e_split {e_split:.3e}")
    assert e_split <= 32 * max(e_exact, e_stock) + 1e-5, (e_exact, e_stock, e_split)
