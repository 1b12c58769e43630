"""--optimizer lars / lamb end to end on one MI355X: the native engine (FusedLARS / FusedLAMB over the
arena) against the stock engine (--impl torch, the per-tensor classes of optim/stock.py)."""
import copy

import pytest
import torch

import trust_oracle as orc
from distributed_pytorch_training_amd import ops
from distributed_pytorch_training_amd.config import parse_args
from distributed_pytorch_training_amd.engine.trainer import Trainer
from distributed_pytorch_training_amd.models import build_model
from distributed_pytorch_training_amd.optim import LAMB, LARS, FusedLAMB, FusedLARS

pytestmark = pytest.mark.gpu


def _pair(cuda, model_name, extra, image=32, classes=10):
    torch.manual_seed(0)
    base = build_model(model_name, classes, cuda, image_size=image)
    a = parse_args(["--model", model_name, "--dataset", "synthetic", "--no-channels-last", "--no-cuda-graph", *extra])
    b = parse_args(["--model", model_name, "--dataset", "synthetic", "--impl", "torch", *extra])
    return (Trainer(copy.deepcopy(base), a, 0, 1, cuda, log=lambda s: None),
            Trainer(copy.deepcopy(base), b, 0, 1, cuda, log=lambda s: None))


@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_native_matches_torch_fp32(cuda, opt):
    """ResNet-18, 32 px, batch 16, three fp32 steps.  The bounds are those of
    test_engine_gpu.py::test_native_matches_torch_fp32: LARS takes the SGD branch (each parameter's
    update within 1 % of the stock update's norm; elementwise 1e-3 or 5 % of the update's largest
    element), LAMB the Adam branch (elementwise 4e-3)."""
    lr = "0.1" if opt == "lars" else "1e-3"
    nat, ref = _pair(cuda, "resnet18", ["--optimizer", opt, "--lr", lr])
    assert type(nat.optimizer) is (FusedLARS if opt == "lars" else FusedLAMB)
    assert type(ref.optimizer) is (LARS if opt == "lars" else LAMB)
    torch.backends.cudnn.deterministic = True
    p0 = [p.detach().clone() for p in ref.module.parameters()]
    g = torch.Generator(device=cuda).manual_seed(1)
    for _ in range(3):
        x = torch.randn(16, 3, 32, 32, device=cuda, generator=g)
        y = torch.randint(0, 10, (16,), device=cuda, generator=g)
        nat.train_step(x, y)
        ref.train_step(x, y)
    worst = 0.0
    for (n, p), (_, q), w0 in zip(nat.module.named_parameters(), ref.module.named_parameters(), p0):
        du_ref = (q - w0).double()
        assert du_ref.norm().item() > 0, f"{n} did not move"
        if opt == "lars":
            rel = ((p - q).double().norm() / du_ref.norm().clamp_min(1e-12)).item()
            worst = max(worst, rel)
            assert rel < 1e-2, f"{n}: |native-torch|/|torch update| = {rel:.3e}"
            atol = max(1e-3, 0.05 * du_ref.abs().max().item())
        else:
            worst = max(worst, (p - q).abs().max().item())
            atol = 4e-3
        torch.testing.assert_close(p, q, rtol=2e-3, atol=atol, msg=lambda m, n=n: f"{n}: {m}")
    print(f"{opt}: worst {'relative update difference' if opt == 'lars' else 'elementwise difference'} {worst:.3e}")
    # 1-D parameters are excluded from the trust ratio, everything else is adapted
    for r, p in zip(nat.optimizer.trust_ratios.tolist(), nat.ddp.arena.params):
        assert (r == 1.0) == (p.ndim <= 1)


@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_amp_bf16_step_and_skipped_inf(cuda, opt):
    nat, ref = _pair(cuda, "resnet18", ["--optimizer", opt, "--amp", "--amp-dtype", "bf16"])
    x = torch.randn(16, 3, 32, 32, device=cuda)
    y = torch.randint(0, 10, (16,), device=cuda)
    nat.train_step(x, y)
    ref.train_step(x, y)
    assert nat.scaler.get_scale() == ref.scaler.get_scale() == 65536.0
    assert nat.optimizer.steps_taken.item() == 1.0
    if nat.ddp.shadow_flat is not None:
        assert torch.equal(nat.ddp.shadow_flat, nat.ddp.arena.param_flat.to(nat.ddp.shadow_flat.dtype))
    # inject a non-finite gradient: the step must be skipped and the scale backed off
    before = [t.clone() for t in (nat.ddp.arena.param_flat, *nat.optimizer.arena_state())]
    with torch.no_grad():
        nat.ddp.arena.grad_flat[10] = float("inf")
    nat.optimizer.step(nat.scaler, host_factor=1.0, grads_checked=False)
    torch.cuda.synchronize()
    for a, b in zip(before, (nat.ddp.arena.param_flat, *nat.optimizer.arena_state())):
        assert torch.equal(a, b)
    assert nat.scaler.get_scale() == 32768.0
    assert nat.scaler.found_inf.item() == 0.0 and nat.optimizer.steps_taken.item() == 1.0
    assert torch.count_nonzero(nat.ddp.arena.grad_flat) == 0


class UseOrderDiffers(torch.nn.Module):
    """Defined head first, used head last: the gradient-ready order is not the reverse of the
    definition order, so the first backward re-lays the arena."""

    def __init__(self):
        super().__init__()
        self.head = torch.nn.Linear(96, 10)
        self.conv = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(8)
        self.mid = torch.nn.Linear(8 * 16 * 16, 96)     # 196,608 weights: 48 chunks

    def forward(self, x):
        x = torch.nn.functional.max_pool2d(torch.relu(self.bn(self.conv(x))), 2)
        return self.head(torch.relu(self.mid(x.flatten(1))))


@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_table_is_rebuilt_after_relayout(cuda, opt):
    torch.manual_seed(0)
    model = UseOrderDiffers().to(cuda)
    args = parse_args(["--dataset", "synthetic", "--no-channels-last", "--no-cuda-graph", "--optimizer", opt,
                       "--lr", "0.1", "--trust-coefficient", "0.02", "--weight-decay", "1e-3"])
    tr = Trainer(model, args, 0, 1, cuda, log=lambda s: None)
    tr.ddp.rebuild_buckets = True           # a 1-rank run does not rebuild by itself (no peers)
    arena, o = tr.ddp.arena, tr.optimizer
    o.trust_ratios                           # a table for the first layout exists
    first, names0, offsets0 = o._table, list(arena.names), list(arena.offsets)
    g = torch.Generator(device=cuda).manual_seed(1)
    for _ in range(2):
        tr.train_step(torch.randn(16, 3, 32, 32, device=cuda, generator=g),
                      torch.randint(0, 10, (16,), device=cuda, generator=g))
    assert tr.ddp._rebuilt and arena.names != names0 and arena.offsets != offsets0
    table = o._table
    assert table is not first and table.offsets == arena.offsets
    assert table.numels == [p.numel() for p in arena.params]
    assert table.flags == [3 if p.ndim > 1 else 0 for p in arena.params]
    # one more optimizer step on known gradients: ratios against norms torch computes on the views
    flat = torch.zeros_like(arena.grad_flat)
    for v in arena.views(flat):
        v.copy_(torch.randn(v.shape, device=cuda, generator=g) * 0.01)
    arena.grad_flat.copy_(flat)
    p_views = [v.detach().double().clone() for v in arena.views(arena.param_flat)]
    g_views = [v.double().clone() for v in arena.views(flat)]
    state = [s.clone() for s in o.arena_state()]
    t = int(o.steps_taken.item()) + 1
    o.step(None, host_factor=1.0)
    got = o.trust_ratios.cpu().double().tolist()
    C = ops.trust_chunk()
    eta, wd = orc.f32(0.02), orc.f32(1e-3)
    for i, (p, gr, r) in enumerate(zip(p_views, g_views, got)):
        if p.ndim <= 1:
            assert r == 1.0, arena.names[i]
            continue
        wn = p.norm().item()
        if opt == "lars":
            want, bound = eta * wn / (gr.norm().item() + wd * wn), orc.lars_ratio_bound(p.numel(), C)
        else:
            # u from the moments the kernel stored (what its own norm was taken over)
            _, _, _, bc1, bc2 = orc.lamb_coefficients(0.9, 0.999, t)
            m, v = (arena.views(s)[i].double() for s in o.arena_state())
            assert not torch.equal(m, arena.views(state[0])[i].double())
            u, mag = orc.lamb_direction(p, m, v, bc1=bc1, bc2=bc2, eps=orc.f32(1e-8), wd_i=wd)
            want = wn / u.norm().item()
            bound = orc.lamb_ratio_bound(p.numel(), C, (mag.norm() / u.norm()).item())
        print(f"{arena.names[i]}: ratio {r:.9g} torch {want:.9g} rel.err {abs(r - want) / want:.3g} bound {bound:.3g}")
        assert abs(r - want) <= bound * want, (arena.names[i], r, want, bound)
