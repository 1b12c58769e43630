"""Block-tail BN apply fused into the next block's 1x1 forward conv (ops/bn.py TAIL_CONV1_FUSE,
csrc/kernels/tail_conv1_kernels.hip).

The fused kernel redoes the apply pass and the unsplit forward conv operation for operation, so every
comparison is bit for bit on the int16 view (NaN payloads and signed zeros count).  The reference is
``bn_apply`` / ``bn_apply_aff`` with ``mask_out`` followed by ``conv_fwd(stats=True)`` with
``conv_set_splitk(0)``; at block and model level, the same network with the switch off.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from distributed_pytorch_training_amd import ops
from distributed_pytorch_training_amd.models import layers
from distributed_pytorch_training_amd.models.resnet import Bottleneck, link_tail_consumers
from distributed_pytorch_training_amd.ops import bn as fused_bn
from distributed_pytorch_training_amd.ops import conv as native_conv

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _bits(t: torch.Tensor) -> torch.Tensor:
    if t.dtype in (torch.uint8, torch.int64):
        return t.contiguous()
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(name, a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, name
    assert torch.equal(_bits(a), _bits(b)), f"{name}: {(_bits(a) != _bits(b)).sum().item()} elements differ"


def _rand(shape, dtype, dev, g, scale=1.0):
    t = (torch.randn(shape, device=dev, generator=g) * scale).to(dtype)
    return t.contiguous(memory_format=CL) if len(shape) == 4 else t


@pytest.fixture
def unsplit():
    """The reference forward conv is the unsplit one; small shapes would otherwise count as split
    under graph capture, which the fused path refuses."""
    C_ = ops.native()
    C_.conv_set_splitk(0)
    yield
    C_.conv_set_splitk(1)


def _operands(dev, dtype, nhw, cin, cout, aff, seed):
    n, h, w_ = nhw
    g = torch.Generator(device=dev).manual_seed(seed)
    x3 = _rand((n, cin, h, w_), dtype, dev, g)
    r = _rand((n, cin, h, w_), dtype, dev, g)
    coef = torch.cat([torch.rand(cin, device=dev, generator=g) + 0.5, torch.randn(cin, device=dev, generator=g) * 0.3])
    coef2 = (torch.cat([torch.rand(cin, device=dev, generator=g) + 0.5,
                        torch.randn(cin, device=dev, generator=g) * 0.3]) if aff else None)
    w = _rand((cout, cin, 1, 1), dtype, dev, g, (2.0 / cin) ** 0.5)
    return x3, r, coef, coef2, w


def _reference(x3, r, coef, coef2, w):
    C_ = ops.native()
    cin = x3.shape[1]
    m = x3.numel() // cin
    mask = torch.zeros((m, cin // 8), dtype=torch.uint8, device=x3.device)
    if coef2 is None:
        y = C_.bn_apply(x3, r, coef[:cin].contiguous(), coef[cin:].contiguous(), True, mask_out=mask)
    else:
        y = C_.bn_apply_aff(x3, r, coef, coef2, mask_out=mask)
    x1, ps, pq = C_.conv_fwd(y, w, 1, 0, True, 0, 0)
    return {"y": y, "mask": mask, "x1": x1, "psum": ps, "psq": pq}


def _fused(x3, r, coef, coef2, w):
    C_ = ops.native()
    cin = x3.shape[1]
    m = x3.numel() // cin
    # poisoned outputs: every element must be written
    y = torch.full_like(x3, float("nan"))
    mask = torch.full((m, cin // 8), 0xA5, dtype=torch.uint8, device=x3.device)
    x1, ps, pq = C_.conv1x1_tail_fwd(x3, r, coef, coef2, w, y, mask)
    return {"y": y, "mask": mask, "x1": x1, "psum": ps, "psq": pq}


# ---- kernel level ------------------------------------------------------------------------------
@pytest.mark.parametrize("aff", [False, True], ids=["res", "two-bn"])
@pytest.mark.parametrize("cout", [64, 128])
@pytest.mark.parametrize("cin", [64, 256, 512])  # 1, 4 and 8 K-steps
@pytest.mark.parametrize("nhw", [(1, 5, 5), (3, 7, 7), (3, 10, 10)], ids=["m25", "m147", "m300"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fused_kernel_is_bitwise_apply_then_conv(cuda, unsplit, dtype, nhw, cin, cout, aff):
    """M = 25 (less than a tile), 147 (ragged second tile) and 300 (three tiles)."""
    ops_ = _operands(cuda, dtype, nhw, cin, cout, aff, 100 + cin + cout + nhw[1])
    ref, out = _reference(*ops_), _fused(*ops_)
    assert ref["x1"].float().abs().max() > 0 and ref["mask"].max() > 0
    for name in ref:
        _same(name, ref[name], out[name])


@pytest.mark.parametrize("aff", [False, True], ids=["res", "two-bn"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fused_kernel_special_values(cuda, unsplit, dtype, aff):
    """-0.0, +-inf, NaN and values that round to +-0 in x3 and the residual: the same bits out,
    NaN payloads and zero signs included."""
    x3, r, coef, coef2, w = _operands(cuda, dtype, (3, 7, 7), 256, 64, aff, 7)
    specials = [-0.0, 0.0, float("inf"), -float("inf"), float("nan")]
    views = []
    for t, shift in ((x3, 0), (r, 3)):
        flat = t.permute(0, 2, 3, 1).reshape(-1, 256)   # a view of the channels_last storage
        assert flat.data_ptr() == t.data_ptr()
        views.append(flat)
        for i, v in enumerate(specials):
            flat[(5 * i + shift) % flat.shape[0], (37 * i + shift) % 256] = v
            flat[-1 - i, (11 * i + shift) % 256] = v
    coef[5] = 0.0    # a = 0: 0 * inf = NaN where x3 is infinite
    coef[256 + 5] = -0.0
    # channel 9: x3 * a is far below the 16-bit type's smallest subnormal and b = 0, residual +-0:
    # the fp32 value is tiny and positive (or negative), the STORED value +0 - and so is its mask bit
    small, a9 = (1e-37, 1e-6) if dtype == torch.bfloat16 else (6e-8, 1e-3)
    coef[9], coef[256 + 9] = a9, 0.0
    if coef2 is not None:
        coef2[256 + 9] = 0.0
    views[0][0:40, 9], views[0][40:60, 9] = small, -small
    views[1][0:60, 9] = 0.0
    views[1][10:20, 9] = -0.0
    ref, out = _reference(x3, r, coef, coef2, w), _fused(x3, r, coef, coef2, w)
    assert torch.isnan(ref["y"].float()).any() and torch.isinf(ref["y"].float()).any()
    y9 = ref["y"].permute(0, 2, 3, 1).reshape(-1, 256)[0:60, 9]
    assert (y9 == 0).all() and (ref["mask"][0:60, 1] & 2 == 0).all()
    for name in ref:
        _same(name, ref[name], out[name])


class _Conv(nn.Module):
    """A bias-free conv with a 16-bit weight parameter (what the engine's shadow weights give the
    model's convs): the MFMA kernels where they support the shape, ATen elsewhere."""

    def __init__(self, cout, cin, k, stride, pad, dtype, g, dev="cuda"):
        super().__init__()
        w = torch.randn((cout, cin, k, k), device=dev, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        self.weight = nn.Parameter(w.to(dtype).contiguous(memory_format=CL))
        self.stride, self.pad = stride, pad

    def forward(self, x):
        if native_conv.supported(x, self.weight, (self.stride,) * 2, (self.pad,) * 2, (1, 1), 1):
            return native_conv.conv2d(x, self.weight, self.stride, self.pad, bn_stats=True)
        return F.conv2d(x, self.weight, None, self.stride, self.pad)


# ---- refusals ----------------------------------------------------------------------------------
_REFUSALS = {
    #            dtype           cin  cout k  stride splitk
    "cout256":  (torch.bfloat16, 256, 256, 1, 1, 0),
    "stride2":  (torch.bfloat16, 256, 64, 1, 2, 0),
    "3x3":      (torch.bfloat16, 256, 64, 3, 1, 0),
    "fp32":     (torch.float32, 256, 64, 1, 1, 0),
    "cin32":    (torch.bfloat16, 32, 64, 1, 1, 0),
    "split-k":  (torch.bfloat16, 256, 64, 1, 1, 1),   # 2 tiles x 4 K-steps: split under graph capture
}


@pytest.mark.parametrize("case", list(_REFUSALS))
def test_refused_shapes_raise_and_python_falls_back(cuda, case, monkeypatch):
    dtype, cin, cout, k, stride, splitk = _REFUSALS[case]
    C_ = ops.native()
    g = torch.Generator(device=cuda).manual_seed(31)
    n, h, w_ = 3, 8, 8
    x3 = _rand((n, cin, h, w_), dtype, cuda, g)
    r = _rand((n, cin, h, w_), dtype, cuda, g)
    conv = _Conv(cout, cin, k, stride, k // 2, dtype, g)
    coef = torch.cat([torch.rand(cin, device=cuda, generator=g) + 0.5, torch.randn(cin, device=cuda, generator=g)])
    C_.conv_set_splitk(splitk)
    try:
        if case == "split-k":
            assert C_.conv_fwd_splits(n * h * w_, cout, cin, True) > 1
        # the binding refuses, and writes nothing
        y = torch.full_like(x3, 7.0)
        mask = torch.full((n * h * w_, cin // 8), 0xA5, dtype=torch.uint8, device=cuda)
        with pytest.raises(RuntimeError):
            C_.conv1x1_tail_fwd(x3, r, coef, None, conv.weight.detach(), y, mask, stride, k // 2)
        torch.cuda.synchronize()
        assert (y == 7.0).all() and (mask == 0xA5).all()

        # the Python path: the tail with that consumer equals the tail without one, y is filled
        bn = layers.FusedBatchNorm2d(cin).to(cuda).train()

        def tail(consumer, force_defer):
            native_conv.reset_side_channels()
            b = copy.deepcopy(bn)
            if force_defer:
                # the shape pre-check says yes: the conv must decline at launch time
                real = fused_bn.native()

                class _Yes:
                    def __getattr__(self, name):
                        return (lambda *a: None) if name == "conv1x1_tail_refusal" else getattr(real, name)

                monkeypatch.setattr(fused_bn, "native", lambda: _Yes())
            xin = x3.detach().clone().requires_grad_(True)
            out = fused_bn.bn_act_train(xin, r, b.weight, b.bias, b.running_mean, b.running_var,
                                        b.num_batches_tracked, b.momentum, b.eps, True, pair=True, consumer=consumer)
            if force_defer:
                monkeypatch.undo()
            assert "_dpt_tail_pending" not in out[0].__dict__
            nxt = conv(out[0])
            return out[0].detach(), out[1].detach(), nxt.detach()

        if dtype == torch.float32:
            want = tail(None, False)
            got = tail(conv, False)
        else:
            want = tail(None, False)
            got = tail(conv, False)
            forced = tail(conv, True)
            for name, a, b in zip(("y", "y-identity", "conv"), want, forced):
                _same("forced " + name, a, b)
        for name, a, b in zip(("y", "y-identity", "conv"), want, got):
            _same(name, a, b)
        assert torch.isfinite(want[0].float()).all() and want[0].float().abs().max() > 0
    finally:
        C_.conv_set_splitk(1)


# ---- block level -------------------------------------------------------------------------------
def _three_blocks(dtype, dev):
    """64 -> (64) -> 256 with a downsample (two-BN tail, feeds a 256 -> 64 conv1), 256 -> (64) -> 256
    (plain tail, feeds the 256 -> 128 conv1 of a stride-2 block), 256 -> (128) -> 512 / stride 2."""
    g = torch.Generator(device=dev).manual_seed(7)
    ds0 = nn.Sequential(nn.Conv2d(64, 256, 1, 1, bias=False), nn.BatchNorm2d(256))
    ds2 = nn.Sequential(nn.Conv2d(256, 512, 1, 2, bias=False), nn.BatchNorm2d(512))
    net = nn.Sequential(Bottleneck(64, 64, 1, ds0), Bottleneck(256, 64), Bottleneck(256, 128, 2, ds2)).to(dev)
    for parent in list(net.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, nn.Conv2d):
                setattr(parent, name, _Conv(child.out_channels, child.in_channels, child.kernel_size[0],
                                            child.stride[0], child.padding[0], dtype, g))
    layers.fuse_batchnorm(net)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.copy_(torch.rand(m.weight.shape, device=dev, generator=g) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, device=dev, generator=g) - 0.5)
    link_tail_consumers([net])
    x = _rand((3, 64, 8, 8), dtype, dev, g)   # M = 192: a full and a ragged tile
    return net.train(), x


def _run_blocks(net0, x0, fuse, monkeypatch, variants=None):
    monkeypatch.setattr(fused_bn, "TAIL_CONV1_FUSE", fuse)
    native_conv.reset_side_channels()
    net = copy.deepcopy(net0)
    ys = []
    hooks = [b.register_forward_hook(lambda m, i, o: ys.append(o)) for b in net]
    if variants is not None:
        native_conv.profile_calls(True)
    x = x0.detach().clone().requires_grad_(True)
    try:
        y = net(x)
        gy = _rand(tuple(y[0].shape), y[0].dtype, x.device, torch.Generator(device=x.device).manual_seed(8))
        y[0].backward(gy)
    finally:
        if variants is not None:
            variants.extend(v for kind, _, v, _, _ in native_conv.take_profile() if kind == "fwd")
            native_conv.profile_calls(False)
        for h in hooks:
            h.remove()
    assert not native_conv._BNB_PARTIALS
    out = {"x.grad": x.grad}
    for i, o in enumerate(ys):
        assert isinstance(o, tuple) and "_dpt_tail_pending" not in o[0].__dict__
        out[f"y{i}.conv"], out[f"y{i}.identity"] = o[0].detach(), o[1].detach()
    out.update({n + ".grad": p.grad for n, p in net.named_parameters()})
    out.update({n: b.detach() for n, b in net.named_buffers()})
    return out


def _same_dicts(a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert a[name] is not None and b[name] is not None, name
        if a[name].is_floating_point():
            assert torch.isfinite(a[name].float()).all(), name
        _same(name, a[name], b[name])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_blocks_switch_on_is_bitwise_switch_off(cuda, unsplit, dtype, monkeypatch):
    net, x = _three_blocks(dtype, cuda)
    v_off, v_on = [], []
    off = _run_blocks(net, x, False, monkeypatch, v_off)
    on = _run_blocks(net, x, True, monkeypatch, v_on)
    assert v_off.count("tail-apply+stats") == 0
    assert v_on.count("tail-apply+stats") == 2 and len(v_on) == len(v_off)   # no conv ran twice
    assert any(k.endswith("num_batches_tracked") for k in off) and any(k.endswith("running_var") for k in off)
    _same_dicts(off, on)


@pytest.mark.parametrize("knob", ["BN_BWD_FUSE", "S2_COMPACT_DRES"])
def test_blocks_with_a_backward_fusion_off(cuda, unsplit, knob, monkeypatch):
    net, x = _three_blocks(torch.bfloat16, cuda)
    monkeypatch.setattr(native_conv, knob, False)
    v_on = []
    off = _run_blocks(net, x, False, monkeypatch)
    on = _run_blocks(net, x, True, monkeypatch, v_on)
    assert v_on.count("tail-apply+stats") == 2
    _same_dicts(off, on)


def test_blocks_under_the_default_split_policy_are_not_fused(cuda, monkeypatch):
    """M = 192 and four K-steps: the graph policy would split these convs, so nothing is fused and
    the results are the parent's in every mode."""
    net, x = _three_blocks(torch.bfloat16, cuda)
    v_on = []
    off = _run_blocks(net, x, False, monkeypatch)
    on = _run_blocks(net, x, True, monkeypatch, v_on)
    assert v_on.count("tail-apply+stats") == 0
    _same_dicts(off, on)


def test_blocks_captured_step_replays_like_eager(cuda, unsplit, monkeypatch):
    net0, x0 = _three_blocks(torch.bfloat16, cuda)
    monkeypatch.setattr(fused_bn, "TAIL_CONV1_FUSE", True)
    gy = None

    def step(net, x):
        nonlocal gy
        native_conv.reset_side_channels()
        y = net(x)
        if gy is None:
            gy = _rand(tuple(y[0].shape), y[0].dtype, x.device, torch.Generator(device=x.device).manual_seed(8))
        y[0].backward(gy)
        return [y[0].detach(), y[1].detach(), x.grad] + [p.grad for p in net.parameters()]

    eager = step(copy.deepcopy(net0), x0.detach().clone().requires_grad_(True))
    net = copy.deepcopy(net0)
    x = x0.detach().clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(copy.deepcopy(net0), x0.detach().clone().requires_grad_(True))   # warm the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    variants = []
    native_conv.profile_calls(False)
    g = torch.cuda.CUDAGraph()
    real = native_conv._tail_fwd
    monkeypatch.setattr(native_conv, "_tail_fwd",
                        lambda *a: (lambda o: (variants.append(o is not None), o)[1])(real(*a)))
    with torch.cuda.graph(g):
        out = step(net, x)
    g.replay()
    torch.cuda.synchronize()
    assert variants == [True, True]
    for i, (a, b) in enumerate(zip(eager, out)):
        _same(f"output {i}", a, b)


# ---- model level -------------------------------------------------------------------------------
def test_resnet50_step_on_is_bitwise_off(cuda, unsplit, monkeypatch):
    from distributed_pytorch_training_amd.config import parse_args
    from distributed_pytorch_training_amd.engine.trainer import Trainer
    from distributed_pytorch_training_amd.models import build_model

    batch, px = 2, 64
    torch.manual_seed(0)
    base = build_model("resnet50", 1000, cuda, image_size=px, channels_last=True)
    state = {k: v.detach().clone() for k, v in base.state_dict().items()}
    del base
    g = torch.Generator(device=cuda).manual_seed(1000)
    x = torch.randn(batch, 3, px, px, device=cuda, generator=g).contiguous(memory_format=CL)
    t = torch.randint(0, 1000, (batch,), device=cuda, generator=g)
    argv = ["--model", "resnet50", "--dataset", "synthetic", "--batch-size", str(batch), "--image-size", str(px),
            "--num-classes", "1000", "--channels-last", "--no-cuda-graph", "--lr", "0.1", "--momentum", "0.9",
            "--weight-decay", "5e-4", "--impl", "native", "--amp", "--amp-dtype", "bf16"]

    def run(fuse):
        monkeypatch.setattr(fused_bn, "TAIL_CONV1_FUSE", fuse)
        m = build_model("resnet50", 1000, cuda, image_size=px, channels_last=True)
        tr = Trainer(m, parse_args(argv), 0, 1, cuda, log=lambda s: None)
        tr.module.load_state_dict(state)
        tr.sync_weights()
        tr.model.train()
        native_conv.profile_calls(True)
        try:
            _, loss = tr.train_step(x, t)
            torch.cuda.synchronize()
            fused = sorted(key[:4] for kind, key, v, _, _ in native_conv.take_profile()
                           if kind == "fwd" and v == "tail-apply+stats")
        finally:
            native_conv.profile_calls(False)
        out = {"loss": loss.detach().clone(), "grads": tr.ddp.arena.grad_flat.detach().clone()}
        out.update({"p." + n: p.detach().clone() for n, p in tr.module.named_parameters()})
        out.update({"b." + n: b.detach().clone() for n, b in tr.module.named_buffers()})
        tr.close()
        return out, fused

    off, f_off = run(False)
    on, f_on = run(True)
    assert f_off == []
    # (Cin, H, W, Cout): layer1.1 / layer1.2 conv1, layer2.0 conv1, layer2.1-3 conv1 at 64 px
    assert f_on == sorted([(256, 16, 16, 64)] * 2 + [(256, 16, 16, 128)] + [(512, 8, 8, 128)] * 3)
    _same_dicts(off, on)
