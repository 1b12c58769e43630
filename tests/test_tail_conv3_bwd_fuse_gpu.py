"""Block-tail BN backward apply fused into conv3's backward-data (ops/conv.py TAIL_CONV3_BWD_FUSE,
csrc/kernels/tail_conv3_bwd_kernels.hip).

The fused kernel redoes the apply pass and the unsplit backward-data with its BNB epilogue operation
for operation, so every comparison is bit for bit on the int16 / int32 view (NaN payloads and signed
zeros count).  The reference is ``bn_bwd_partials`` / ``bn2_bwd_partials`` (from_dz) followed by
``conv_dgrad_bnstats`` with ``conv_set_splitk(0)``; at block and model level, the same network with
the switch off.
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
FUSED = "tail-bwd-apply+dgrad"


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
    """The reference backward-data is the unsplit one; small shapes would otherwise count as split
    under graph capture, which the fused path refuses."""
    C_ = ops.native()
    C_.conv_set_splitk(0)
    yield
    C_.conv_set_splitk(1)


# ---- kernel level ------------------------------------------------------------------------------
def _operands(dev, dtype, nhw, c4, c, two, seed):
    n, h, w_ = nhw
    g = torch.Generator(device=dev).manual_seed(seed)
    o = {"dz": _rand((n, c4, h, w_), dtype, dev, g), "x3": _rand((n, c4, h, w_), dtype, dev, g),
         "x2": _rand((n, c4, h, w_), dtype, dev, g) if two else None}
    for s in ("", "2"):
        o["gamma" + s] = torch.rand(c4, device=dev, generator=g) + 0.5
        o["mean" + s] = torch.randn(c4, device=dev, generator=g) * 0.3
        o["invstd" + s] = torch.rand(c4, device=dev, generator=g) + 0.5
    for s in ("p1", "p2", "p3"):   # the statistics partials of the consuming conv's epilogue: any values
        o[s] = torch.randn(c4, 3, device=dev, generator=g)
    o["w"] = _rand((c4, c, 1, 1), dtype, dev, g, (2.0 / c4) ** 0.5)
    o["bn_x"] = _rand((n, c, h, w_), dtype, dev, g)
    o["bn_mean"] = torch.randn(c, device=dev, generator=g) * 0.3
    o["bn_coef"] = torch.cat([torch.rand(c, device=dev, generator=g) + 0.5, torch.randn(c, device=dev, generator=g) * 0.3])
    return o


def _finalize_and_apply(o, apply):
    C_ = ops.native()
    if o["x2"] is None:
        return C_.bn_bwd_partials(o["dz"], o["x3"], o["gamma"], o["mean"], o["invstd"], None, o["p1"], o["p2"],
                                  True, True, apply)
    return C_.bn2_bwd_partials(o["dz"], o["x3"], o["x2"], o["gamma"], o["gamma2"], o["mean"], o["invstd"],
                               o["mean2"], o["invstd2"], o["p1"], o["p2"], o["p3"], True, apply)


def _reference(o):
    C_ = ops.native()
    r = _finalize_and_apply(o, True)
    out = {"dx3": r[0], "dx_ds": r[1] if o["x2"] is not None else None}
    out.update({f"dparam{i}": t for i, t in enumerate(r[(1 if o["x2"] is None else 2):])})
    out["dx"], out["p1"], out["p2"], _ = C_.conv_dgrad_bnstats(out["dx3"], o["w"], 0, o["bn_x"], o["bn_mean"],
                                                               o["bn_coef"])
    return out


def _poison(shapes_dtypes, dev):
    """Best effort: leave freed blocks of the outputs' sizes filled with NaNs / 0xA5 bytes in the caching
    allocator.  The binding allocates its outputs itself, and they usually land on these blocks, where an
    element the kernel skips then shows; nothing here depends on it - the bitwise comparison with the
    reference covers every element either way (uninitialised memory does not equal the reference)."""
    junk = []
    for shape, dtype in shapes_dtypes:
        t = torch.empty(shape, dtype=dtype, device=dev)
        t.view(torch.uint8).fill_(0xA5) if dtype == torch.float32 else t.fill_(float("nan"))
        junk.append(t)
    torch.cuda.synchronize()
    del junk


def _fused(o):
    C_ = ops.native()
    r = _finalize_and_apply(o, False)
    wt = C_.conv_wt_flip_multi([o["w"]])[0]
    c, m = o["w"].shape[1], o["dz"].numel() // o["dz"].shape[1]
    _poison([(tuple(o["dz"].shape), o["dz"].dtype)] * 2 + [(tuple(o["bn_x"].shape), o["dz"].dtype)]
            + [((c, (m + 127) // 128), torch.float32)] * 2, o["dz"].device)
    dx3, dx_ds, dx, p1, p2 = C_.conv1x1_tail_bwd(o["dz"], o["x3"], o["x2"], r[0], o["mean"],
                                                 o["mean2"] if o["x2"] is not None else None, wt, o["bn_x"],
                                                 o["bn_mean"], o["bn_coef"])
    out = {"dx3": dx3, "dx_ds": dx_ds}
    out.update({f"dparam{i}": t for i, t in enumerate(r[(1 if o["x2"] is None else 2):])})
    out.update({"dx": dx, "p1": p1, "p2": p2})
    return out


def _same_outputs(ref, out):
    assert ref.keys() == out.keys()
    for name in ref:
        if ref[name] is None:
            assert out[name] is None, name
        else:
            _same(name, ref[name], out[name])


@pytest.mark.parametrize("two", [False, True], ids=["one-bn", "two-bn"])
@pytest.mark.parametrize("c", [64, 128])
@pytest.mark.parametrize("c4", [64, 256, 512])  # 1, 4 and 8 K-steps
@pytest.mark.parametrize("nhw", [(1, 5, 5), (3, 7, 7), (3, 10, 10)], ids=["m25", "m147", "m300"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fused_kernel_is_bitwise_apply_then_dgrad(cuda, unsplit, dtype, nhw, c4, c, two):
    """M = 25 (less than a tile), 147 (ragged second tile) and 300 (three tiles)."""
    o = _operands(cuda, dtype, nhw, c4, c, two, 300 + c4 + c + nhw[1])
    ref, out = _reference(o), _fused(o)
    assert ref["dx"].float().abs().max() > 0 and ref["p1"].abs().max() > 0 and ref["p2"].abs().max() > 0
    _same_outputs(ref, out)


@pytest.mark.parametrize("two", [False, True], ids=["one-bn", "two-bn"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_fused_kernel_special_values(cuda, unsplit, dtype, two):
    """-0.0, +-inf, NaN and values that round to +-0 in dz, x3 and bn2's input, a zero k1 channel, and
    mask decisions at fma(x, a, b) = +-0: the same bits out, NaN payloads and zero signs included."""
    c4, c = 256, 64
    o = _operands(cuda, dtype, (3, 7, 7), c4, c, two, 11)
    specials = [-0.0, 0.0, float("inf"), -float("inf"), float("nan")]
    small = 1e-37 if dtype == torch.bfloat16 else 6e-8
    flat = {}
    for name, shift in (("dz", 0), ("x3", 3), ("bn_x", 5)):
        t = o[name]
        ch = t.shape[1]
        flat[name] = t.permute(0, 2, 3, 1).reshape(-1, ch)   # a view of the channels_last storage
        assert flat[name].data_ptr() == t.data_ptr()
        for i, v in enumerate(specials):
            flat[name][(5 * i + shift) % 147, (37 * i + shift) % ch] = v
            flat[name][-1 - i, (11 * i + shift) % ch] = v
    o["gamma"][5] = 0.0          # k1 = 0: 0 * inf = NaN where dz is infinite
    # channel 9: dz far below the 16-bit type's normal range and x3 = mean: dx3 rounds to +-0 or k3
    flat["dz"][0:40, 9], flat["dz"][40:60, 9] = small, -small
    flat["x3"][0:60, 9] = 0.0
    o["mean"][9] = 0.0
    # bn2 channels 3 / 4 / 5: fma(x, a, b) is exactly +0, +0 and -0: the mask is off, dz = 0
    a, b = o["bn_coef"][:c], o["bn_coef"][c:]
    a[3], b[3] = 1.0, -0.5
    a[4], b[4] = -1.0, 0.5
    a[5], b[5] = -1.0, -0.0
    flat["bn_x"][0:50, 3] = 0.5
    flat["bn_x"][0:50, 4] = 0.5
    flat["bn_x"][0:50, 5] = 0.0
    flat["bn_x"][50:60, 5] = -0.0    # (-0) * (-1) + (-0) = +0
    flat["bn_x"][60:80, 3] = small   # tiny against b: the mask follows b's sign
    ref, out = _reference(o), _fused(o)
    assert torch.isnan(ref["dx3"].float()).any() and torch.isinf(ref["dx3"].float()).any()
    assert torch.isnan(ref["dx"].float()).any()
    _same_outputs(ref, out)


def test_finalize_only_leaves_the_apply_to_the_caller(cuda):
    """bn_bwd_partials(apply=False) + bn_bwd_apply_pre is bn_bwd_partials, bit for bit."""
    C_ = ops.native()
    o = _operands(cuda, torch.bfloat16, (3, 7, 7), 256, 64, True, 5)
    o1 = dict(o, x2=None)
    dx, dg, db = _finalize_and_apply(o1, True)
    kbuf, dg_, db_ = _finalize_and_apply(o1, False)
    _same("dx", dx, C_.bn_bwd_apply_pre(o["dz"], o["x3"], o["mean"], kbuf))
    _same("dgamma", dg, dg_)
    _same("dbeta", db, db_)
    dx, dx2, *dp = _finalize_and_apply(o, True)
    kbuf, none, *dp_ = _finalize_and_apply(o, False)
    assert none is None and kbuf.numel() == 6 * 256
    _same("dx", dx, C_.bn_bwd_apply_pre(o["dz"], o["x3"], o["mean"], kbuf[:768]))
    _same("dx2", dx2, C_.bn_bwd_apply_pre(o["dz"], o["x2"], o["mean2"], kbuf[768:]))
    for i, (p, q) in enumerate(zip(dp, dp_)):
        _same(f"dparam{i}", p, q)


# ---- refusals ----------------------------------------------------------------------------------
def test_refused_shapes_raise_and_write_nothing(cuda):
    C_ = ops.native()
    C_.conv_set_splitk(0)
    try:
        assert C_.conv1x1_tail_bwd_refusal(192, 256, 64) is None
        assert C_.conv1x1_tail_bwd_refusal(192, 1024, 256) is not None     # two output-channel tiles
        assert C_.conv1x1_tail_bwd_refusal(192, 96, 64) is not None        # 4C % 64
        C_.conv_set_variant(9)                                             # a forced 8-wave tile
        assert C_.conv1x1_tail_bwd_refusal(192, 256, 64) is not None
        C_.conv_set_variant(0)
        C_.conv_set_splitk(1)
        # M = 192 and four K-steps: not split eagerly, split under graph capture - refused in both
        assert C_.conv_fwd_splits(192, 64, 256, False) == 1 and C_.conv_fwd_splits(192, 64, 256, True) > 1
        assert C_.conv1x1_tail_bwd_refusal(192, 256, 64) is not None
        o = _operands(cuda, torch.bfloat16, (3, 8, 8), 256, 64, False, 3)
        kbuf = _finalize_and_apply(o, False)[0]
        wt = C_.conv_wt_flip_multi([o["w"]])[0]
        before = torch.cuda.memory_allocated()
        with pytest.raises(RuntimeError):
            C_.conv1x1_tail_bwd(o["dz"], o["x3"], None, kbuf, o["mean"], None, wt, o["bn_x"], o["bn_mean"], o["bn_coef"])
        assert torch.cuda.memory_allocated() == before
        # a 3x3 weight, a strided conv's smaller output and a wrong channel count never reach the kernel
        C_.conv_set_splitk(0)
        w3 = _rand((64, 256, 3, 3), torch.bfloat16, cuda, torch.Generator(device=cuda).manual_seed(1))
        for bad_wt, bad_dz in ((w3, o["dz"]), (wt, o["dz"][:, :, ::2, ::2].contiguous(memory_format=CL))):
            with pytest.raises(RuntimeError):
                C_.conv1x1_tail_bwd(bad_dz, o["x3"], None, kbuf, o["mean"], None, bad_wt, o["bn_x"], o["bn_mean"],
                                    o["bn_coef"])
    finally:
        C_.conv_set_variant(0)
        C_.conv_set_splitk(1)


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


# ---- block level -------------------------------------------------------------------------------
def _three_blocks(dtype, dev, planes=64):
    """64 -> (64) -> 256 with a downsample (two-BN tail over a 64 -> 256 conv3), 256 -> (64) -> 256
    (plain tail), 256 -> (128) -> 512 / stride 2 (the last tail: its gradient comes from outside, no
    masked dz, nothing to fuse).  N = 3 at 10x10: M = 300, two full tiles and a ragged one."""
    g = torch.Generator(device=dev).manual_seed(7)
    p = planes
    ds0 = nn.Sequential(nn.Conv2d(64, 4 * p, 1, 1, bias=False), nn.BatchNorm2d(4 * p))
    ds2 = nn.Sequential(nn.Conv2d(4 * p, 8 * p, 1, 2, bias=False), nn.BatchNorm2d(8 * p))
    net = nn.Sequential(Bottleneck(64, p, 1, ds0), Bottleneck(4 * p, p), Bottleneck(4 * p, 2 * p, 2, ds2)).to(dev)
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
    x = _rand((3, 64, 10, 10), dtype, dev, g)
    return net.train(), x


def _run_blocks(net0, x0, fuse, monkeypatch, variants=None, between=None, extra_loss=False, repeat=1,
                fuse_bwd=None):
    """Forward and backward of a copy of the blocks with the switch at ``fuse`` (``fuse_bwd``: its
    value from the end of the forward on); ``between(net)`` runs between the two."""
    native_conv.reset_side_channels()
    net = copy.deepcopy(net0)
    if variants is not None:
        native_conv.profile_calls(True)
    out = {}
    try:
        for rep in range(repeat):
            monkeypatch.setattr(native_conv, "TAIL_CONV3_BWD_FUSE", fuse)
            x = x0.detach().clone().requires_grad_(True)
            net.zero_grad(set_to_none=True)
            seen = []
            hook = net[1].conv3.register_forward_hook(lambda m, i, o: seen.append(o))
            try:
                y = net(x)
            finally:
                hook.remove()
            if fuse_bwd is not None:
                monkeypatch.setattr(native_conv, "TAIL_CONV3_BWD_FUSE", fuse_bwd)
            if between is not None:
                between(net)
            gy = _rand(tuple(y[0].shape), y[0].dtype, x.device, torch.Generator(device=x.device).manual_seed(8))
            if extra_loss:   # a second consumer of block 1's x3: autograd accumulates into its gradient
                side = (seen[0].float() ** 2).sum() * 1e-3
                torch.autograd.backward([y[0], side], [gy, torch.ones_like(side)])
            else:
                y[0].backward(gy)
            out = {"x.grad": x.grad, "y.conv": y[0].detach(), "y.identity": y[1].detach()}
    finally:
        if variants is not None:
            variants.extend(v for kind, _, v, _, _ in native_conv.take_profile() if kind == "dgrad")
            native_conv.profile_calls(False)
    assert not native_conv._BNB_PARTIALS and not native_conv._TAIL_STASHED
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
    assert v_off.count(FUSED) == 0 and not any(v.startswith("taken-from-tail") for v in v_off)
    # block 0 (two BatchNorms) and block 1 (one); each conv3's own backward then launched no backward-data
    assert v_on.count(FUSED) == 2 and sum(v.startswith("taken-from-tail") for v in v_on) == 2
    assert len(v_on) == len(v_off) + 2
    _same_dicts(off, on)


@pytest.mark.parametrize("knob", ["TAIL_CONV1_FUSE", "BN_BWD_FUSE", "S2_COMPACT_DRES"])
def test_blocks_with_another_fusion_off(cuda, unsplit, knob, monkeypatch):
    net, x = _three_blocks(torch.bfloat16, cuda)
    monkeypatch.setattr(fused_bn if knob == "TAIL_CONV1_FUSE" else native_conv, knob, False)
    v_on = []
    off = _run_blocks(net, x, False, monkeypatch)
    on = _run_blocks(net, x, True, monkeypatch, v_on)
    # without BN_BWD_FUSE no conv forms the tail's masked gradient: nothing to fuse
    assert v_on.count(FUSED) == (0 if knob == "BN_BWD_FUSE" else 2)
    _same_dicts(off, on)


@pytest.mark.parametrize("fwd, bwd", [(True, False), (False, True)], ids=["on-off", "off-on"])
def test_blocks_switch_flipped_between_forward_and_backward(cuda, unsplit, fwd, bwd, monkeypatch):
    net, x = _three_blocks(torch.bfloat16, cuda)
    v = []
    off = _run_blocks(net, x, False, monkeypatch)
    mixed = _run_blocks(net, x, fwd, monkeypatch, v, fuse_bwd=bwd)
    assert v.count(FUSED) == 0
    _same_dicts(off, mixed)


def test_blocks_under_the_default_split_policy_are_not_fused(cuda, monkeypatch):
    """M = 300 and four K-steps: the graph policy would split these backward-datas, so nothing is
    fused and the results are the parent's."""
    net, x = _three_blocks(torch.bfloat16, cuda)
    v_on = []
    off = _run_blocks(net, x, False, monkeypatch)
    on = _run_blocks(net, x, True, monkeypatch, v_on)
    assert v_on.count(FUSED) == 0
    _same_dicts(off, on)


def test_blocks_with_two_channel_tiles_are_not_fused(cuda, unsplit, monkeypatch):
    """C = 256 in the first two blocks: two output-channel tiles, the kernel refuses."""
    net, x = _three_blocks(torch.bfloat16, cuda, planes=256)
    v_on = []
    off = _run_blocks(net, x, False, monkeypatch)
    on = _run_blocks(net, x, True, monkeypatch, v_on)
    assert v_on.count(FUSED) == 0
    _same_dicts(off, on)


def _captured_blocks(net0, x0, fuse, monkeypatch):
    """One forward and backward of the blocks captured in a graph and replayed: (outputs, fused launches)."""
    monkeypatch.setattr(native_conv, "TAIL_CONV3_BWD_FUSE", fuse)
    gy = _rand((3, 512, 5, 5), x0.dtype, x0.device, torch.Generator(device=x0.device).manual_seed(8))

    def step(net, x):
        native_conv.reset_side_channels()
        y = net(x)
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
    fused = []
    real = native_conv.tail_bwd_launch
    monkeypatch.setattr(native_conv, "tail_bwd_launch", lambda *a: (fused.append(True), real(*a))[1])
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = step(net, x)
        g.replay()
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(native_conv, "tail_bwd_launch", real)
    return eager, out, len(fused)


def test_blocks_captured_step_replays_like_eager(cuda, unsplit, monkeypatch):
    net0, x0 = _three_blocks(torch.bfloat16, cuda)
    eager, out, fused = _captured_blocks(net0, x0, True, monkeypatch)
    assert fused == 2
    for i, (a, b) in enumerate(zip(eager, out)):
        _same(f"output {i}", a, b)
    _, out_off, none = _captured_blocks(net0, x0, False, monkeypatch)
    assert none == 0
    for i, (a, b) in enumerate(zip(out_off, out)):
        _same(f"output {i} against the switch off", a, b)


def test_blocks_captured_under_the_default_split_policy_are_not_fused(cuda, monkeypatch):
    """Under capture these backward-datas are split: the switch changes nothing in the replayed step."""
    net0, x0 = _three_blocks(torch.bfloat16, cuda)
    assert ops.native().conv_fwd_splits(300, 64, 256, True) > 1
    _, off, f_off = _captured_blocks(net0, x0, False, monkeypatch)
    _, on, f_on = _captured_blocks(net0, x0, True, monkeypatch)
    assert f_off == 0 and f_on == 0
    for i, (a, b) in enumerate(zip(off, on)):
        _same(f"output {i}", a, b)


# ---- stale stashes -----------------------------------------------------------------------------
def test_backward_twice_on_fresh_graphs(cuda, unsplit, monkeypatch):
    net, x = _three_blocks(torch.bfloat16, cuda)
    v = []
    off = _run_blocks(net, x, False, monkeypatch, repeat=2)
    on = _run_blocks(net, x, True, monkeypatch, v, repeat=2)
    assert v.count(FUSED) == 4
    _same_dicts(off, on)


def test_weight_changed_between_forward_and_backward(cuda, unsplit, monkeypatch):
    """In place behind autograd's back (``.data``: no version bump): both paths flip the weight as it is
    at backward time.  With a version bump autograd itself refuses the backward in either mode."""
    net, x = _three_blocks(torch.bfloat16, cuda)

    def halve(n):
        n[1].conv3.weight.data.mul_(0.5)

    off = _run_blocks(net, x, False, monkeypatch, between=halve)
    on = _run_blocks(net, x, True, monkeypatch, between=halve)
    _same_dicts(off, on)

    def bump(n):
        with torch.no_grad():
            n[1].conv3.weight.mul_(0.5)

    for fuse in (False, True):
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            _run_blocks(net, x, fuse, monkeypatch, between=bump)
        native_conv.reset_side_channels()


def test_x3_with_a_second_consumer(cuda, unsplit, monkeypatch):
    """Autograd adds a second gradient to the tail's dx3: conv3's backward sees another tensor (or
    another version), ignores the stash and runs its backward-data on what it was given."""
    net, x = _three_blocks(torch.bfloat16, cuda)
    v = []
    off = _run_blocks(net, x, False, monkeypatch, extra_loss=True)
    on = _run_blocks(net, x, True, monkeypatch, v, extra_loss=True)
    assert v.count(FUSED) == 2                                              # the tails did fuse
    assert sum(t.startswith("taken-from-tail") for t in v) == 1             # block 0's conv3 took it, block 1's not
    plain = _run_blocks(net, x, False, monkeypatch)
    assert not torch.equal(_bits(plain["x.grad"]), _bits(off["x.grad"]))    # the second consumer counts
    _same_dicts(off, on)


# ---- model level -------------------------------------------------------------------------------
def test_resnet50_step_on_is_bitwise_off(cuda, unsplit, monkeypatch):
    from distributed_pytorch_training_amd.config import parse_args
    from distributed_pytorch_training_amd.engine.trainer import Trainer
    from distributed_pytorch_training_amd.models import build_model

    batch, px = 4, 64
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
        monkeypatch.setattr(native_conv, "TAIL_CONV3_BWD_FUSE", fuse)
        m = build_model("resnet50", 1000, cuda, image_size=px, channels_last=True)
        tr = Trainer(m, parse_args(argv), 0, 1, cuda, log=lambda s: None)
        tr.module.load_state_dict(state)
        tr.sync_weights()
        tr.model.train()
        native_conv.profile_calls(True)
        try:
            logits, loss = tr.train_step(x, t)
            torch.cuda.synchronize()
            fused = sorted(key[:4] for kind, key, v, _, _ in native_conv.take_profile()
                           if kind == "dgrad" and v == FUSED)
        finally:
            native_conv.profile_calls(False)
        out = {"loss": loss.detach().clone(), "grads": tr.ddp.arena.grad_flat.detach().clone()}
        if torch.is_tensor(logits):
            out["logits"] = logits.detach().clone()
        out.update({"p." + n: p.detach().clone() for n, p in tr.module.named_parameters()})
        out.update({"b." + n: b.detach().clone() for n, b in tr.module.named_buffers()})
        tr.close()
        return out, fused

    off, f_off = run(False)
    on, f_on = run(True)
    assert f_off == []
    # (C, H, W, 4C): layer1.0-2 conv3 and layer2.0-3 conv3 at 64 px
    assert f_on == sorted([(64, 16, 16, 256)] * 3 + [(128, 8, 8, 512)] * 4)
    _same_dicts(off, on)
