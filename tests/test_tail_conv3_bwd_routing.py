"""Link and stash logic of the tail-backward / conv3 backward-data fusion (ops/conv.py
TAIL_CONV3_BWD_FUSE) on the CPU, with a fake native module: the stash is taken once, ignored on every
mismatch, dropped by begin_step(), and never consulted with the switch off."""
import types

import pytest
import torch

from distributed_pytorch_training_amd.ops import conv as native_conv
from distributed_pytorch_training_amd.ops.handover import BnSource, TailSlot

CL = torch.channels_last


class _Red:
    done = False


class _FakeNative:
    """Records the launches ops/conv.py asks for; every result is a fresh tensor of the right shape."""

    def __init__(self):
        self.calls = []

    def conv_wgrad_deferred(self, dy, x, wshape, s, p):
        self.calls.append("wgrad")
        return torch.zeros(wshape), _Red()

    def conv_wgrad(self, dy, x, wshape, s, p, fp32_out):
        self.calls.append("wgrad+reduce")
        return torch.zeros(wshape)

    def bn_bwd_apply_pre(self, dz, x, mean, kbuf):
        self.calls.append("apply")
        assert kbuf.numel() == 3 * x.shape[1]
        return torch.full_like(x, 7.0)

    def conv_reduce_flush(self, red):
        self.calls.append("reduce")
        red.done = True

    def conv_dgrad_bnstats(self, dy, w, p, bn_x, bn_mean, bn_coef, w_flipped=None, wgrad_reduce=None):
        self.calls.append("dgrad")
        if wgrad_reduce is not None:
            wgrad_reduce.done = True
        c = w.shape[1]
        return torch.full_like(bn_x, 2.0), torch.zeros(c, 1), torch.zeros(c, 1), None

    def conv_wt_flip_multi(self, ws):
        self.calls.append("flip")
        return [w.permute(1, 0, 2, 3).contiguous(memory_format=CL) for w in ws]

    def conv1x1_tail_bwd(self, dz, x3, x2, kbuf, mean, mean2, wt, bn_x, bn_mean, bn_coef):
        self.calls.append("fused")
        c = bn_x.shape[1]
        return (torch.full_like(x3, 3.0), None if x2 is None else torch.full_like(x2, 4.0),
                torch.full_like(bn_x, 5.0), torch.ones(c, 1), torch.ones(c, 1))

    def conv1x1_tail_bwd_refusal(self, m, c4, c):
        self.calls.append("refusal")
        return None if c in (64, 128) else "needs C of 64 or 128"


@pytest.fixture
def fake(monkeypatch):
    f = _FakeNative()
    monkeypatch.setattr(native_conv, "native", lambda: f)
    monkeypatch.setattr(native_conv, "TAIL_CONV3_BWD_FUSE", True)
    monkeypatch.setattr(native_conv, "BN_BWD_FUSE", True)
    native_conv.end_caching()
    native_conv.reset_side_channels()
    yield f
    native_conv.reset_side_channels()


def _case(c=64, c4=256):
    """conv3 (C -> 4C, 1x1) on a BN+ReLU output, the tail's input x3 and masked gradient dz."""
    n, h, w_ = 2, 3, 3
    bn_x = torch.randn(n, c, h, w_).to(torch.bfloat16).contiguous(memory_format=CL)
    x = torch.randn(n, c, h, w_).to(torch.bfloat16).contiguous(memory_format=CL).requires_grad_(True)
    w = torch.randn(c4, c, 1, 1).to(torch.bfloat16).contiguous(memory_format=CL).requires_grad_(True)
    bn_src = BnSource(bn_x, torch.zeros(c), torch.zeros(2 * c))
    x3 = torch.randn(n, c4, h, w_).to(torch.bfloat16).contiguous(memory_format=CL)
    dz = torch.randn_like(x3)
    link = native_conv._tail_link(x, w, 1, 0, (0, 0), bn_src)
    ctx = types.SimpleNamespace(saved_tensors=(x.detach(), w), stride=1, pad=0, needs_input_grad=(True, True),
                                bn_src=bn_src, res_slot=None, compact_dres=False, tail_link=link)
    return ctx, link, x3, dz, w


def _tail(link, x3, dz):
    assert native_conv.tail_bwd_refusal(link, x3) is None
    return native_conv.tail_bwd_launch(link, dz, x3, torch.zeros(3 * x3.shape[1]), torch.zeros(x3.shape[1]))[0]


def test_link_only_for_an_eligible_conv3(fake):
    ctx, link, x3, dz, w = _case()
    assert link is not None and link.w is w and link.wv == w._version and link.bn_src is ctx.bn_src
    x = ctx.saved_tensors[0].requires_grad_(True)
    w3 = torch.randn(256, 64, 3, 3).to(torch.bfloat16).contiguous(memory_format=CL)
    assert native_conv._tail_link(x, w3, 1, 1, (0, 0), ctx.bn_src) is None                  # 3x3
    assert native_conv._tail_link(x, w, 2, 0, (0, 0), ctx.bn_src) is None                   # stride 2
    assert native_conv._tail_link(x, w, 1, 0, (3, 3), ctx.bn_src) is None                   # explicit output size
    assert native_conv._tail_link(x, w, 1, 0, (0, 0), None) is None                         # no BN+ReLU before it
    assert native_conv._tail_link(x, w, 1, 0, (0, 0), BnSource(ctx.bn_src.x, ctx.bn_src.mean, slot=TailSlot())) is None   # a block tail
    assert native_conv._tail_link(x.detach(), w, 1, 0, (0, 0), ctx.bn_src) is None          # no input gradient
    with torch.no_grad():
        assert native_conv._tail_link(x, w, 1, 0, (0, 0), ctx.bn_src) is None


def test_refusals_reach_the_tail(fake, monkeypatch):
    ctx, link, x3, dz, w = _case()
    assert native_conv.tail_bwd_refusal(None, x3) == "no link"
    assert native_conv.tail_bwd_refusal(link, x3.float()) is not None        # not a 16-bit type
    assert native_conv.tail_bwd_refusal(link, x3[:, :128]) is not None       # not this conv's output
    ctx2, link2, x32, _, _ = _case(c=256, c4=1024)
    assert native_conv.tail_bwd_refusal(link2, x32) == "needs C of 64 or 128"
    with torch.no_grad():
        w.mul_(2.0)                                                          # the weight changed since the forward
    assert native_conv.tail_bwd_refusal(link, x3) is not None
    monkeypatch.setattr(native_conv, "TAIL_CONV3_BWD_FUSE", False)
    assert native_conv.tail_bwd_refusal(link2, x32) == "switched off"


def test_stash_is_taken_once(fake):
    ctx, link, x3, dz, w = _case()
    dx3 = _tail(link, x3, dz)
    assert (dx3 == 3.0).all() and link.stash is not None and len(native_conv._TAIL_STASHED) == 1
    fake.calls.clear()
    dx, dw = native_conv._backward(ctx, dx3)
    assert (dx == 5.0).all() and fake.calls == ["wgrad+reduce"]              # no backward-data launch
    assert link.stash is None and not native_conv._TAIL_STASHED
    part = native_conv.take_bnb_partials(dx)
    assert part is not None and (part.p1 == 1.0).all() and part.dres_ptr is None   # bn2's statistics travel on
    fake.calls.clear()
    dx, dw = native_conv._backward(ctx, dx3)                                 # a second backward: nothing left
    assert (dx == 2.0).all() and fake.calls == ["wgrad", "dgrad"]


@pytest.mark.parametrize("how", ["other-tensor", "version", "generation", "shape", "weight-version", "weight"])
def test_stash_is_ignored_on_a_mismatch(fake, how):
    ctx, link, x3, dz, w = _case()
    dx3 = _tail(link, x3, dz)
    dy = dx3
    if how == "other-tensor":
        dy = dx3 + 1.0                      # autograd summed a second gradient out of place
    elif how == "version":
        dx3.add_(1.0)                       # ... or in place
    elif how == "generation":
        native_conv._GEN[0] += 1
    elif how == "shape":
        def fold(t):   # [2, C, 3, 3] channels_last seen as [1, C, 6, 3]: the same memory, version and pointer
            c = t.shape[1]
            return t.as_strided((1, c, 6, 3), (18 * c, 1, 3 * c, c))

        dy = fold(dx3)
        assert dy.data_ptr() == dx3.data_ptr() and dy._version == dx3._version and dy.shape != dx3.shape
        ctx.saved_tensors = (fold(ctx.saved_tensors[0]), w)
        ctx.bn_src = BnSource(fold(ctx.bn_src.x), ctx.bn_src.mean, ctx.bn_src.coef)
    elif how == "weight-version":
        with torch.no_grad():
            w.mul_(2.0)
    elif how == "weight":
        ctx.saved_tensors = (ctx.saved_tensors[0], w.detach().clone(memory_format=torch.preserve_format))
    fake.calls.clear()
    dx, dw = native_conv._backward(ctx, dy)
    assert (dx == 2.0).all() and fake.calls == ["wgrad", "dgrad"]            # the unfused backward-data
    assert link.stash is None and not native_conv._TAIL_STASHED             # and the stash is gone


@pytest.mark.parametrize("drop", ["begin_step", "reset_side_channels"])
def test_leftover_stash_is_dropped(fake, drop):
    ctx, link, x3, dz, w = _case()
    dx3 = _tail(link, x3, dz)
    assert link.stash is not None
    getattr(native_conv, drop)()
    native_conv.end_caching()
    assert link.stash is None and not native_conv._TAIL_STASHED
    fake.calls.clear()
    dx, dw = native_conv._backward(ctx, dx3)
    assert (dx == 2.0).all() and fake.calls == ["wgrad", "dgrad"]


def test_stash_is_never_consulted_with_the_switch_off(fake, monkeypatch):
    ctx, link, x3, dz, w = _case()
    dx3 = _tail(link, x3, dz)
    monkeypatch.setattr(native_conv, "TAIL_CONV3_BWD_FUSE", False)           # flipped before conv3's backward

    class _NoTouch:
        def __getattr__(self, name):
            raise AssertionError("the link was consulted")

    ctx.tail_link = _NoTouch()
    fake.calls.clear()
    dx, dw = native_conv._backward(ctx, dx3)
    assert (dx == 2.0).all() and fake.calls == ["wgrad", "dgrad"]
    # and with the switch off at forward time there is no link at all
    x = ctx.saved_tensors[0].requires_grad_(True)
    assert native_conv._tail_link(x, w, 1, 0, (0, 0), ctx.bn_src) is None


def test_flip_cache_is_used_when_on(fake):
    ctx, link, x3, dz, w = _case()
    native_conv.begin_step()
    try:
        _tail(link, x3, dz)
        assert fake.calls.count("flip") == 1
        fake.calls.clear()
        _tail(link, x3, dz)                 # same step: the cached flipped weight
        assert fake.calls.count("flip") == 0
    finally:
        native_conv.end_caching()


@pytest.mark.parametrize("two", [False, True])
def test_a_launch_the_binding_refuses_falls_back_to_the_apply_pass(fake, two, monkeypatch):
    ctx, link, x3, dz, w = _case()
    x2 = torch.randn_like(x3) if two else None
    kbuf, mean = torch.zeros((6 if two else 3) * 256), torch.zeros(256)

    def refuse(*a):
        fake.calls.append("fused")
        raise RuntimeError("conv1x1_tail_bwd: the split-K policy splits this backward-data")

    fake.conv1x1_tail_bwd = refuse
    monkeypatch.setattr(native_conv, "_mark", lambda: 0)     # (no timing events on the CPU)
    monkeypatch.setattr(native_conv, "_CALLS", [])
    dx3, dx_ds = native_conv.tail_bwd_apply(link, dz, x3, kbuf, mean, x2, mean if two else None)
    noted = [v for kind, _, v, _, _ in native_conv._CALLS]
    monkeypatch.setattr(native_conv, "_CALLS", None)
    assert (dx3 == 7.0).all() and (dx_ds is None) == (not two)               # filled by the apply pass(es)
    assert fake.calls == ["flip", "fused"] + ["apply"] * (2 if two else 1)
    assert link.stash is None and not native_conv._TAIL_STASHED and noted == ["tail-bwd-refused"]
    fake.calls.clear()
    dx, dw = native_conv._backward(ctx, dx3)                                 # conv3 runs its own backward-data
    assert (dx == 2.0).all() and fake.calls == ["wgrad", "dgrad"]


@pytest.mark.parametrize("err", [RuntimeError("x3 must be channels_last contiguous"),
                                 RuntimeError("HIP error: an illegal memory access was encountered")])
def test_other_errors_of_the_launch_are_raised(fake, err):
    ctx, link, x3, dz, w = _case()

    def fail(*a):
        raise err

    fake.conv1x1_tail_bwd = fail
    with pytest.raises(RuntimeError) as got:
        native_conv.tail_bwd_apply(link, dz, x3, torch.zeros(768), torch.zeros(256))
    assert got.value is err and "apply" not in fake.calls
