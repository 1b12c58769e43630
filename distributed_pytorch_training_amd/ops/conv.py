"""Channels-last bf16 / fp16 convolution autograd op on the hand-written MFMA kernels
(csrc/kernels/conv_kernels.hip).

forward   implicit-GEMM conv; with ``bn_stats`` its epilogue also emits the per-channel
          (sum, sum of squares) partials of the bf16 output, which the following fused
          BatchNorm consumes instead of re-reading the activation (ops/bn.py picks them up
          from the output tensor's ``_dpt_bn_partials`` attribute).
backward  input gradient: the same kernel on dy reading the weight as [co][ci] with flipped taps
          through transposing LDS reads (stride 1), or, stride 2, four parity-class convs whose
          outputs are scattered onto the even/odd rows and columns of dx (a 1x1 downsample conv on a
          block tail's identity alias keeps its one non-empty class compact instead and hands it to
          the tail's conv-path consumer, S2_COMPACT_DRES); weight gradient: split-K MFMA kernel
          with transposing LDS reads, bf16 (the shadow weight's dtype).

Replaces the reference's cuDNN convolutions (reference
``train_ddp.py:205,207`` -> torchvision ``resnet18`` convs); measured per shape against MIOpen
in ``profiles/conv_kernels_vs_miopen_v1.md``.
"""
from __future__ import annotations

import os

import torch

from . import native, native_available
from .handover import (COMPACT_RES, MASKED_NO_RES, _BNB_PARTIALS, _GEN, _TAIL_STASHED,  # noqa: F401 (re-exported)
                       Conv1Out, Conv3Link, _put_bnb, register_bnb_partials, reset_side_channels, take_bnb_partials)

_CL = torch.channels_last
# element types of the MFMA kernels (bf16 and fp16 operands, fp32 accumulation)
_DT16 = (torch.bfloat16, torch.float16)
# process-wide kill switch (environment); per-model routing lives on the conv modules
ENABLED = os.environ.get("DPT_NATIVE_CONV", "1") != "0"
# Backward-data of a conv fed by a fused BN+ReLU also sums that BN's backward statistics in its
# epilogue (the BN backward then skips its statistics pass).
BN_BWD_FUSE = os.environ.get("DPT_BN_BWD_FUSE", "1") != "0"
# Stride-2 backward-data on the MFMA kernels (four parity-class convs); 0 = MIOpen
S2_DGRAD = os.environ.get("DPT_S2_DGRAD", "1") != "0"
# A 1x1 / stride-2 downsample conv fed by a block tail's identity alias hands its input gradient
# to the tail's conv-path consumer compactly, [N, C, ceil(H/2), ceil(W/2)] (the pixels it read),
# and returns None to autograd: the full-resolution tensor, three quarters explicit zeros, is
# neither written nor read back by the consumer's BNR epilogue.  0 = the full tensor.
S2_COMPACT_DRES = os.environ.get("DPT_S2_COMPACT_DRES", "1") != "0"
# Backward-weight before backward-data, its split-K reduce run by extra blocks in the
# backward-data launch's tail (conv_wgrad_deferred / wgrad_reduce=): no reduce launch of its own
WGRAD_REDUCE_FUSE = os.environ.get("DPT_WGRAD_REDUCE_FUSE", "1") != "0"
# A bottleneck tail's backward apply also runs conv3's backward-data (one output-channel tile: 64 or
# 128 channels, ResNet-50's layer1 / layer2 conv3s; csrc/kernels/tail_conv3_bwd_kernels.hip): the tail
# writes dx3 and conv3's input gradient in one kernel and leaves the latter for conv3's backward, which
# then launches no backward-data - dx3 is not read back from HBM a second time.  0 = the two kernels.
TAIL_CONV3_BWD_FUSE = os.environ.get("DPT_TAIL_CONV3_BWD_FUSE", "1") != "0"
# The im2col stem path is correct but measured slower than MIOpen on ResNet-50's 7x7/2 stem at
# batch 256 (the [3.2M x 192] bf16 patch matrix is 1.2 GB written and read twice): opt-in only.
STEM_ENABLED = os.environ.get("DPT_NATIVE_STEM", "0") == "1"


# Convs with fewer output pixels than this go to MIOpen (default: none; a model can override it
# per conv through models.layers.fuse_native_layers(min_pixels=...)).  Small tile grids used to
# lose to MIOpen's small-shape kernels under hipGraph (ResNet-18 on 32x32: 128-2048 output
# pixels in layer2-4 at batch 128); the kernels now split the K loop over blocks there
# (conv_fwd_splits), which beats MIOpen at every size (BASELINE.md ResNet-18 table).
MIN_PIXELS = int(os.environ.get("DPT_CONV_MIN_PIXELS", "0"))


def supported(x: torch.Tensor, w: torch.Tensor, stride, padding, dilation, groups, min_pixels=None) -> bool:
    if not (ENABLED and x.is_cuda and native_available() and x.dtype in _DT16
            and w.dtype == x.dtype and x.dim() == 4 and groups == 1):
        return False
    if tuple(dilation) != (1, 1) or stride[0] != stride[1] or padding[0] != padding[1]:
        return False
    cout, cin, r, s = w.shape
    ho = (x.shape[2] + 2 * padding[0] - r) // stride[0] + 1
    wo = (x.shape[3] + 2 * padding[1] - s) // stride[1] + 1
    return (cin % 64 == 0 and cout % 64 == 0 and r == s and x.shape[1] == cin
            and x.shape[0] * ho * wo >= (MIN_PIXELS if min_pixels is None else min_pixels)
            and x.is_contiguous(memory_format=_CL))


def _cl(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous(memory_format=_CL) else t.contiguous(memory_format=_CL)


# In-step attribution (bench/conv_instep.py): when a list, every conv pass records a timing event
# on the current stream before and after its launches, tagged (pass, shape, epilogue variant).
# Off (None) in training: no event, no Python work.
_CALLS = None


def profile_calls(on: bool) -> None:
    global _CALLS
    _CALLS = [] if on else None


def take_profile():
    """[(pass, shape, variant, start_event, end_event)] recorded since profile_calls(True)."""
    out = list(_CALLS or [])
    if _CALLS is not None:
        _CALLS.clear()
    return out


def _mark():
    if _CALLS is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _note(kind, x, w, stride, pad, variant, e0, out_hw=(0, 0)):
    if _CALLS is None or e0 is None:
        return
    co, ci, r, _ = w.shape
    key = (ci, x.shape[2], x.shape[3], co, r, int(stride), int(pad), tuple(int(v) for v in out_hw))
    _CALLS.append((kind, key, variant, e0, _mark()))


def _dgrad_stride1(ctx, dy, x, w, src, wt, red, stash, compact):
    """(dx, variant) of a stride-1 conv; ``src``: the BnSource whose backward statistics the epilogue
    sums, ``compact``: the tail's slot holds a downsample conv's compact gradient to fold."""
    p = ctx.pad
    if src is not None and not src.is_tail and stash is not None:
        # the tail's backward formed dy and this gradient in one kernel
        _put_bnb(stash.dx, stash.p1, stash.p2, None, None)
        return stash.dx, "taken-from-tail"   # (the launch was noted as tail-bwd-apply+dgrad by the tail)
    if src is not None and not src.is_tail:
        dx, p1, p2, _ = native().conv_dgrad_bnstats(dy, w, p, src.x, src.mean, src.coef, w_flipped=wt,
                                                    wgrad_reduce=red)
        _put_bnb(dx, p1, p2, None, None)
        return dx, "bnrelu-stats"
    if (src is not None and _dres_ok(dres := src.slot.take_dres(), x)
            and (compact or dres.shape == x.shape)):
        # block-tail BN+add+ReLU (ops/bn.py pair outputs): the next block's tail already
        # produced the identity-path gradient dres; dx becomes the tail's masked total
        # gradient, the conv's input x is the tail's output y (the ReLU mask).  x2, mean2: the tail's
        # identity path was a downsample BatchNorm folded into it (ops/bn.py _BN2AddReLUPair) - also
        # sum that BN's statistic
        x2, mean2 = src.x2, src.mean2
        # the tail's 1-bit ReLU mask (ops/bn.py) is read instead of its output x when present
        dx, p1, p2, p3 = native().conv_dgrad_bnstats(dy, w, p, src.x, src.mean, None, x, dres, wt, x2, mean2,
                                                     wgrad_reduce=red, bn_mask=src.slot.mask,
                                                     bn_res_s2=compact)
        _put_bnb(dx, p1, p2, COMPACT_RES if compact else dres.data_ptr(), p3 if x2 is not None else None)
        return dx, "tail-stats-s2res" if compact else "tail+ds-stats" if x2 is not None else "tail-stats"
    dx = (native().conv_dgrad_flip(dy, w, p, wgrad_reduce=red)[0] if wt is None
          else native().conv_dgrad_preflipped(dy, wt, p, wgrad_reduce=red))
    return dx, "plain"


def _dgrad_stride2(ctx, dy, x, w, red):
    """(dx, variant) of a stride-2 conv on the parity-class kernels; dx is None when the gradient
    went compact into the tail's slot (``s2-compact``)."""
    p = ctx.pad
    src = ctx.bn_src if BN_BWD_FUSE else None
    rs = ctx.res_slot
    if (ctx.compact_dres and S2_COMPACT_DRES and BN_BWD_FUSE and rs is not None and rs.fold_s2
            and rs.dres is None):
        # the conv-path consumer of the tail has not run yet and will fold (see conv2d)
        rs.dres = native().conv_dgrad_s2(dy, w, p, x.shape[2], x.shape[3], wgrad_reduce=red, compact=True)[0]
        rs.dres_s2 = True
        return None, "s2-compact"
    if src is not None and not src.is_tail and w.shape[2] > 1:
        # BN+ReLU input: its backward statistics from the parity-class epilogues too
        dx, p1, p2 = native().conv_dgrad_s2(dy, w, p, x.shape[2], x.shape[3], src.x, src.mean, src.coef,
                                            wgrad_reduce=red)
        _put_bnb(dx, p1, p2, None, None)
        return dx, "s2-bnrelu-stats"
    return native().conv_dgrad_s2(dy, w, p, x.shape[2], x.shape[3], wgrad_reduce=red)[0], "s2"


def _backward(ctx, dy):
    x, w = ctx.saved_tensors
    dy = _cl(dy.to(x.dtype))
    s, p = ctx.stride, ctx.pad
    dx = dw = red = variant = None
    # the tail that produced dy may already have run this conv's backward-data (TAIL_CONV3_BWD_FUSE)
    link = getattr(ctx, "tail_link", None)
    stash = link.take_stash(dy, w) if (link is not None and TAIL_CONV3_BWD_FUSE) else None
    e0 = _mark()
    if ctx.needs_input_grad[1]:
        # (a taken stash: no backward-data launch will carry the reduce, so it is not deferred)
        if ctx.needs_input_grad[0] and WGRAD_REDUCE_FUSE and stash is None:
            dw, red = native().conv_wgrad_deferred(dy, x, list(w.shape), s, p)
        else:
            dw = native().conv_wgrad(dy, x, list(w.shape), s, p, False)
        _note("wgrad", x, w, s, p, "deferred-reduce" if red is not None else "reduce", e0)
        e0 = _mark()
    if ctx.needs_input_grad[0]:
        src = ctx.bn_src if (s == 1 and BN_BWD_FUSE) else None
        wt = _flipped(w) if s == 1 else None
        slot = ctx.bn_src.slot if ctx.bn_src is not None else None
        compact = False
        if slot is not None:
            # from here on the tail's downsample conv must not leave a compact gradient behind
            slot.fold_s2 = False
            # it ran first, left its compact gradient in the slot and returned None to autograd
            # (S2_COMPACT_DRES): fold it below, or nobody accounts for it
            compact = slot.take_dres_s2()
            if compact and not (src is not None and not src.has_downsample and _is_compact_of(slot.dres, x)):
                raise RuntimeError("fused block-tail backward: a downsample conv handed over a compact "
                                   "identity-path gradient that this conv's backward-data cannot fold")
        if s == 1:
            dx, variant = _dgrad_stride1(ctx, dy, x, w, src, wt, red, stash, compact)
        elif s == 2 and S2_DGRAD and x.dim() == 4:
            dx, variant = _dgrad_stride2(ctx, dy, x, w, red)
        else:
            dx = torch.ops.aten.convolution_backward(dy, x, w, None, (s, s), (p, p), (1, 1), False, (0, 0), 1,
                                                     (True, False, False))[0]
    if red is not None and not red.done:
        native().conv_reduce_flush(red)   # no native backward-data launch took it
    if variant is not None:
        _note("dgrad", x, w, s, p, variant + ("+reduce" if red is not None else ""), e0)
    if variant == "s2-compact":
        return None, dw   # the gradient went to the consumer through the slot, not through autograd
    if dx is not None and ctx.res_slot is not None:
        # x is the identity alias of a fused block tail and this conv its downsample: hand the
        # identity-path gradient to the tail's conv-path consumer (see ops/bn.py)
        ctx.res_slot.dres = dx
    return dx, dw


# Per-step flip cache: the stride-1 backward-data reads a flipped/transposed weight copy
# wt[ci][R-1-r][S-1-s][co].  With the cache on (the trainer calls begin_step() each step) the
# forward registers every such weight and the first backward-data of the step flips them all
# in ONE launch (46 launches per ResNet-50 step otherwise).
_FLIP = {"on": False, "pending": {}, "done": {}}


def begin_step() -> None:
    reset_side_channels()
    _FLIP["on"] = True
    _FLIP["pending"].clear()
    _FLIP["done"].clear()


def end_caching() -> None:
    _FLIP["on"] = False
    _FLIP["pending"].clear()
    _FLIP["done"].clear()


def _flipped(w: torch.Tensor):
    if not _FLIP["on"]:
        return None
    key = (w.data_ptr(), tuple(w.shape))
    wt = _FLIP["done"].get(key)
    if wt is None:
        pend = _FLIP["pending"]
        pend.setdefault(key, w)
        keys = list(pend.keys())
        for k, t in zip(keys, native().conv_wt_flip_multi([pend[k] for k in keys])):
            _FLIP["done"][k] = t
        pend.clear()
        wt = _FLIP["done"][key]
    return wt


# ---- a block tail's backward apply fused with conv3's backward-data (TAIL_CONV3_BWD_FUSE) ----------
# conv3's forward leaves a Conv3Link (ops/handover.py) on its output x3 and on its own ctx.  The
# tail's backward (ops/bn.py) finds it through x3, launches the fused kernel itself - it never returns
# an unfilled dx3 - and stashes conv3's input gradient in the link; conv3's backward takes the stash
# when the dy autograd hands it is that very dx3, unmodified, in the same step generation.


def _tail_link(x, w, stride, pad, out_hw, bn_src):
    """The link of an eligible conv3: native 1x1 / stride 1 / unpadded with statistics output whose
    input comes from a fused BN+ReLU (``bn_src.coef``), else None."""
    if not (TAIL_CONV3_BWD_FUSE and BN_BWD_FUSE and torch.is_grad_enabled() and x.requires_grad):
        return None
    if not (int(stride) == 1 and int(pad) == 0 and tuple(out_hw) == (0, 0) and w.shape[2] == 1 and w.shape[3] == 1):
        return None
    if bn_src is None or bn_src.is_tail:
        return None
    return Conv3Link(w, w._version, bn_src)


def tail_bwd_refusal(link, x3):
    """Why the tail on ``x3`` cannot run the linked conv3's backward-data (None: it can)."""
    if not TAIL_CONV3_BWD_FUSE:
        return "switched off"
    if link is None:
        return "no link"
    w = link.w
    if w._version != link.wv:
        return "the weight changed since the forward"
    if x3.dtype not in _DT16 or w.dtype != x3.dtype or tuple(w.shape) != (x3.shape[1], link.bn_src.x.shape[1], 1, 1):
        return "operand types or shapes"
    return native().conv1x1_tail_bwd_refusal(x3.numel() // x3.shape[1], x3.shape[1], w.shape[1])


def tail_bwd_apply(link, dz, x3, kbuf, mean, x2=None, mean2=None):
    """(dx3, dx_ds | None) of a tail whose finalize left ``kbuf``, filled when this returns: the fused
    launch, or - only when the binding itself refuses the launch after all - the apply pass(es) the
    finalize was for, noted as ``tail-bwd-refused``.  Any other error (layout, memory, device) is raised."""
    try:
        return tail_bwd_launch(link, dz, x3, kbuf, mean, x2, mean2)
    except RuntimeError as e:
        if "conv1x1_tail_bwd: " not in str(e) and "tail_conv3_bwd: " not in str(e):
            raise
    e0 = _mark()
    c4 = x3.shape[1]
    dx3 = native().bn_bwd_apply_pre(dz, x3, mean, kbuf[:3 * c4])
    dx_ds = None if x2 is None else native().bn_bwd_apply_pre(dz, x2, mean2, kbuf[3 * c4:])
    _note("dgrad", link.bn_src.x, link.w, 1, 0, "tail-bwd-refused", e0)
    return dx3, dx_ds


def tail_bwd_launch(link, dz, x3, kbuf, mean, x2=None, mean2=None):
    """The fused launch for a tail whose finalize left ``kbuf``: (dx3, dx_ds | None), both filled;
    conv3's input gradient and bn2's statistics wait in the link for conv3's backward."""
    w, src = link.w, link.bn_src
    wt = _flipped(w)
    if wt is None:   # no per-step flip cache (outside the trainer)
        wt = native().conv_wt_flip_multi([w])[0]
    e0 = _mark()
    dx3, dx_ds, dx, p1, p2 = native().conv1x1_tail_bwd(dz, x3, x2, kbuf, mean, mean2, wt, src.x, src.mean, src.coef)
    link.put_stash(dx3, dx, p1, p2)
    _note("dgrad", src.x, w, 1, 0, "tail-bwd-apply+dgrad", e0)
    return dx3, dx_ds


def _is_compact_of(dres, x) -> bool:
    """dres has the shape of a 1x1 / stride-2 conv's compact input gradient for the input x."""
    n, c, h, w = x.shape
    return (dres is not None and dres.dtype == x.dtype and dres.is_contiguous(memory_format=_CL)
            and tuple(dres.shape) == (n, c, (h + 1) // 2, (w + 1) // 2))


def _dres_ok(dres, x) -> bool:
    """dres can be folded into the backward-data of the conv whose input is x: x's dtype and layout,
    x's shape or its compact form (the caller knows which from the slot's ``dres_s2``)."""
    return (dres is not None and dres.dtype == x.dtype and (dres.shape == x.shape or _is_compact_of(dres, x))
            and dres.is_contiguous(memory_format=_CL))


class _Conv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride: int, pad: int, out_hw, bn_src, res_slot, compact_dres):
        e0 = _mark()
        y = native().conv_fwd(x, w, stride, pad, False, *out_hw)[0]
        _note("fwd", x, w, stride, pad, "plain", e0, out_hw)
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.pad, ctx.bn_src, ctx.res_slot = stride, pad, bn_src, res_slot
        ctx.compact_dres = compact_dres
        return y

    @staticmethod
    def backward(ctx, dy):
        return _backward(ctx, dy) + (None,) * 6


def materialize_tail(pending) -> None:
    """Fill a block tail's deferred output ``y`` (and its ReLU mask) with the apply kernel the tail
    itself would have launched (ops/bn.py TAIL_CONV1_FUSE), once."""
    if pending.done:
        return
    x3, r, coef, coef2 = pending.x3, pending.r, pending.coef, pending.coef2
    c = x3.shape[1]
    if coef2 is None:
        native().bn_apply(x3, r, coef[:c], coef[c:], True, mask_out=pending.mask, y_out=pending.y)
    else:
        native().bn_apply_aff(x3, r, coef, coef2, mask_out=pending.mask, y_out=pending.y)
    pending.done = True


def _tail_fwd(x, w, stride, pad, out_hw, pending):
    """The forward of a conv whose input ``x`` is a block tail's still unfilled output: one kernel
    writes ``x``, its mask and the conv output.  A conv the kernel refuses first materialises ``x``
    with the tail's own apply pass; None then, and the caller runs the plain forward."""
    if pending.y.data_ptr() != x.data_ptr() or tuple(out_hw) != (0, 0):
        materialize_tail(pending)
        return None
    try:
        out = native().conv1x1_tail_fwd(pending.x3, pending.r, pending.coef, pending.coef2, w, x,
                                        pending.mask, stride, pad)
    except RuntimeError:
        materialize_tail(pending)
        return None
    pending.done = True
    return out


class _ConvStats(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, stride: int, pad: int, out_hw, bn_src, res_slot, compact_dres, pending, link=None):
        e0 = _mark()
        fused = _tail_fwd(x, w, stride, pad, out_hw, pending) if pending is not None else None
        if fused is not None:
            y, ps, pq = fused
            _note("fwd", x, w, stride, pad, "tail-apply+stats", e0, out_hw)
        else:
            y, ps, pq = native().conv_fwd(x, w, stride, pad, True, *out_hw)
            _note("fwd", x, w, stride, pad, "stats", e0, out_hw)
        ctx.save_for_backward(x, w)
        ctx.stride, ctx.pad, ctx.bn_src, ctx.res_slot = stride, pad, bn_src, res_slot
        ctx.compact_dres = compact_dres
        ctx.tail_link = link
        ctx.mark_non_differentiable(ps, pq)
        ctx.set_materialize_grads(False)  # no zero-filled gradients for the statistics outputs
        return y, ps, pq

    @staticmethod
    def backward(ctx, dy, _dps, _dpq):
        return _backward(ctx, dy) + (None,) * 8


def conv2d(x: torch.Tensor, w: torch.Tensor, stride: int, pad: int, bn_stats: bool = False,
           out_hw=(0, 0)) -> torch.Tensor:
    """y = conv2d(x, w, stride, pad) on the MFMA kernels; ``bn_stats`` attaches the output's
    BatchNorm partial sums as ``y._dpt_bn_partials`` (consumed by ops/bn.py).  ``out_hw``:
    explicit output size (asymmetric padding: top/left ``pad``, bottom/right what fits)."""
    w = _cl(w)
    # the tail that produced x already ran this very conv on it, fused with its apply pass
    # (ops/bn.py TAIL_CONV1_FUSE): hand that result over
    done = x.__dict__.pop("_dpt_conv1_out", None)
    if done is not None and done.w is w and (done.stride, done.pad, done.bn_stats) == (
            int(stride), int(pad), bool(bn_stats)) and tuple(out_hw) == (0, 0):
        return done.y
    # x is a block tail's output that is not filled yet: this conv's forward fills it
    pending = x.__dict__.pop("_dpt_tail_pending", None)
    if pending is not None and not bn_stats:
        materialize_tail(pending)
        pending = None
    if _FLIP["on"] and int(stride) == 1 and x.requires_grad:
        _FLIP["pending"].setdefault((w.data_ptr(), tuple(w.shape)), w)
    # the fused BN+ReLU or block tail that produced x, if any (ops/bn.py)
    bn_src = x.__dict__.get("_dpt_bn_src")
    # x is the identity alias of a fused block tail (this conv is a downsample)
    res_slot = x.__dict__.get("_dpt_res_slot")
    one_by_one = w.shape[2] == 1 and w.shape[3] == 1
    if (int(stride) == 1 and one_by_one and BN_BWD_FUSE and bn_src is not None and bn_src.is_tail
            and not bn_src.has_downsample):
        # a 1x1 / stride-1 conv on a block tail's conv-path output: its backward-data folds the
        # identity-path gradient (BNR), a stride-2 downsample conv's compact one included - told to
        # that conv (which runs after this one, models/resnet.py) through the shared slot
        bn_src.slot.fold_s2 = True
    compact_dres = bool(S2_COMPACT_DRES and S2_DGRAD and int(stride) == 2 and one_by_one and int(pad) == 0
                        and tuple(out_hw) == (0, 0) and res_slot is not None and res_slot.fold_s2)
    if not bn_stats:
        return _Conv.apply(x, w, int(stride), int(pad), tuple(out_hw), bn_src, res_slot, compact_dres)
    link = _tail_link(x, w, stride, pad, out_hw, bn_src)
    y, ps, pq = _ConvStats.apply(x, w, int(stride), int(pad), tuple(out_hw), bn_src, res_slot, compact_dres,
                                 pending, link)
    y._dpt_bn_partials = (ps, pq)
    if link is not None:
        y._dpt_tail_link = link
    if pending is not None:  # fused or not, y is the result of this conv on the filled x
        pending.conv = Conv1Out(w, int(stride), int(pad), True, y)
    return y


def take_bn_partials(x: torch.Tensor):
    """The (psum, psq) partials a native conv attached to ``x``, once (None otherwise)."""
    part = x.__dict__.pop("_dpt_bn_partials", None)
    return part


def s2d_stem_supported(x: torch.Tensor, w: torch.Tensor, stride, padding, dilation, groups) -> bool:
    """ResNet's 7x7/2 pad-3 stem on <= 4 input channels: space-to-depth + 4x4 MFMA conv."""
    if not (ENABLED and x.is_cuda and native_available() and x.dim() == 4 and groups == 1
            and x.dtype in (torch.float32, torch.bfloat16) and w.dtype in _DT16):
        return False
    cout, cin, r, s = w.shape
    return (cin <= 4 and cout % 64 == 0 and (r, s) == (7, 7) and tuple(stride) == (2, 2)
            and tuple(padding) == (3, 3) and tuple(dilation) == (1, 1) and not x.requires_grad
            and x.shape[1] == cin and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0
            and x.is_contiguous(memory_format=_CL))


def s2d_stem_conv2d(x: torch.Tensor, w: torch.Tensor, bn_stats: bool = False) -> torch.Tensor:
    """7x7 / stride 2 / pad 3 conv as a 4x4 / stride 1 conv on the 2x2 space-to-depth image.

    With r = 2r' + a - 1 and s = 2s' + b - 1 (r', s' in 0..3, a, b in {0, 1}; tap -1 has zero
    weight) the input row 2*ho - 3 + r is 2*(ho - 2 + r') + a, so
    y[ho, wo] = sum_{r', s'} X2[ho - 2 + r', wo - 2 + s'] . W2[r', s']  with
    X2[i, j, (a*2 + b)*4 + c] = x[2i + a, 2j + b, c] and W2[r', s', (a*2+b)*4 + c] = w[2r'+a-1, 2s'+b-1, c]:
    K = 4*4*16 = 256, each 64-wide K-step four consecutive pixels of one row (the kernels' narrow-
    input path), top/left padding 2, output H/2 x W/2.  The weight re-indexing is plain torch ops,
    so autograd maps the 4x4 weight gradient back onto the 7x7 one."""
    cout, cin = w.shape[0], w.shape[1]
    x2 = native().space_to_depth2(x, w.dtype == torch.float16)
    wk = torch.nn.functional.pad(w.permute(0, 2, 3, 1), (0, 4 - cin, 1, 0, 1, 0))       # [Co, 8, 8, 4]
    w2 = wk.reshape(cout, 4, 2, 4, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(cout, 4, 4, 16)
    w2 = w2.permute(0, 3, 1, 2)                                                         # [Co, 16, 4, 4] cl
    return conv2d(x2, w2, 1, 2, bn_stats, out_hw=(x.shape[2] // 2, x.shape[3] // 2))


def stem_supported(x: torch.Tensor, w: torch.Tensor, stride, padding, dilation, groups) -> bool:
    """Narrow-input conv (any kernel/stride) on the im2col + MFMA GEMM path."""
    if not (ENABLED and x.is_cuda and native_available() and x.dim() == 4 and groups == 1
            and x.dtype in (torch.float32, torch.bfloat16) and w.dtype == torch.bfloat16):
        return False
    cout, cin, r, s = w.shape
    return (cin < 64 and cout % 64 == 0 and not x.requires_grad and tuple(dilation) == (1, 1)
            and stride[0] == stride[1] and padding[0] == padding[1] and x.shape[1] == cin
            and x.is_contiguous(memory_format=_CL))


def stem_conv2d(x: torch.Tensor, w: torch.Tensor, stride: int, pad: int, bn_stats: bool = False) -> torch.Tensor:
    """conv2d for a narrow input that needs no input gradient: one im2col kernel writes the
    [pixels, Kp] bf16 patch matrix (Kp = R*S*Cin rounded up to 64, zero-padded), then the 1x1
    MFMA conv (GEMM) with the weight flattened to [Cout, R*S*Cin] (KRSC order) and zero-padded
    - its backward-weight is the 1x1 split-K kernel on the saved patch matrix."""
    cout, cin, r, s = w.shape
    k = r * s * cin
    kp = (k + 63) // 64 * 64
    a = native().im2col(x, r, s, int(stride), int(pad), kp)
    wf = torch.nn.functional.pad(w.permute(0, 2, 3, 1).reshape(cout, k), (0, kp - k))
    return conv2d(a, wf.view(cout, kp, 1, 1), 1, 0, bn_stats)
