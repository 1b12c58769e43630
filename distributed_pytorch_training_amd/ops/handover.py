"""The records one op's forward or backward leaves for another (ops/conv.py, ops/bn.py, ops/pool.py)
and the per-step state that keeps a stale one from being honoured.  Carried on tensors:
``_dpt_bn_src`` (BnSource), ``_dpt_res_slot`` (TailSlot), ``_dpt_tail_pending`` (TailPending),
``_dpt_tail_link`` (Conv3Link), ``_dpt_conv1_out`` (Conv1Out).  Imports nothing from the op modules.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, NamedTuple, Optional

# The step generation: a record made in one is never honoured in another (reset_side_channels)
_GEN = [0]
# dx.data_ptr() -> _BnbEntry: from the backward that wrote dx to the BN backward that receives dx as
# its output gradient (ops/bn.py), consumed once
_BNB_PARTIALS = {}
# id -> Conv3Link holding a stash (dropped by reset_side_channels)
_TAIL_STASHED = {}

# dres_ptr of an entry whose gradient is a block tail's already-masked gradient with no
# identity-path gradient folded in (the last tail, whose output only fed the average pool)
MASKED_NO_RES = -1
# dres_ptr of an entry whose gradient is a block tail's masked gradient with a downsample conv's
# compact identity-path gradient folded in (S2_COMPACT_DRES): autograd delivers no second gradient
COMPACT_RES = -2


class TensorStamp(NamedTuple):
    """What a hand-over remembers of the tensor it was made for; ``gen``: the step generation."""
    ptr: int
    version: int
    gen: int
    shape: tuple

    def matches(self, t) -> bool:
        """``t`` is that tensor, unmodified (autograd accumulating a second gradient into it in place
        bumps the version), in this step generation."""
        return (self.ptr == t.data_ptr() and self.version == t._version and self.gen == _GEN[0]
                and self.shape == tuple(t.shape))


def stamp_of(t) -> TensorStamp:
    return TensorStamp(t.data_ptr(), t._version, _GEN[0], tuple(t.shape))


@dataclass(slots=True, eq=False)
class TailSlot:
    """Shared by a block tail and the consumers of its two outputs: the tail's 1-bit ReLU mask and
    the identity-path gradient ``dres`` on its way to the conv-path conv's backward-data.  ``fold_s2``:
    that conv folds a stride-2 downsample conv's compact gradient; ``dres_s2``: ``dres`` is one."""
    mask: Any = None
    dres: Any = None
    dres_s2: bool = False
    fold_s2: bool = False

    def take_dres(self):
        dres, self.dres = self.dres, None
        return dres

    def take_dres_s2(self) -> bool:
        compact, self.dres_s2 = self.dres_s2, False
        return compact


@dataclass(slots=True, eq=False)
class BnSource:
    """The fused BatchNorm that produced a tensor, for the backward of whatever consumes it: a
    BN+ReLU (``coef``) or a block tail (``slot``; ``x2`` / ``mean2``: its downsample BatchNorm)."""
    x: Any
    mean: Any
    coef: Any = None
    slot: Optional[TailSlot] = None
    x2: Any = None
    mean2: Any = None

    def __post_init__(self):
        if (self.coef is None) == (self.slot is None):
            raise ValueError("BnSource: exactly one of coef (BN+ReLU) and slot (block tail)")

    @property
    def is_tail(self) -> bool:
        return self.slot is not None

    @property
    def has_downsample(self) -> bool:
        return self.x2 is not None


class Conv1Out(NamedTuple):
    """The output ``y`` of the conv a deferred tail ran on its own output (``_dpt_conv1_out``)."""
    w: Any
    stride: int
    pad: int
    bn_stats: bool
    y: Any


@dataclass(slots=True, eq=False)
class TailPending:
    """A block tail's apply pass left to the forward of the conv that reads its output ``y``
    (ops/bn.py TAIL_CONV1_FUSE); ``conv``: that conv's run, kept for the next block's call of it."""
    x3: Any = None
    r: Any = None
    coef: Any = None
    coef2: Any = None
    y: Any = None
    mask: Any = None
    done: bool = False
    conv: Optional[Conv1Out] = None

    def fill(self, x3, r, coef, coef2, y, mask) -> None:
        self.x3, self.r, self.coef, self.coef2, self.y, self.mask = x3, r, coef, coef2, y, mask


class TailStash(NamedTuple):
    """conv3's input gradient and bn2's statistics, written by the tail's backward for ``stamp``."""
    stamp: TensorStamp
    wv: int
    dx: Any
    p1: Any
    p2: Any


@dataclass(slots=True, eq=False)
class Conv3Link:
    """From a conv3 to the tail on its output (ops/conv.py TAIL_CONV3_BWD_FUSE); ``wv``: the weight's
    version at the forward, ``stash``: what the tail's backward left."""
    w: Any
    wv: int
    bn_src: BnSource
    stash: Optional[TailStash] = None

    def put_stash(self, dx3, dx, p1, p2) -> None:
        self.stash = TailStash(stamp_of(dx3), self.w._version, dx, p1, p2)
        _TAIL_STASHED[id(self)] = self

    def take_stash(self, dy, w) -> Optional[TailStash]:
        """The stash left for the conv whose output gradient is ``dy``, once; None when there is none
        or it was made for another tensor, version, step generation or weight."""
        ent, self.stash = self.stash, None
        if ent is None:
            return None
        _TAIL_STASHED.pop(id(self), None)
        if not ent.stamp.matches(dy) or ent.wv != w._version or self.w.data_ptr() != w.data_ptr():
            return None
        return ent


class TailLinks(NamedTuple):
    """A fused BatchNorm op's neighbours: its own slot (block tails), the slot of the tail whose
    identity alias is its residual, a deferred apply pass, the conv3 before it."""
    own_slot: Optional[TailSlot] = None
    res_slot: Optional[TailSlot] = None
    defer: Optional[TailPending] = None
    conv3: Optional[Conv3Link] = None


class BnbPartials(NamedTuple):
    """p1, p2: the BN backward statistics; dres_ptr: None for BN+ReLU, else the data pointer of the
    identity-path gradient folded into the gradient (block tails), or MASKED_NO_RES / COMPACT_RES;
    p3: the folded downsample BN's statistic (tails with a downsample branch), else None."""
    p1: Any
    p2: Any
    dres_ptr: Optional[int]
    p3: Any


class _BnbEntry(NamedTuple):
    stamp: TensorStamp
    part: BnbPartials


def reset_side_channels() -> None:
    """New step generation: forget every hand-over not consumed so far (an aborted backward), so a
    reused allocation can never pick up stale statistics."""
    _GEN[0] += 1
    _BNB_PARTIALS.clear()
    for link in _TAIL_STASHED.values():
        link.stash = None
    _TAIL_STASHED.clear()


def _put_bnb(dx, p1, p2, dres_ptr, p3) -> None:
    _BNB_PARTIALS[dx.data_ptr()] = _BnbEntry(stamp_of(dx), BnbPartials(p1, p2, dres_ptr, p3))


def register_bnb_partials(dx, p1, p2, masked: bool = False) -> None:
    """Hand BN backward-statistics partials summed by dx's producer to the BN backward that
    receives dx as its output gradient (other producers than convs: the stem pool for BN+ReLU;
    the average-pool backward for the last block tail, ``masked``: dx is already dz)."""
    _put_bnb(dx, p1, p2, MASKED_NO_RES if masked else None, None)


def take_bnb_partials(dy) -> Optional[BnbPartials]:
    """What the backward that wrote ``dy`` summed for it, once; None when there is nothing or it was
    made for another version, step generation or shape of that storage."""
    if not _BNB_PARTIALS:
        return None
    ent = _BNB_PARTIALS.pop(dy.data_ptr(), None)
    if ent is None or not ent.stamp.matches(dy):
        return None
    return ent.part
