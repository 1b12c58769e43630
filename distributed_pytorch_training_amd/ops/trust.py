"""Segment table of the layer-wise adaptive optimizers (LARS, LAMB).

The fused SGD / Adam kernels sweep the flat arena blindly.  A trust ratio needs a norm per
parameter, so the device has to know where one parameter ends and the next begins.  Each
parameter is a *segment* ``[offset, offset + numel)``; every segment is cut into chunks of
``TRUST_CHUNK`` elements counted from the segment's own start, so no chunk crosses a segment
boundary and a chunk's contents do not depend on where the segment lies in the arena.

Per chunk: ``(start, length, segment id, 0)``.  Per segment: first chunk, chunk count and a flag
word (``ADAPT``: apply the trust ratio, ``DECAY``: apply weight decay).

The kernels read whole float4s: a segment's end is rounded up to 4 elements.  Segments start on
16-element boundaries (parallel/flat.py), so the rounding never reaches the next segment, and
the padding it covers is zero in parameters, gradients and state and stays zero.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

TRUST_CHUNK = 4096          # mirrors kTrustChunk (csrc/kernels/kernels.h); checked in ops/__init__.py
ADAPT, DECAY = 1, 2


def flags_for(params: Sequence[torch.Tensor], adapt_1d: bool = False) -> List[int]:
    """The 1-D rule: biases and norm weights (``ndim <= 1``) get neither a trust ratio nor weight
    decay unless ``adapt_1d``."""
    return [ADAPT | DECAY if (adapt_1d or p.ndim > 1) else 0 for p in params]


def cut_chunks(offsets: Sequence[int], numels: Sequence[int], chunk: int = TRUST_CHUNK
               ) -> Tuple[List[Tuple[int, int, int]], List[int], List[int]]:
    """``(chunks, seg_first, seg_count)``: chunks are ``(start, length, segment)``."""
    chunks: List[Tuple[int, int, int]] = []
    seg_first: List[int] = []
    seg_count: List[int] = []
    for seg, (off, n) in enumerate(zip(offsets, numels)):
        if n < 1:
            raise ValueError(f"segment {seg} is empty")
        seg_first.append(len(chunks))
        for s in range(0, n, chunk):
            chunks.append((off + s, min(chunk, n - s), seg))
        seg_count.append(len(chunks) - seg_first[-1])
    return chunks, seg_first, seg_count


@dataclass
class TrustTable:
    """Host lists (the CPU reference walks them) and, for a GPU arena, their device copies."""
    offsets: List[int]
    numels: List[int]
    flags: List[int]
    numel: int                                   # arena length the table was validated against
    chunks: List[Tuple[int, int, int]]
    seg_first: List[int]
    seg_count: List[int]
    ratio: torch.Tensor                          # [segments] fp32, written by every step
    partial: Optional[torch.Tensor] = None       # [chunks, 2] fp32 (GPU only)
    device_tensors: Tuple[torch.Tensor, ...] = field(default_factory=tuple)

    @property
    def nseg(self) -> int:
        return len(self.offsets)

    @property
    def nchunks(self) -> int:
        return len(self.chunks)


def build_table(offsets: Sequence[int], numels: Sequence[int], flags: Sequence[int], arena_numel: int,
                device, native=None) -> TrustTable:
    offsets, numels, flags = [int(o) for o in offsets], [int(n) for n in numels], [int(f) for f in flags]
    if not (len(offsets) == len(numels) == len(flags)) or not offsets:
        raise ValueError("offsets, numels and flags must be equally long and non-empty")
    end = 0
    for i, (off, n, fl) in enumerate(zip(offsets, numels, flags)):
        if off % 4 != 0 or off < end:
            raise ValueError(f"segment {i} at {off} overlaps its predecessor or is not 4-element aligned")
        if fl & ~(ADAPT | DECAY):
            raise ValueError(f"segment {i}: unknown flag bits {fl:#x}")
        end = off + (n + 3) // 4 * 4
        if n < 1 or end > arena_numel:
            raise ValueError(f"segment {i} [{off}, {off + n}) does not fit an arena of {arena_numel}")
    chunks, seg_first, seg_count = cut_chunks(offsets, numels)
    device = torch.device(device)
    table = TrustTable(offsets, numels, flags, int(arena_numel), chunks, seg_first, seg_count,
                       ratio=torch.ones(len(offsets), dtype=torch.float32, device=device))
    if device.type == "cuda":
        if native is None:
            raise RuntimeError("a GPU segment table needs the native extension")
        i32 = lambda rows: torch.tensor(rows, dtype=torch.int32)
        table.device_tensors = tuple(native.trust_segments(
            i32([(s, n, g, 0) for s, n, g in chunks]).reshape(-1, 4), i32(seg_first), i32(seg_count),
            i32(flags), int(arena_numel), table.ratio))
        table.partial = torch.zeros(len(chunks), 2, dtype=torch.float32, device=device)
    return table
