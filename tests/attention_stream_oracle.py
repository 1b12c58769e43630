"""Rounding model of the streaming attention kernels (csrc/kernels/attn_stream_kernels.hip) in
fp64, next to ``attention_oracle`` (the fp64 reference, the bounds and the data kinds, which hold
unchanged: the arithmetic is the same, only the softmax is split).  A helper, not a test.

``model`` walks the keys in chunks as the forward kernel does: the running maximum ``m`` of the
raw fp32 scores, P of a chunk taken against the maximum *so far* and rounded to bf16 as the MFMA
operand, ``l`` summed from the unrounded P, and ``o`` / ``l`` rescaled by the fp32 factor
``exp2((m_old - m_new) * scale_log2)`` and kept in fp32 between chunks.  The backward recomputes P
from ``lse2`` and so does not depend on the chunking; it is ``attention_oracle.model``'s.

``mirror`` turns the ``lastkey`` kind (dominant key at S-1: every earlier chunk is rescaled) into
its mirror image (dominant key at 0: every later chunk is added under an old maximum).
"""
import torch

import attention_oracle as ao


def _f32(x):
    return x.float().double()


def model(qkv, dout, heads, scale, chunk):
    """-> out [B,S,H*64], lse2 [B,H,S], dqkv [B,S,3*H*64] (laid out as ``attention_oracle.reference``)."""
    q, k, v = ao.split_heads(qkv.detach().double(), heads)
    do = ao._heads_of(dout.double(), heads)
    sl2 = scale * ao.LOG2E
    s = _f32(q @ k.transpose(-1, -2))                      # raw scores leave the MFMA as fp32
    b, h, sq, _ = q.shape
    m = torch.full((b, h, sq, 1), float("-inf"), dtype=torch.float64, device=q.device)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for c0 in range(0, sq, chunk):
        sc = s[..., c0:c0 + chunk]
        m_new = torch.maximum(m, sc.amax(-1, keepdim=True))
        alpha = _f32(torch.exp2((m - m_new) * sl2))        # first chunk: exp2(-inf) = 0
        p = torch.exp2((sc - m_new) * sl2)
        l = _f32(l * alpha + p.sum(-1, keepdim=True))
        o = _f32(_f32(o * alpha) + ao.bf16(p) @ v[..., c0:c0 + chunk, :])
        m = m_new
    out = ao.bf16(o / l)
    lse2 = _f32(m * sl2 + torch.log2(l))
    # backward: attention_oracle.model's, from this forward's lse2 and bf16 output
    d = (do * out).sum(-1, keepdim=True)
    pb = torch.exp2(s * sl2 - lse2)
    ds = pb * (do @ v.transpose(-1, -2) - d)
    dv = ao.bf16(ao.bf16(pb).transpose(-1, -2) @ do)
    dk = ao.bf16(scale * (ao.bf16(ds).transpose(-1, -2) @ q))
    dq = ao.bf16(scale * (ao.bf16(ds) @ k))
    dqkv = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(b, sq, 3 * h * 64)
    return ao.merge_heads(out), lse2.squeeze(-1), dqkv


def mirror(qkv, dout):
    """The same problem with the sequence reversed (key S-1 becomes key 0), contiguous."""
    return qkv.flip(1).contiguous(), dout.flip(1).contiguous()


def dominant_probability(qkv, heads, scale, key):
    """Smallest fp64 softmax probability, over all queries, of key ``key``."""
    q, k, _ = ao.split_heads(qkv.detach().double(), heads)
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    return p[..., key].min().item()
