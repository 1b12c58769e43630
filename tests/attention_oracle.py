"""fp64 oracle, rounding model and worst-case error bounds for the fused attention kernels
(csrc/kernels/attn_kernels.hip).  A helper, not a test: plain torch, CPU or GPU tensors.

Layouts follow the kernel: ``qkv`` is ``[B, S, 3*H*64]`` (= ``[B, S, 3, H, 64]``), ``out`` / ``dout``
are ``[B, S, H*64]``, ``lse2`` and ``p`` are per head (``[B, H, S]``, ``[B, H, S, S]``).

``reference``  everything in fp64 from the exact bf16 input values (gradient by fp64 autograd).
``bounds``     first-order worst-case rounding bounds of the kernel's stated arithmetic: bf16
               operands, P and dS rounded to bf16 before they become MFMA operands, fp32
               accumulation, bf16 outputs.  With u = 2^-8 (bf16 unit round-off):
                 out = bf16(bf16(P) V / l)        two roundings of relative size u over terms of
                                                  size p|v|:        E_out = 2u (p @ |v|)
                 dV  = bf16(bf16(P)^T dO)         E_dV = u (p^T @ |dO|) + u |dV|
                 D   = rowsum(dO * bf16(O))       |D - D_exact| <= u A,  A[q] = sum_d |dO||O|
                 dS  = P (dP - D), then bf16      |dS - dS_exact| <= u (|dS| + p A) = u W
                 dK  = bf16(scale bf16(dS)^T Q)   E_dK = u scale (W^T @ |q|) + u |dK|
                 dQ  = bf16(scale bf16(dS) K)     E_dQ = u scale (W @ |k|) + u |dQ|
               (fp32 accumulation, <= 256 terms at 2^-24, and second-order terms are left to the
               caller's factor over the bound.)
``model``      the kernel's rounding points emulated in fp64 (everything else exact); it exists to
               show on the CPU that the bounds are reachable (tests/test_attention_oracle_cpu.py).
``inputs``     the data families the tests sweep.
"""
import torch

U = 2.0 ** -8          # bf16 unit round-off
LOG2E = 1.4426950408889634
# The bounds are relative-error bounds; they do not cover underflow.  A probability below fp32's
# normal range (2^-126 = 1.2e-38, the `peaked` kind has them) flushes to zero in the bf16 operand
# while its fp64 value, and so its u * p bound, is 1e-41 and smaller.  Every comparison therefore
# allows this absolute slack, thirty orders of magnitude below any output here.
TINY = 1e-30
KINDS = ("gauss", "peaked", "negative", "lastkey", "uniform")


def split_heads(qkv, heads):
    """[B, S, 3*H*64] -> q, k, v, each [B, H, S, 64] (views)."""
    b, s, _ = qkv.shape
    return qkv.view(b, s, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)


def merge_heads(x):
    """[B, H, S, 64] -> [B, S, H*64]."""
    b, h, s, d = x.shape
    return x.transpose(1, 2).reshape(b, s, h * d)


def _heads_of(x, heads):
    """[B, S, H*64] -> [B, H, S, 64]."""
    b, s, _ = x.shape
    return x.view(b, s, heads, 64).transpose(1, 2)


def bf16(x):
    """Round an fp64 tensor to bf16 (through fp32, as the kernel's conversions do) and back."""
    return x.float().bfloat16().double()


def reference(qkv, dout, heads, scale):
    """-> out [B,S,H*64], lse2 [B,H,S], dqkv [B,S,3*H*64], p [B,H,S,S]; all fp64."""
    x = qkv.detach().double().requires_grad_(True)
    q, k, v = split_heads(x, heads)
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.softmax(s, dim=-1)
    out = merge_heads(p @ v)
    (dqkv,) = torch.autograd.grad(out, x, dout.double())
    lse2 = torch.logsumexp(s.detach(), dim=-1) * LOG2E
    return out.detach(), lse2, dqkv, p.detach()


def bounds(qkv, dout, heads, scale):
    """-> E_out, E_dQ, E_dK, E_dV, each [B, S, H*64] fp64 (see the module docstring)."""
    q, k, v = split_heads(qkv.detach().double(), heads)
    do = _heads_of(dout.double(), heads)
    p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    o = p @ v
    d = (do * o).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-1, -2) - d)
    a = (do.abs() * o.abs()).sum(-1, keepdim=True)
    w = ds.abs() + p * a
    dv = p.transpose(-1, -2) @ do
    dk = scale * (ds.transpose(-1, -2) @ q)
    dq = scale * (ds @ k)
    e_out = 2 * U * (p @ v.abs())
    e_dv = U * (p.transpose(-1, -2) @ do.abs()) + U * dv.abs()
    e_dk = U * scale * (w.transpose(-1, -2) @ q.abs()) + U * dk.abs()
    e_dq = U * scale * (w @ k.abs()) + U * dq.abs()
    return merge_heads(e_out), merge_heads(e_dq), merge_heads(e_dk), merge_heads(e_dv)


def model(qkv, dout, heads, scale):
    """The kernel's rounding points in fp64 -> out, lse2, dqkv (laid out as in ``reference``)."""
    q, k, v = split_heads(qkv.detach().double(), heads)
    do = _heads_of(dout.double(), heads)
    sl2 = scale * LOG2E
    s = (q @ k.transpose(-1, -2)).float().double()          # raw scores leave the MFMA as fp32
    m = s.amax(-1, keepdim=True)
    p = torch.exp2((s - m) * sl2)
    l = p.sum(-1, keepdim=True)                             # summed from the unrounded p
    out = bf16((bf16(p) @ v) / l)
    lse2 = m * sl2 + torch.log2(l)
    # backward: P recomputed from lse2, D from the bf16 output
    d = (do * out).sum(-1, keepdim=True)
    pb = torch.exp2(s * sl2 - lse2)
    ds = pb * (do @ v.transpose(-1, -2) - d)
    dv = bf16(bf16(pb).transpose(-1, -2) @ do)
    dk = bf16(scale * (bf16(ds).transpose(-1, -2) @ q))
    dq = bf16(scale * (bf16(ds) @ k))
    b, h, sq, _ = q.shape
    dqkv = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(b, sq, 3 * h * 64)
    return merge_heads(out), lse2.squeeze(-1), dqkv


def inputs(kind, B, S, H, seed):
    """bf16 qkv [B, S, 3*H*64] and dout [B, S, H*64] on the CPU, from a seeded CPU generator.

    gauss     x * 1.5 (the data of test_attention_fwd_bwd_matches_fp32)
    peaked    x * 6: scaled scores of std ~36, exp2 overflows fp32 without the row-max
              subtraction, softmax near one-hot
    negative  q = 0.3 x_q + 13 u, k = 0.3 x_k - 13 u: every scaled score near -21, so a wrongly
              admitted padding key (score 0) takes the whole softmax
    lastkey   q = 0.3 x_q + 8 u, k = 0.3 x_k, plus 12 u on key S-1 only: the last key dominates every
              query (p > 0.9), masking one key too many changes every output.  (12, not 8: the
              last key's lead is 8 * 12 * scale = 12 at scale 1/8 less ~3 of noise, and p > 0.9
              against 255 other keys needs ln(9 * 255) = 7.7; a lead of 8 * 8 / 8 = 8 gives
              p ~ 0.75 at S >= 129.)
    uniform   every key equal to one random row: p == 1/S exactly, out = mean(V),
              lse2 = s * scale * log2(e) + log2(S); counts keys
    """
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, 3, H, 64, generator=g)
    u64 = torch.randn(64, generator=g)
    u64 = u64 / u64.norm()
    dout = torch.randn(B, S, H * 64, generator=g)
    if kind == "gauss":
        x = x * 1.5
    elif kind == "peaked":
        x = x * 6
    elif kind == "negative":
        x[:, :, 0] = 0.3 * x[:, :, 0] + 13 * u64
        x[:, :, 1] = 0.3 * x[:, :, 1] - 13 * u64
    elif kind == "lastkey":
        x[:, :, 0] = 0.3 * x[:, :, 0] + 8 * u64
        x[:, :, 1] = 0.3 * x[:, :, 1]
        x[:, S - 1, 1] += 12 * u64
    elif kind == "uniform":
        x[:, :, 1] = x[:, :1, 1]
    else:
        raise ValueError(kind)
    return x.reshape(B, S, 3 * H * 64).bfloat16(), dout.bfloat16()


def split_dqkv(dqkv, heads):
    """[B, S, 3*H*64] -> dQ, dK, dV, each [B, S, H*64]."""
    b, s, _ = dqkv.shape
    return dqkv.view(b, s, 3, heads * 64).unbind(2)


def worst_ratio(got, want, bound):
    """max over elements of (|got - want| - TINY) / bound, so ``worst_ratio(..) <= f`` is
    ``|got - want| <= f * bound + TINY`` elementwise."""
    err = ((got.double() - want).abs() - TINY).clamp(min=0)
    return (err / bound.clamp(min=1e-300)).max().item() if err.numel() else 0.0
