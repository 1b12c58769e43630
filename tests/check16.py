"""Half-ulp checker and fp64 references shared by the kernel edge tests (plain module, no fixtures).

A kernel that computes in fp32 and rounds once to a 16-bit type can be at most half a 16-bit ulp
plus its fp32 evaluation error away from the exact result.  ``check16`` asserts exactly that, so
the tolerance follows the magnitude of every element instead of one rtol/atol pair sized for the
largest of them.
"""
from __future__ import annotations

import math

import torch

# (mantissa bits, minimum normal exponent)
_FMT = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}
KIND = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
DTYPE = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}


def ulp16(ref64: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Spacing of ``dtype`` (bf16 / fp16) at |ref|, in fp64.  The exponent is clamped at the
    type's minimum normal exponent: every fp16 subnormal (and zero) has spacing 2^-24."""
    mant, emin = _FMT[dtype]
    a = ref64.double().abs()
    _, e = torch.frexp(a)                      # a = m * 2^e, m in [0.5, 1)  ->  floor(log2 a) = e - 1
    e = torch.where(a > 0, e.to(torch.int64) - 1, torch.full_like(e, emin, dtype=torch.int64))
    e = e.clamp(min=emin)
    return torch.ldexp(torch.ones_like(a), (e - mant).to(torch.int32))


def gelu64(z: torch.Tensor) -> torch.Tensor:
    """Exact GELU in fp64, in the erfc form (no 1 + erf cancellation in the negative tail)."""
    z = z.double()
    return 0.5 * z * torch.special.erfc(-z / math.sqrt(2.0))


def dgelu64(z: torch.Tensor) -> torch.Tensor:
    z = z.double()
    return 0.5 * torch.special.erfc(-z / math.sqrt(2.0)) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def check16(out: torch.Tensor, ref64: torch.Tensor, slack, inp: torch.Tensor | None = None, what: str = "") -> None:
    """|out - ref64| <= 0.5 * ulp16(ref64, out.dtype) + slack, elementwise.  ``slack`` is a number
    or a tensor broadcastable to ``ref64``; ``inp`` (optional) is reported with the worst element."""
    assert out.dtype in _FMT, out.dtype
    ref64 = ref64.double()
    assert out.shape == ref64.shape, (what, tuple(out.shape), tuple(ref64.shape))
    slack = torch.as_tensor(slack, dtype=torch.float64, device=ref64.device).expand(ref64.shape)
    err = (out.double() - ref64).abs()
    bound = 0.5 * ulp16(ref64, out.dtype) + slack
    bad = ~(err <= bound)                      # a NaN in out is bad
    if not bool(bad.any()):
        return
    excess = torch.where(bad, torch.nan_to_num(err - bound, nan=math.inf, posinf=math.inf), torch.zeros_like(err))
    flat = int(excess.flatten().argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ref64.shape)) if ref64.dim() else ()
    msg = (f"{what or 'check16'} ({out.dtype}): {int(bad.sum())} of {bad.numel()} elements beyond half an ulp + slack; "
           f"worst at {idx}: out {out[idx].item()!r} ref {ref64[idx].item()!r} err {err[idx].item():.3e} "
           f"bound {bound[idx].item():.3e} (ulp {2 * (bound[idx] - slack[idx]).item():.3e}, slack {slack[idx].item():.3e})")
    if inp is not None:
        msg += f" input {inp.expand(ref64.shape)[idx].item()!r}"
    raise AssertionError(msg)


def all_finite16(dtype: torch.dtype, max_abs: float | None = None) -> torch.Tensor:
    """Every finite value of a 16-bit type (both zeros included), optionally only |v| <= max_abs."""
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    keep = torch.isfinite(v.float())
    if max_abs is not None:
        keep &= v.float().abs() <= max_abs
    return v[keep]
