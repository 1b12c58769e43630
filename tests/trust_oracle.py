"""fp64 oracle and derived rounding bounds for the LARS / LAMB arena steps
(csrc/kernels/trust_kernels.hip, ops/reference.py).  A helper, not a test: plain torch and numpy,
nothing imported from the extension.

Oracle.  ``lars_oracle`` / ``lamb_oracle`` run one step per segment in fp64 on flat CPU tensors.
Hyper-parameters are first rounded as the kernels receive them (fp32; LAMB's ``1 - beta`` and the
bias corrections are formed in double and rounded once), so what separates the oracle from the
kernels is the kernels' fp32 arithmetic alone.  Given ``ratios`` the oracle applies those instead
of its own: the elementwise checks use the kernel's read-back ratios, the ratio check compares the
ratios themselves.

Bound on a ratio.  ``u = 2^-24`` is fp32's unit round-off and ``gamma(k) = k u / (1 - k u)`` bounds
any product of k factors ``(1 + d)^(+-1)``, ``|d| <= u`` (Higham, Accuracy and Stability, Lemma 3.1);
``gamma(j) + gamma(k) + gamma(j) gamma(k) <= gamma(j + k)``, so factors are simply counted.

* A sum of squares.  Every term is non-negative, so the computed sum is
  ``sum x_i^2 (1 + e_i)`` and its relative error is at most the largest ``|e_i|``.  A term passes
  through ``L`` additions (the chain: squares added per thread, the levels of the two trees, the
  chunks added per lane, the last tree), one rounding of the square (none when fused) and, for
  the gradient, two for the rounding of ``g * factor`` before it is squared: ``L + 3`` factors.
  (An unscaled term, such as a weight, passes through ``L + 1``; the bound takes the larger count.)
* A norm is the square root: the ``L + 3`` factors are halved, the root itself is within one ulp,
  2 factors.  Two norms enter every ratio: ``L + 3`` factors from the sums, 4 from the roots.
* LARS, ``eta wn / (gn + wd wn)``: ``wd * wn``, the addition (both summands positive, so the
  relative errors do not grow) and ``eta * wn`` one factor each, the division 2: 5 more.

      |ratio - exact| / exact <= gamma(L + 12)                                  (LARS)

* LAMB, ``wn / un``: the division, 2 factors.  ``un`` is the norm of values the kernel computed
  itself: from the stored ``m``, ``v`` and ``p`` an element ``u_i = r_i + wd p_i`` carries
  ``m / bc1`` (2), ``v / bc2`` and the root of it (2/2 + 2), ``+ eps`` (1), the division (2), two
  for the bias corrections (pow in double on the device, rounded to fp32: the last bit may
  differ from the host's), then ``wd * p`` and the final addition one each.  The addition may
  cancel, so the error is relative to ``|r_i| + |wd p_i|``, not to ``|u_i|``:
  ``|u_i - exact| <= 11 u (|r_i| + |wd p_i|)`` and, by the triangle inequality on the norms,
  ``un`` moves by at most ``11 u A`` of itself, with ``A = || |r| + |wd p| || / || u ||`` a property
  of the inputs (1 without weight decay) that ``lamb_oracle`` returns per segment.

      |ratio - exact| / exact <= gamma(L + 9 + 11 A)                            (LAMB)

``chain_length`` is a Python mirror of the kernels' summation order and must change with them.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

U = 2.0 ** -24
BLOCK, WAVE = 256, 64            # kBlock and the wave width of trust_kernels.hip


def f32(x: float) -> float:
    return float(np.float32(x))


def gamma(k: float) -> float:
    return k * U / (1.0 - k * U)


def chain_length(numel: int, chunk: int) -> int:
    """Additions a term passes through: squares per thread (float4s t, t+256, ... of a chunk, four
    squares each), the wave's 6-level tree, the 2-level tree over the 4 waves, the chunks one lane
    of seg_finish adds (chunks l, l+64, ...), and its 6-level tree."""
    vecs = math.ceil(min(numel, chunk) / 4)
    per_thread = 4 * math.ceil(vecs / BLOCK)
    block_tree = int(math.log2(WAVE)) + int(math.log2(BLOCK // WAVE))
    chunks = math.ceil(numel / chunk)
    return per_thread + block_tree + math.ceil(chunks / WAVE) + int(math.log2(WAVE))


def lars_ratio_bound(numel: int, chunk: int) -> float:
    return gamma(chain_length(numel, chunk) + 12)


def lamb_ratio_bound(numel: int, chunk: int, amplification: float) -> float:
    return gamma(chain_length(numel, chunk) + 9 + 11 * amplification)


def _d(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", torch.float64).clone()


def lars_oracle(p, g, buf, offsets: Sequence[int], numels: Sequence[int], flags: Sequence[int], *, lr,
                momentum, weight_decay, eta, nesterov, factor: float = 1.0, first: bool,
                ratios: Optional[Sequence[float]] = None):
    """One LARS step in fp64.  Returns ``(p, buf, ratios)``; elements outside the segments are
    returned unchanged."""
    p, g, buf = _d(p), _d(g), _d(buf)
    lr, mu, wd, eta, factor = f32(lr), f32(momentum), f32(weight_decay), f32(eta), f32(factor)
    out: List[float] = []
    for i, (off, n, fl) in enumerate(zip(offsets, numels, flags)):
        sl = slice(off, off + n)
        gi = g[sl] * factor
        wd_i = wd if fl & 2 else 0.0
        wn, gn = float(p[sl].norm()), float(gi.norm())
        r = eta * wn / (gn + wd_i * wn) if (fl & 1 and wn > 0 and gn > 0) else 1.0
        out.append(r)
        if ratios is not None:
            r = float(ratios[i])
        d = r * (gi + wd_i * p[sl])
        buf[sl] = d if first else mu * buf[sl] + d
        p[sl] = p[sl] - lr * (d + mu * buf[sl] if nesterov else buf[sl])
    return p, buf, out


def lamb_coefficients(beta1: float, beta2: float, t: int):
    """(1 - beta1, beta2, 1 - beta2, bc1, bc2) as the kernel holds them: formed in double, fp32."""
    return (f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(1.0 - beta1 ** t), f32(1.0 - beta2 ** t))


def lamb_direction(p, m, v, *, bc1, bc2, eps, wd_i):
    """u and |r| + |wd p| in fp64 from stored p, m, v."""
    r = (m / bc1) / ((v / bc2).sqrt() + eps)
    return r + wd_i * p, r.abs() + (wd_i * p).abs()


def lamb_oracle(p, g, m, v, offsets: Sequence[int], numels: Sequence[int], flags: Sequence[int], *, lr,
                beta1, beta2, eps, weight_decay, factor: float = 1.0, t: int,
                ratios: Optional[Sequence[float]] = None):
    """One LAMB step in fp64 (``t``: 1 for the first).  Returns ``(p, m, v, ratios)``."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    omb1, b2, omb2, bc1, bc2 = lamb_coefficients(beta1, beta2, t)
    lr, eps, wd, factor = f32(lr), f32(eps), f32(weight_decay), f32(factor)
    out: List[float] = []
    for i, (off, n, fl) in enumerate(zip(offsets, numels, flags)):
        sl = slice(off, off + n)
        gi = g[sl] * factor
        wd_i = wd if fl & 2 else 0.0
        m[sl] = m[sl] + omb1 * (gi - m[sl])
        v[sl] = b2 * v[sl] + omb2 * gi * gi
        u, _ = lamb_direction(p[sl], m[sl], v[sl], bc1=bc1, bc2=bc2, eps=eps, wd_i=wd_i)
        wn, un = float(p[sl].norm()), float(u.norm())
        r = wn / un if (fl & 1 and wn > 0 and un > 0) else 1.0
        out.append(r)
        if ratios is not None:
            r = float(ratios[i])
        p[sl] = p[sl] - lr * r * u
    return p, m, v, out


def lamb_ratio_from_stored(p_before, m_after, v_after, offsets, numels, flags, *, beta1, beta2, eps,
                           weight_decay, t: int):
    """Exact ratios, and the amplification A of the bound, from what the kernel itself read: the
    parameters before the step and the moments it stored."""
    p, m, v = _d(p_before), _d(m_after), _d(v_after)
    _, _, _, bc1, bc2 = lamb_coefficients(beta1, beta2, t)
    eps, wd = f32(eps), f32(weight_decay)
    ratios, amps = [], []
    for off, n, fl in zip(offsets, numels, flags):
        sl = slice(off, off + n)
        u, mag = lamb_direction(p[sl], m[sl], v[sl], bc1=bc1, bc2=bc2, eps=eps, wd_i=wd if fl & 2 else 0.0)
        wn, un = float(p[sl].norm()), float(u.norm())
        ok = fl & 1 and wn > 0 and un > 0
        ratios.append(wn / un if ok else 1.0)
        amps.append(float(mag.norm()) / un if un > 0 else 1.0)
    return ratios, amps
