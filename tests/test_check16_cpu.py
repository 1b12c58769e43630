"""The half-ulp checker of tests/check16.py against an fp32 emulation of csrc/kernels/gelu.h.

The GPU edge tests trust ``check16`` with the slacks asserted here: it must accept the documented
fp32 formula (A&S 7.1.26, one exp, one reciprocal) on every 16-bit input, and it must reject a
kernel that is only subtly wrong (the tanh approximation, one perturbed polynomial coefficient).
"""
import math

import pytest
import torch

from check16 import all_finite16, check16, dgelu64, gelu64, ulp16

# The slacks the GPU tests use (tests/test_vit_kernels_edges_gpu.py).  gelu.h documents
# |erf error| <= 1.5e-7, so GELU is off by <= 0.75e-7 |z| before fp32 rounding; measured worst of
# this emulation 1.9e-7 max(1,|z|) forward and 3.0e-7 for the derivative.  The margin is for the
# hardware's approximate exp and rcp.
FWD_SLACK = 5e-7
BWD_SLACK = 1e-6

COEF = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
BIASES = (0.0, 0.37, -1.9)


def _erf_and_gauss32(z, coef=COEF):
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    x = z.abs() * f(0.70710678118654752)
    t = 1.0 / (1.0 + f(0.3275911) * x)
    p = t * (f(coef[0]) + t * (f(coef[1]) + t * (f(coef[2]) + t * (f(coef[3]) + t * f(coef[4])))))
    g = torch.exp(-x * x)
    return torch.copysign(1.0 - p * g, z), g


def gelu32(z, coef=COEF):
    erf, _ = _erf_and_gauss32(z, coef)
    return 0.5 * z * (1.0 + erf)


def dgelu32(z, coef=COEF):
    erf, g = _erf_and_gauss32(z, coef)
    return 0.5 * (1.0 + erf) + z * g * torch.tensor(0.39894228040143268, dtype=torch.float32)


def gelu_tanh32(z):
    return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z * z * z)))


def _inputs(dtype):
    u = all_finite16(dtype).float()
    u = u[u.abs() < 3e4]
    z = torch.cat([u + b for b in BIASES])      # fp32 sums, as the kernels form them
    assert z.dtype == torch.float32 and z.numel() > 90_000
    return z


def test_ulp16_values():
    r = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 0.0, 1e-6, 6e-8, 65504.0, 2.0 ** -14], dtype=torch.float64)
    assert ulp16(r, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -11, 2.0 ** -9, 2.0 ** -24,
                                                2.0 ** -24, 2.0 ** -24, 32.0, 2.0 ** -24]
    assert ulp16(r, torch.bfloat16)[:6].tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6, 2.0 ** -133]
    # every neighbouring pair of finite values is exactly one ulp16 (of the smaller one) apart
    for dt in (torch.float16, torch.bfloat16):
        v = all_finite16(dt).double()
        v = v[v >= 0].sort().values
        lo, hi = v[:-1], v[1:]
        nz = hi > lo                             # +0 / -0
        assert torch.equal((hi - lo)[nz], ulp16(lo, dt)[nz])


def test_check16_accepts_rounding_and_rejects_one_ulp():
    for dt in (torch.float16, torch.bfloat16):
        # fp32-representable references: a kernel rounds fp32 -> 16 bit once (fp64 -> 16 bit on the host rounds twice)
        ref = torch.cat([torch.randn(4096) * s for s in (1e-7, 1e-3, 1.0, 100.0)]).double()
        good = ref.to(dt)
        check16(good, ref, 0.0)
        worse = good.clone()
        worse[17] = (good[17].double() + 1.01 * ulp16(ref[17], dt) * (1 if good[17] >= ref[17] else -1)).to(dt)
        with pytest.raises(AssertionError, match=r"worst at \(17,\)"):
            check16(worse, ref, 0.0)
        nan = good.clone()
        nan[3] = float("nan")
        with pytest.raises(AssertionError):
            check16(nan, ref, 1.0)


def test_fp64_references():
    z = torch.linspace(-9, 9, 3601, dtype=torch.float64).requires_grad_(True)
    ref = torch.nn.functional.gelu(z)
    ref.sum().backward()
    # the 1 + erf form is only absolutely accurate: compare absolutely, then the tail relatively to erfc
    assert (gelu64(z.detach()) - ref.detach()).abs().max() < 4e-15
    assert (dgelu64(z.detach()) - z.grad).abs().max() < 4e-15
    assert gelu64(torch.tensor(-8.0)).item() == pytest.approx(-8.0 * 0.5 * math.erfc(8.0 / math.sqrt(2.0)), rel=1e-14)
    assert gelu64(torch.tensor(-8.0)).item() < 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gelu_h_formula_passes_check16(dtype):
    z = _inputs(dtype)
    z64 = z.double()
    mag = z64.abs().clamp(min=1.0)
    h, d = gelu32(z), dgelu32(z)
    fwd_err = ((h.double() - gelu64(z64)).abs() / mag).max().item()
    bwd_err = (d.double() - dgelu64(z64)).abs().max().item()
    print(f"{dtype}: forward error before rounding {fwd_err:.3e} * max(1,|z|), derivative error {bwd_err:.3e}")
    assert fwd_err <= FWD_SLACK and bwd_err <= BWD_SLACK
    check16(h.to(dtype), gelu64(z64), FWD_SLACK * mag, inp=z, what="gelu.h forward")
    check16(d.to(dtype), dgelu64(z64), BWD_SLACK, inp=z, what="gelu.h derivative")
    # with a gradient: gu = gh * gelu'(z), slack 1e-6 |gh|
    gh = torch.randn(z.shape, generator=torch.Generator().manual_seed(0)).to(dtype).float()
    check16((gh * d).to(dtype), gh.double() * dgelu64(z64), BWD_SLACK * gh.double().abs(), inp=z, what="gelu.h gu")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_check16_rejects_subtly_wrong_gelu(dtype):
    z = _inputs(dtype)
    z64 = z.double()
    mag = z64.abs().clamp(min=1.0)
    with pytest.raises(AssertionError, match="beyond half an ulp"):
        check16(gelu_tanh32(z).to(dtype), gelu64(z64), FWD_SLACK * mag, inp=z, what="tanh gelu")
    # each coefficient changed in its 5th significant digit
    for k in range(5):
        digits = 4 - math.floor(math.log10(abs(COEF[k])))
        wrong = list(COEF)
        wrong[k] = COEF[k] + 10.0 ** -digits
        assert abs(wrong[k] / COEF[k] - 1) < 5e-4
        with pytest.raises(AssertionError, match="beyond half an ulp"):
            check16(gelu32(z, wrong).to(dtype), gelu64(z64), FWD_SLACK * mag, inp=z, what=f"coef {k}")
        with pytest.raises(AssertionError, match="beyond half an ulp"):
            check16(dgelu32(z, wrong).to(dtype), dgelu64(z64), BWD_SLACK, inp=z, what=f"coef {k} derivative")
