"""optim_kernels.hip at its edges: ragged sizes and the second trip of the grid-stride loops, the
16-bit weight shadows in both kinds, and the arguments no other test passes (dampening,
zero_grad=False, Adam under a loss scale, Adam's found_inf skip).

Every in-place tensor is a 16-byte-aligned view into a larger buffer filled with a sentinel bit
pattern, and every test asserts that the sentinels around the view survive.
"""
import pytest
import torch

from distributed_pytorch_training_amd import ops
from distributed_pytorch_training_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

PAD = 8                      # elements on either side: 32 bytes of fp32, 16 bytes of a 16-bit shadow
SENT32, SENT16 = 0x4B5A5A5A, 0x5B5A
# kUnroll = 2, 2048 blocks x 256 threads x float4: the second trip starts at 4,194,304 elements
SIZES = [4, 8, 1020, 2044, 2048, 2052, 4_195_332]


class Arena:
    """A [n] view at a 16-byte-aligned offset inside a sentinel-filled buffer."""

    def __init__(self, n, dev, dtype=torch.float32):
        self.ibits = torch.int32 if dtype == torch.float32 else torch.int16
        self.sent = SENT32 if dtype == torch.float32 else SENT16
        self.buf = torch.full((n + 2 * PAD,), self.sent, dtype=self.ibits, device=dev)
        self.t = self.buf[PAD:PAD + n].view(dtype)
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()

    def set(self, values):
        self.t.copy_(values)
        return self

    def bits(self):
        return self.t.view(self.ibits).clone()

    def intact(self):
        return bool((self.buf[:PAD] == self.sent).all()) and bool((self.buf[-PAD:] == self.sent).all())


def _rand(n, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(n, device=dev, generator=g)


def _arenas(dev, n, *values):
    return [Arena(n, dev).set(v) for v in values]


def _intact(*arenas):
    return all(a.intact() for a in arenas)


SGD_KW = dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=5e-4, nesterov=False)
ADAM_KW = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, adamw=True)


def _ref_sgd(p, g, b, kw, scale, host_factor, fi, step, zero_grad):
    ref.sgd_step(p, g, b, kw["lr"], kw["momentum"], kw["dampening"], kw["weight_decay"], kw["nesterov"], scale,
                 host_factor, fi, step, zero_grad)


def _ref_adam(p, g, m, v, kw, scale, host_factor, fi, step, zero_grad):
    ref.adam_step(p, g, m, v, kw["lr"], kw["beta1"], kw["beta2"], kw["eps"], kw["weight_decay"], kw["adamw"], scale,
                  host_factor, fi, step, zero_grad)


# ---- 1. ragged and large sizes ----------------------------------------------------------------
@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_sgd_ragged_sizes(cuda, n, nesterov):
    p0, g0 = _rand(n, cuda, 1), _rand(n, cuda, 2)
    scale, step, fi = torch.tensor([256.0], device=cuda), torch.zeros(1, device=cuda), torch.zeros(1, device=cuda)
    P, G, B = _arenas(cuda, n, p0, g0 * 256, torch.zeros(n, device=cuda))
    pb, gb, bb = p0.clone(), g0 * 256, torch.zeros(n, device=cuda)
    kw = dict(SGD_KW, nesterov=nesterov)
    for it in range(3):
        ops.sgd_step(P.t, G.t, B.t, **kw, scale=scale, host_factor=0.25, found_inf=fi, step=step, zero_grad=True)
        _ref_sgd(pb, gb, bb, kw, scale, 0.25, fi, step, True)
        assert torch.count_nonzero(G.t) == 0
        step += 1
        G.set(g0 * 256 * (it + 2))
        gb.copy_(g0 * 256 * (it + 2))
    torch.testing.assert_close(P.t, pb, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(B.t, bb, rtol=1e-5, atol=1e-6)
    assert _intact(P, G, B)


@pytest.mark.parametrize("n", SIZES)
def test_adamw_ragged_sizes(cuda, n):
    p0, g0 = _rand(n, cuda, 4), _rand(n, cuda, 5)
    step, fi = torch.zeros(1, device=cuda), torch.zeros(1, device=cuda)
    z = torch.zeros(n, device=cuda)
    P, G, M, V = _arenas(cuda, n, p0, g0, z, z)
    pb, mb, vb = p0.clone(), z.clone(), z.clone()
    for it in range(3):
        G.set(g0 * (it + 1))
        gb = g0 * (it + 1)
        ops.adam_step(P.t, G.t, M.t, V.t, **ADAM_KW, scale=None, host_factor=1.0, found_inf=fi, step=step, zero_grad=True)
        _ref_adam(pb, gb, mb, vb, ADAM_KW, None, 1.0, fi, step, True)
        assert torch.count_nonzero(G.t) == 0
        step += 1
    torch.testing.assert_close(P.t, pb, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(M.t, mb, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(V.t, vb, rtol=1e-5, atol=1e-9)
    assert _intact(P, G, M, V)


def test_grad_check_second_trip(cuda):
    """grad_check_kernel<4>: 2048 blocks x 256 threads x 4 float4 = 8,388,608 elements per trip;
    the non-finite value sits in the last 1000 of 8,390,660, which only the second trip reads."""
    n = 8_390_660
    G = Arena(n, cuda).set(_rand(n, cuda, 3))
    scale, fi = torch.tensor([1024.0], device=cuda), torch.zeros(1, device=cuda)
    ops.grad_check(G.t, scale, 0.5, fi)
    assert fi.item() == 0.0
    for pos, val in [(n - 700, float("inf")), (n - 1, float("nan"))]:
        old = G.t[pos].item()
        G.t[pos] = val
        fi.zero_()
        ops.grad_check(G.t, scale, 0.5, fi)
        assert fi.item() == 1.0, (pos, val)
        G.t[pos] = old
    fi.zero_()
    ops.grad_check(G.t, scale, 0.5, fi)
    assert fi.item() == 0.0 and G.intact()


# ---- 2. shadows -------------------------------------------------------------------------------
def _step(opt, P, G, S1, S2, SH, **over):
    """One SGD / Adam / AdamW step on arenas (S1, S2 = momentum buffer | exp_avg, exp_avg_sq)."""
    kw = dict(scale=None, host_factor=1.0, found_inf=None, step=None, zero_grad=True, shadow=SH.t if SH else None)
    if opt == "sgd":
        kw.update(SGD_KW)
        kw.update(over)
        ops.sgd_step(P.t, G.t, S1.t, **kw)
    else:
        kw.update(ADAM_KW, adamw=(opt == "adamw"))
        kw.update(over)
        ops.adam_step(P.t, G.t, S1.t, S2.t, **kw)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("opt", ["sgd", "adam", "adamw"])
def test_shadow_is_rounding_of_stored_param(cuda, opt, dt):
    n = 2052
    g = torch.Generator(device=cuda)
    g.manual_seed(9)
    # magnitudes from 1e-8 to 1e5: fp16 zero, subnormal, normal and infinity all occur
    p0 = torch.randn(n, device=cuda, generator=g) * 10 ** (torch.rand(n, device=cuda, generator=g) * 13 - 8)
    P, G, S1, S2 = _arenas(cuda, n, p0, torch.zeros(n, device=cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda))
    SH = Arena(n, cuda, dt)
    step = torch.zeros(1, device=cuda)
    for it in range(3):
        G.set(torch.randn(n, device=cuda, generator=g))
        before = P.bits()
        _step(opt, P, G, S1, S2, SH, step=step)
        step += 1
        assert not torch.equal(P.bits(), before)
        assert torch.equal(SH.t, P.t.to(dt)), f"step {it}"
    assert _intact(P, G, S1, S2, SH)


def _halfway_params(dev):
    """fp32 values whose rounding to 16 bits is decided by the tie, range and subnormal rules."""
    bf_ties = [(b << 16) | 0x8000 for b in (0x3F80, 0x3F81, 0xBF80, 0xBF81, 0x0080, 0x0081, 0x7F7E)]
    v = [torch.tensor(bf_ties, dtype=torch.int64).to(torch.int32).view(torch.float32)]
    h = torch.tensor([0x3C00, 0x3C01, -0x4400, -0x43FF, 0x0001, 0x0002, 0x03FF, 0x7BFE, 0x7BFF],
                     dtype=torch.int16).view(torch.float16)      # even / odd lower neighbours, +-; 0x7bff + half = 65520
    nxt = torch.tensor([0x3C01, 0x3C02, -0x43FF, -0x43FE, 0x0002, 0x0003, 0x0400, 0x7BFF, 0x7BFF],
                       dtype=torch.int16).view(torch.float16).float()
    mid = (h.float() + nxt) / 2                       # exact in fp32
    mid[-1] = 65520.0                                 # half-way between the largest fp16 and 2^16: rounds to inf
    v.append(mid)
    v.append(torch.tensor([1e5, -1e5, 3e-6, -3e-6, 1e-9, -1e-9, 0.0, -0.0, 2.0 ** -25, 2.0 ** -24 * 1.5]))
    p = torch.cat(v)
    p = torch.cat([p, torch.ones((-p.numel()) % 4)])
    return p.to(dev)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("opt", ["sgd", "adam", "adamw"])
def test_shadow_of_unchanged_param_ties_and_range(cuda, opt, dt):
    p0 = _halfway_params(cuda)
    n = p0.numel()
    z = torch.zeros(n, device=cuda)
    P, G, S1, S2 = _arenas(cuda, n, p0, _rand(n, cuda, 6), z, z)
    SH = Arena(n, cuda, dt)
    _step(opt, P, G, S1, S2, SH, lr=0.0, weight_decay=0.0)
    assert torch.equal(P.t, p0)                      # lr = 0, no decay: stored unchanged
    assert torch.equal(SH.t, P.t.to(dt))
    assert torch.equal(SH.t.view(torch.int16), P.t.to(dt).view(torch.int16)), "bit patterns (signs of zero, inf)"
    if dt == torch.float16:
        assert bool(torch.isinf(SH.t.float()).any()) and bool(((SH.t.float() != 0) & (SH.t.float().abs() < 6e-5)).any())
    assert _intact(P, G, S1, S2, SH)


@pytest.mark.parametrize("zero_grad", [True, False])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_found_inf_leaves_everything_but_grad(cuda, opt, zero_grad):
    n = 2052
    P, G, S1, S2 = _arenas(cuda, n, _rand(n, cuda, 1), _rand(n, cuda, 2), _rand(n, cuda, 3), _rand(n, cuda, 4).abs())
    SH = Arena(n, cuda, torch.bfloat16).set(_rand(n, cuda, 5))
    before = [a.bits() for a in (P, G, S1, S2, SH)]
    _step(opt, P, G, S1, S2, SH, found_inf=torch.ones(1, device=cuda), step=torch.ones(1, device=cuda),
          zero_grad=zero_grad)
    after = [a.bits() for a in (P, G, S1, S2, SH)]
    for i, name in ((0, "p"), (2, "buf / exp_avg"), (3, "exp_avg_sq"), (4, "shadow")):
        assert torch.equal(after[i], before[i]), name
    if zero_grad:
        assert torch.count_nonzero(after[1]) == 0
    else:
        assert torch.equal(after[1], before[1])
    assert _intact(P, G, S1, S2, SH)


# ---- 3. untested arguments --------------------------------------------------------------------
def test_sgd_dampening(cuda):
    n = 2052
    p0, g0 = _rand(n, cuda, 1), _rand(n, cuda, 2)
    P, G, B = _arenas(cuda, n, p0, g0, torch.full((n,), 7.0, device=cuda))      # a stale buffer: step 0 must overwrite it
    pb, bb = p0.clone(), torch.full((n,), 7.0, device=cuda)
    kw = dict(SGD_KW, dampening=0.1)
    step = torch.zeros(1, device=cuda)
    for it in range(3):
        G.set(g0 * (it + 1))
        gb = g0 * (it + 1)
        ops.sgd_step(P.t, G.t, B.t, **kw, scale=None, host_factor=1.0, found_inf=None, step=step, zero_grad=True)
        _ref_sgd(pb, gb, bb, kw, None, 1.0, None, step, True)
        if it == 0:      # torch's first step stores buf = d, not (1 - dampening) * d
            torch.testing.assert_close(B.t, g0 + 5e-4 * p0, rtol=1e-6, atol=1e-7)
        step += 1
    torch.testing.assert_close(P.t, pb, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(B.t, bb, rtol=1e-5, atol=1e-6)
    # and the result is what torch.optim.SGD computes
    q = p0.clone().requires_grad_(True)
    o = torch.optim.SGD([q], lr=0.1, momentum=0.9, dampening=0.1, weight_decay=5e-4)
    for it in range(3):
        q.grad = g0 * (it + 1)
        o.step()
    torch.testing.assert_close(P.t, q.detach(), rtol=1e-5, atol=1e-6)
    assert _intact(P, G, B)


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_zero_grad_false_keeps_grad(cuda, opt):
    n = 2052
    p0, g0 = _rand(n, cuda, 1), _rand(n, cuda, 2)
    z = torch.zeros(n, device=cuda)
    P, G, S1, S2 = _arenas(cuda, n, p0, g0, z, z)
    gbits = G.bits()
    _step(opt, P, G, S1, S2, None, zero_grad=False)
    assert torch.equal(G.bits(), gbits)
    pb, s1, s2 = p0.clone(), z.clone(), z.clone()
    if opt == "sgd":
        _ref_sgd(pb, g0.clone(), s1, SGD_KW, None, 1.0, None, None, False)
    else:
        _ref_adam(pb, g0.clone(), s1, s2, dict(ADAM_KW, adamw=False), None, 1.0, None, None, False)
    torch.testing.assert_close(P.t, pb, rtol=1e-5, atol=1e-6)
    assert not torch.equal(P.t, p0) and _intact(P, G, S1, S2)


@pytest.mark.parametrize("adamw", [False, True])
def test_adam_under_loss_scale(cuda, adamw):
    n = 2052
    p0, g0 = _rand(n, cuda, 4), _rand(n, cuda, 5)
    scale, step, fi = torch.tensor([1024.0], device=cuda), torch.zeros(1, device=cuda), torch.zeros(1, device=cuda)
    z = torch.zeros(n, device=cuda)
    P, G, M, V = _arenas(cuda, n, p0, z, z, z)
    pb, mb, vb = p0.clone(), z.clone(), z.clone()
    pu, mu, vu = p0.clone(), z.clone(), z.clone()      # the same steps on unscaled gradients
    kw = dict(ADAM_KW, adamw=adamw)
    for it in range(3):
        G.set(g0 * (it + 1) * 2048)          # loss scale 1024, host_factor 0.5 (two ranks' sum)
        ops.adam_step(P.t, G.t, M.t, V.t, **kw, scale=scale, host_factor=0.5, found_inf=fi, step=step, zero_grad=True)
        _ref_adam(pb, g0 * (it + 1) * 2048, mb, vb, kw, scale, 0.5, fi, step, True)
        _ref_adam(pu, g0 * (it + 1), mu, vu, kw, None, 1.0, fi, step, True)
        step += 1
    for a, b, atol in ((P.t, pb, 1e-6), (M.t, mb, 1e-7), (V.t, vb, 1e-9)):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=atol)
    torch.testing.assert_close(P.t, pu, rtol=1e-5, atol=1e-6)      # powers of two: the scaling is exact
    assert _intact(P, G, M, V)


def test_adam_skips_on_inf(cuda):
    n = 8196
    P, G, M, V = _arenas(cuda, n, _rand(n, cuda, 1), _rand(n, cuda, 2), _rand(n, cuda, 3), _rand(n, cuda, 4).abs())
    before = [a.bits() for a in (P, M, V)]
    ops.adam_step(P.t, G.t, M.t, V.t, **ADAM_KW, scale=None, host_factor=1.0, found_inf=torch.ones(1, device=cuda),
                  step=torch.ones(1, device=cuda), zero_grad=True)
    assert all(torch.equal(a.bits(), b) for a, b in zip((P, M, V), before))
    assert torch.count_nonzero(G.t) == 0 and _intact(P, G, M, V)
