"""ConvNeXt block kernels (csrc/kernels/cnx_kernels.hip) against fp64 on the CPU.

The references read the already rounded operands.  Bounds have the form u_out |ref| + k e A with
u = 2^-8 (bf16), 2^-11 (fp16), e = 2^-24 (fp32), A the reference expression on absolute values and
k counted from the kernel's fp32 operations (first order; C channels, T rows):

LayerNorm forward.  mean: a C-term sum and a multiply by the rounded 1/C, k = C + 1 on mean|y|.
d = y - mean: one rounding plus the mean's error, (C + 2) e (|y| + mean|y|).  var: C fused squares,
the 1/C multiply and the 2 e relative of d (the common mean error cancels to first order as
sum d = 0): C + 4, + 1 for eps; rstd = rsqrtf(var) halves that and adds 2 e for the instruction:
k = C/2 + 5 on rstd.  h = fma(d * rstd, gamma, beta): (C + 2) + (C/2 + 5) + 1 for the product, + 1
for the fma: k = 1.5 C + 9 on A = rstd (|y| + mean|y|) |gamma| + |beta|.

LayerNorm backward, with X = rstd (|y| + mean|y|) >= |xhat| and g = |gh| |gamma|.  xhat carries the
saved statistics' errors: (1.5 C + 9) e X.  c1 = mean(g): C + 2 on mean g.  c2 = mean(g xhat):
(C + 2) + (1.5 C + 9) on mean(g X).  g - c1 - xhat c2: 1 + (C + 2) + (1.5 C + 9) + (2.5 C + 11) and 3
for its own three roundings, times rstd with (C/2 + 5) + 1: k = 4.5 C + 29 on
A = rstd (g + mean g + X mean(g X)).  dgamma = sum_t gh xhat: at most T additions and the final
rounding, plus xhat's error: k = T + 1.5 C + 10 on sum |gh| X.  dbeta: k = T + 1 on sum |gh|.

Block tail.  out = fma(ls, z + b2, x): k = 2 on |x| + |ls| (|z| + |b2|).  dz = ls dout: k = 1.
dls = sum_t dout (z + b2) and db2 = sum_t ls dout: k = T + 2 on the sums of absolute values.

The kernel's output rounding acts on the computed value, so the slack is multiplied by (1 + u),
and below the output type's normal range it is absolute: half the smallest subnormal (2^-25 for
fp16, where a |dz| under 6e-5 among 2 M normal draws is certain) is added.
"""
import copy

import pytest
import torch

from distributed_pytorch_training_amd import ops
from distributed_pytorch_training_amd.ops import convnext as cnx

pytestmark = pytest.mark.gpu

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
E = 2.0 ** -24
KIND = {torch.bfloat16: 1, torch.float16: 2}
WIDTHS = (96, 192, 384, 768, 128, 256, 512, 1024)
EPS = 1e-6
# T as a function of (R rows per block pass, B most blocks): one row, a ragged second block, uneven slices
ROWS = {"one": lambda R, B: 1, "ragged": lambda R, B: R + 1, "slices": lambda R, B: 2 * R * B + 3}


def _within(out, ref, u, slack, what):
    err = (out.double().cpu() - ref).abs()
    fi = torch.finfo(out.dtype)
    bound = u * ref.abs() + (1 + u) * slack + fi.smallest_normal * fi.eps / 2   # half the smallest subnormal
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max err/bound {worst:.3f}")
    assert out.shape == ref.shape and bool((err <= bound).all()), (what, err.max().item(), worst)


def _ln_ref(y, gamma, beta, gh):
    """fp64 (h, mean, rstd, gy, dgamma, dbeta, X) of LayerNorm over the last dim."""
    mean = y.mean(-1, keepdim=True)
    d = y - mean
    rstd = (d.pow(2).mean(-1, keepdim=True) + EPS).rsqrt()
    xh, g = d * rstd, gh * gamma
    gy = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    X = rstd * (y.abs() + y.abs().mean(-1, keepdim=True))
    return xh * gamma + beta, mean[:, 0], rstd[:, 0], gy, (gh * xh).sum(0), gh.sum(0), X


def _ln_inputs(T, C, dt, in_f32, cuda, seed=0):
    g = torch.Generator().manual_seed(seed)
    off, scale = (torch.rand(T, 1, generator=g) * 1.5 + 0.5 for _ in range(2))
    y = (torch.randn(T, C, generator=g) * scale + off).to(torch.float32 if in_f32 else dt).to(cuda)
    gamma, beta = (torch.randn(C, generator=g).to(cuda) for _ in range(2))
    gh = torch.randn(T, C, generator=g).to(dt).to(cuda)
    return y, gamma, beta, gh


@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("in_f32", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C", WIDTHS)
def test_channel_layer_norm_against_fp64(cuda, C, dt, in_f32, rows):
    nat = ops.native()
    T = ROWS[rows](*nat.cnx_ln_geometry(C))
    y, gamma, beta, gh = _ln_inputs(T, C, dt, in_f32, cuda)
    h, mean, rstd = nat.cnx_ln_fwd(y, gamma, beta, EPS, KIND[dt])
    gy, dg, db = nat.cnx_ln_bwd(gh, y, mean, rstd, gamma)
    assert h.dtype == dt and gy.dtype == y.dtype and dg.dtype == db.dtype == torch.float32
    y64, ga64, be64, gh64 = (t.double().cpu() for t in (y, gamma, beta, gh))
    rh, rmean, rrstd, rgy, rdg, rdb, X = _ln_ref(y64, ga64, be64, gh64)
    ya, g = y64.abs(), gh64.abs() * ga64.abs()
    _within(mean, rmean, E, (C + 1) * E * ya.mean(-1), "mean")
    _within(rstd, rrstd, E, (C / 2 + 5) * E * rrstd, "rstd")
    _within(h, rh, U[dt], (1.5 * C + 9) * E * (X * ga64.abs() + be64.abs()), "h")
    A = rrstd[:, None] * (g + g.mean(-1, keepdim=True) + X * (g * X).mean(-1, keepdim=True))
    _within(gy, rgy, U[y.dtype], (4.5 * C + 29) * E * A, "gy")
    _within(dg, rdg, E, (T + 1.5 * C + 10) * E * (gh64.abs() * X).sum(0), "dgamma")
    _within(db, rdb, E, (T + 1) * E * gh64.abs().sum(0), "dbeta")


def _sr_inputs(T, C, dt, b2_dt, cuda, seed=0):
    g = torch.Generator().manual_seed(seed)
    x, dout = (torch.randn(T, C, generator=g).to(cuda) for _ in range(2))
    z = torch.randn(T, C, generator=g).to(dt).to(cuda)
    b2 = torch.randn(C, generator=g).to(b2_dt).to(cuda)
    ls = (torch.rand(C, generator=g) * 0.9 + 0.1).to(cuda)
    return x, z, b2, ls, dout


@pytest.mark.parametrize("rows", list(ROWS))
@pytest.mark.parametrize("b2_f32", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C", [8, 96, 1024])
def test_scale_residual_against_fp64(cuda, C, dt, b2_f32, rows):
    T = ROWS[rows](*ops.native().cnx_scale_residual_geometry(C))
    b2_dt = torch.float32 if b2_f32 else dt
    x, z, b2, ls, dout = _sr_inputs(T, C, dt, b2_dt, cuda)
    for t in (x, z, b2, ls):
        t.requires_grad_(True)
    out = cnx.scale_residual(x, z, b2, ls)
    dx, dz, db2, dls = torch.autograd.grad(out, (x, z, b2, ls), dout)
    assert out.dtype == torch.float32 and dz.dtype == dt and db2.dtype == b2_dt and dls.dtype == torch.float32
    assert dx.data_ptr() == dout.data_ptr()     # the residual gradient is dout itself
    x64, z64, b64, l64, d64 = (t.detach().double().cpu() for t in (x, z, b2, ls, dout))
    zb = z64.abs() + b64.abs()
    _within(out.detach(), x64 + l64 * (z64 + b64), E, 2 * E * (x64.abs() + l64 * zb), "out")
    _within(dz, l64 * d64, U[dt], E * (l64 * d64).abs(), "dz")
    _within(dls, (d64 * (z64 + b64)).sum(0), E, (T + 2) * E * (d64.abs() * zb).sum(0), "dls")
    _within(db2, (l64 * d64).sum(0), U[b2_dt], (T + 2) * E * (l64 * d64).abs().sum(0), "db2")


def test_parameter_gradients_are_deterministic(cuda):
    nat = ops.native()
    C, dt = 96, torch.bfloat16
    y, gamma, beta, gh = _ln_inputs(ROWS["slices"](*nat.cnx_ln_geometry(C)), C, dt, False, cuda, seed=1)
    _, mean, rstd = nat.cnx_ln_fwd(y, gamma, beta, EPS, 1)
    (_, dg1, db1), (_, dg2, db2) = (nat.cnx_ln_bwd(gh, y, mean, rstd, gamma) for _ in range(2))
    assert torch.equal(dg1, dg2) and torch.equal(db1, db2)
    x, z, b2, ls, dout = _sr_inputs(ROWS["slices"](*nat.cnx_scale_residual_geometry(C)), C, dt, dt, cuda, seed=1)
    (_, dl1, dc1), (_, dl2, dc2) = (nat.cnx_scale_residual_bwd(dout, z, b2, ls) for _ in range(2))
    assert torch.equal(dl1, dl2) and torch.equal(dc1, dc2)


@pytest.mark.parametrize("dim", [96, 192])
def test_block_against_the_fp64_module(cuda, monkeypatch, dim):
    """One CNBlock, forward and backward under bf16 autocast: output, input gradient and every
    parameter gradient of the native route are no further from the fp64 module than twice the
    stock autocast route's (+1e-6): the two routes differ only in where values are rounded.
    dim 96 takes gelu_linear16's unfused fallback, 192 the fused backward."""
    from distributed_pytorch_training_amd.models.convnext import CNBlock, set_native

    torch.manual_seed(0)
    base = CNBlock(dim, 1e-6)
    with torch.no_grad():
        base.layer_scale.fill_(0.5)
    x0 = torch.randn(2, dim, 9, 7)
    dout = torch.randn(2, dim, 9, 7)

    def run(block, x, dy, autocast):
        x = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = block(x)
        grads = torch.autograd.grad(out, [x, *block.parameters()], dy)
        return [t.detach().double().cpu() for t in (out, *grads)]

    ref = run(copy.deepcopy(base).double(), x0.double(), dout.double(), False)
    gpu = copy.deepcopy(base).to(cuda).to(memory_format=torch.channels_last)
    xg, dg = (t.to(cuda).contiguous(memory_format=torch.channels_last) for t in (x0, dout))
    stock = run(gpu, xg, dg, True)
    assert set_native(gpu) == 1
    monkeypatch.setattr(cnx, "CALLS", 0)
    native = run(gpu, xg, dg, True)
    assert cnx.CALLS == 2, cnx.CALLS
    names = ["out", "dx"] + [n for n, _ in base.named_parameters()]
    for name, r, s, n in zip(names, ref, stock, native):
        es, en = (s - r).abs().max().item(), (n - r).abs().max().item()
        print(f"{name}: max err stock {es:.3e} native {en:.3e}")
        assert n.shape == r.shape and en <= 2 * es + 1e-6, (name, es, en)
    monkeypatch.setattr(cnx, "ENABLED", False)
    monkeypatch.setattr(cnx, "CALLS", 0)
    run(gpu, xg, dg, True)
    assert cnx.CALLS == 0
