"""gelu_grn16 (csrc/kernels/grn_kernels.hip) against fp64 autograd of the official formula on the CPU.

The reference reads the same 16-bit u, b1 and dg, builds G with torch.linalg.vector_norm (whose
gradient at a zero norm is 0) and differentiates by autograd.  Bounds have the form
(one rounding of the output) + slack, the slack counted to first order from the kernel's fp32
operations with e = 2^-24, R rows per sample, D channels:

One rounding.  A 16-bit output (g, du, db1 in b1's type) is rounded once from fp32: half an ulp of its
type at the reference (check16.ulp16: 2^-9 |ref| at the top of a binade, 2^-8 |ref| at its bottom for
bf16; 2^-12 .. 2^-11 for fp16).  An fp32 output (dgamma, dbeta) adds e |ref|.

GELU.  gelu.h's y and GELU' are within 5e-7 max(1, |z|) and 1e-6 of fp64 for an fp32 z
(tests/test_check16_cpu.py); z = u + b1 is itself rounded, e |z|, which GELU' <= 1.13 and
GELU'' <= 0.8 carry over: ey = (5e-7 + 1.13 e) max(1, |z|), egp = (1e-6 + e) max(1, |z|).

Sums.  A sum over a sample's rows is a chain of at most ceil(R / RB) fused adds in a thread, RB
slots and at most ceil(R / RB) slices with RB <= 5 at the tested widths: K_R = R + 8 roundings on
the sum of absolute terms.  A sum over D in the finalize kernels is D / 256 terms per thread, six
butterfly steps, three wave adds, the multiply by the rounded 1 / D: K_D = D / 256 + 14.  The column
sums over partials (colsum_rows) run in fp64 and round once, the output rounding above.

Forward.  G = sqrt(sum y^2): by Cauchy-Schwarz sum |y| ey <= G sqrt(sum ey^2), so
eG = sqrt(sum_rows ey^2) + (K_R / 2 + 1) e G.  m = mean_D G: em = mean eG + K_D e m;
inv = 1 / (m + eps) has relative error rinv = em inv + 2 e.  Nx = G inv: eNx = inv eG + Nx (rinv + e).
s = fma(gamma, Nx, 1): es = |gamma| eNx + e (1 + |gamma| Nx).  g = fma(y, s, beta):
slack |s| ey + |y| es + e (|y s| + |beta|).

Backward.  S = sum_rows dg y: eS = sum |dg| ey + K_R e sum |dg y|.  dbeta: K_R e sum |dg|.
dgamma = sum_n S (G inv): sum_n (Nx eS + |S| eNx + 2 e |S| Nx).  dNx = gamma S: edNx = |gamma| eS +
e |dNx|.  A = sum_D dNx G: eA = sum (edNx G + |dNx| eG) + K_D e sum |dNx G|.  dG = c1 - c2 with
c1 = dNx inv (ec1 = inv edNx + |c1| (rinv + e)) and c2 = A inv^2 / D (ec2 = inv^2 / D eA + |c2| (2 rinv
+ 4 e)): edG = ec1 + ec2 + e (|c1| + |c2|).  y t = y dG / G with |y| <= G:
eyt = |y| / G (edG + |dG| eG / G + 2 e |dG|) + |t| ey, all 0 where G == 0 (there y == 0 in every row
and the kernel sets t = 0).  dy = fma(dg, s, y t): edy = |dg| es + eyt + e (|dg s| + 2 |y t|).
du = dy GELU': slack |GELU'| edy + |dy| egp + e |du|.  db1 = sum du over all rows: the sum of du's
slacks + K_R e sum |du|.
"""
import copy

import pytest
import torch

from check16 import dgelu64, gelu64, ulp16
from distributed_pytorch_training_amd.ops import convnext as cnx

pytestmark = pytest.mark.gpu

E, EPS = 2.0 ** -24, 1e-6
# (N, H*W, D): rows under one block pass with an odd count, a sample boundary and 48 column groups; several
# ragged slices per sample; column blocks on grid.y; a single row
SHAPES = [(2, 49, 384), (3, 200, 768), (2, 17, 4096), (1, 1, 384)]


def _within(out, ref, slack, what):
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    one = E * ref.abs() if out.dtype == torch.float32 else 0.5 * ulp16(ref, out.dtype)
    err, bound = (out.double().cpu() - ref).abs(), one + slack
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max err/bound {worst:.3f}")
    assert bool((err <= bound).all()), (what, err.max().item(), worst)    # a NaN or inf in out fails


def _inputs(N, R, D, dt, zero_channel, seed=0):
    g = torch.Generator().manual_seed(seed)
    u = (torch.randn(N, R, D, generator=g) * 1.5).to(dt)
    b1 = (torch.randn(D, generator=g) * 0.5).to(dt)
    gamma, beta = (torch.randn(D, generator=g) for _ in range(2))
    dg = torch.randn(N, R, D, generator=g).to(dt)
    if zero_channel:
        u[N - 1, :, 5] = -b1[5]                   # u + b1 == 0 in every row: G == 0 for (last sample, channel 5)
    return u, b1, gamma, beta, dg


def _reference(u, b1, gamma, beta, dg):
    """fp64 autograd of the official formula: (g, du, db1, dgamma, dbeta)."""
    leaves = [t.clone().requires_grad_(True) for t in (u, b1, gamma, beta)]
    x = 0.5 * (leaves[0] + leaves[1]) * torch.special.erfc(-(leaves[0] + leaves[1]) / 2.0 ** 0.5)
    G = torch.linalg.vector_norm(x, ord=2, dim=1, keepdim=True)
    g = leaves[2] * (x * (G / (G.mean(dim=-1, keepdim=True) + EPS))) + leaves[3] + x
    out = (g.detach(), *torch.autograd.grad(g, leaves, dg))
    assert all(bool(torch.isfinite(t).all()) for t in out)
    return out


def _slacks(u, b1, gamma, dg, beta):
    """The docstring's slacks of (g, du, db1, dgamma, dbeta) from fp64 u [N, R, D], b1, gamma, dg."""
    N, R, D = u.shape
    KR, KD = R + 8, D / 256 + 14
    z = u + b1
    za = z.abs().clamp(min=1.0)
    y, gp, ey, egp = gelu64(z), dgelu64(z), (5e-7 + 1.13 * E) * za, (1e-6 + E) * za
    rows, chans = (lambda t: t.sum(1, keepdim=True)), (lambda t: t.sum(-1, keepdim=True))
    G = rows(y * y).sqrt()
    pos = G > 0
    eG = rows(ey * ey).sqrt() + (KR / 2 + 1) * E * G
    m = chans(G) / D
    inv = 1.0 / (m + EPS)
    rinv = (chans(eG) / D + KD * E * m) * inv + 2 * E
    Nx, ga = G * inv, gamma.abs()
    eNx = inv * eG + Nx * (rinv + E)
    s, es = 1 + gamma * Nx, ga * eNx + E * (1 + ga * Nx)
    sl_g = s.abs() * ey + y.abs() * es + E * ((y * s).abs() + beta.abs())
    S, eS = rows(dg * y), rows(dg.abs() * ey) + KR * E * rows((dg * y).abs())
    sl_dbeta = KR * E * dg.abs().sum((0, 1))
    sl_dgamma = (Nx * eS + S.abs() * eNx + 2 * E * S.abs() * Nx).sum((0, 1))
    dNx = gamma * S
    edNx = ga * eS + E * dNx.abs()
    A, eA = chans(dNx * G), chans(edNx * G + dNx.abs() * eG) + KD * E * chans((dNx * G).abs())
    c1, c2 = dNx * inv, A * inv * inv / D
    dG = c1 - c2
    edG = inv * edNx + c1.abs() * (rinv + E) + inv * inv / D * eA + c2.abs() * (2 * rinv + 4 * E) + E * (c1.abs() + c2.abs())
    Gs = torch.where(pos, G, torch.ones_like(G))
    t = torch.where(pos, dG / Gs, torch.zeros_like(G))
    eyt = torch.where(pos, y.abs() / Gs * (edG + dG.abs() * eG / Gs + 2 * E * dG.abs()), torch.zeros_like(y)) + t.abs() * ey
    dy = dg * s + y * t
    edy = dg.abs() * es + eyt + E * ((dg * s).abs() + 2 * (y * t).abs())
    sl_du = gp.abs() * edy + dy.abs() * egp + E * (dy * gp).abs()
    sl_db1 = sl_du.sum((0, 1)) + KR * E * (dy * gp).abs().sum((0, 1))
    return sl_g, sl_du, sl_db1, sl_dgamma, sl_dbeta


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape,zero_channel", [(s, False) for s in SHAPES] + [(SHAPES[0], True)])
def test_gelu_grn_against_fp64(cuda, shape, zero_channel, dt):
    N, R, D = shape
    cpu = _inputs(N, R, D, dt, zero_channel)
    u, b1, gamma, beta, dg = (t.to(cuda) for t in cpu)
    leaves = [t.requires_grad_(True) for t in (u, b1, gamma, beta)]
    g = cnx.gelu_grn16(u, b1, gamma, beta, R)
    grads = torch.autograd.grad(g, leaves, dg)
    assert g.dtype == grads[0].dtype == grads[1].dtype == dt and grads[2].dtype == grads[3].dtype == torch.float32
    u64, b64, ga64, be64, dg64 = (t.double() for t in cpu)
    refs = _reference(u64, b64, ga64, be64, dg64)
    if zero_channel:
        assert bool((refs[0][N - 1, :, 5] == be64[5]).all())      # y == 0 there: g is beta alone
    slacks = _slacks(u64, b64, ga64, dg64, be64)
    for name, out, ref, slack in zip(("g", "du", "db1", "dgamma", "dbeta"), (g.detach(), *grads), refs, slacks):
        _within(out, ref, slack, name)
    again = torch.autograd.grad(cnx.gelu_grn16(u, b1, gamma, beta, R), leaves, dg)
    assert all(torch.equal(a, b) for a, b in zip(grads, again))   # fixed-order sums: bitwise repeatable


def test_unsupported_gpu_input_raises(cuda):
    u, v = torch.zeros(2, 4, 20, device=cuda, dtype=torch.bfloat16), torch.zeros(20, device=cuda)
    with pytest.raises(RuntimeError, match="D % 8 == 0"):
        cnx.gelu_grn16(u, v.bfloat16(), v, v, 4)


def test_v2_block_takes_the_native_route(cuda, monkeypatch):
    """One CNBlockV2 with non-zero GRN parameters under bf16 autocast: the native route advances
    cnx.CALLS and is no further from the fp64 module than twice the module-by-module route under
    autocast (+1e-6), output, input gradient and every parameter gradient, as
    tests/test_cnblock_gpu.py holds the V1 block."""
    from distributed_pytorch_training_amd.models.convnext import CNBlockV2, set_native

    torch.manual_seed(0)
    base = CNBlockV2(96)
    with torch.no_grad():
        base.grn.gamma.normal_()
        base.grn.beta.normal_()
    x0, dout = torch.randn(2, 96, 9, 7), torch.randn(2, 96, 9, 7)

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
    assert cnx.CALLS == 3, cnx.CALLS          # channel_layer_norm16, gelu_grn16, scale_residual
    names = ["out", "dx"] + [n for n, _ in base.named_parameters()]
    for name, r, s, n in zip(names, ref, stock, native):
        es, en = (s - r).abs().max().item(), (n - r).abs().max().item()
        print(f"{name}: max err stock {es:.3e} native {en:.3e}")
        assert n.shape == r.shape and en <= 2 * es + 1e-6, (name, es, en)
    monkeypatch.setattr(cnx, "ENABLED", False)
    monkeypatch.setattr(cnx, "CALLS", 0)
    run(gpu, xg, dg, True)
    assert cnx.CALLS == 0
