"""vit_kernels.hip at its edges: every LayerNorm width in both 16-bit kinds, the four backward
template paths, the row-partition caps, GELU over every 16-bit input, and the small reduction /
copy kernels, each against an fp64 reference on the same (16-bit-rounded or fp32) inputs.

The bindings are called directly (``ops.native().ln_fwd(...)``).  16-bit outputs are held to half
an ulp of their type plus the fp32 evaluation error (tests/check16.py; the GELU slacks are
justified in tests/test_check16_cpu.py); fp32 LayerNorm gradients are held to 4x the error the
fp32 PyTorch composition makes on the same inputs.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from check16 import DTYPE, KIND, all_finite16, check16, dgelu64, gelu64, ulp16
from distributed_pytorch_training_amd import ops

pytestmark = pytest.mark.gpu

WIDTHS = [256, 512, 768, 1024, 1280, 1536, 1792, 2048]      # VPL 1..8
ROWS = [1, 3, 17, 67]      # idle waves, a partial 4-row block, a short last block, several blocks
EPS = 1e-6
FWD_SLACK, BWD_SLACK = 5e-7, 1e-6      # tests/test_check16_cpu.py


def _gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def _cpu_gen(seed):
    """The LayerNorm inputs come from the CPU generator: the same rows on every machine (see the
    conditioning note in _check_ln_fwd)."""
    return torch.Generator().manual_seed(seed)


def _randn(shape, g, dev):
    return torch.randn(shape, generator=g, device=g.device).to(dev)


def _ulp32(ref64):
    a = ref64.abs()
    _, e = torch.frexp(a)
    e = torch.where(a > 0, e.to(torch.int64) - 1, torch.full_like(e, -126, dtype=torch.int64)).clamp(min=-126)
    return torch.ldexp(torch.ones_like(a), (e - 23).to(torch.int32))


def _bias(choice, D, dt, dev, g, std=0.1):
    """choice 0 none / 1 fp32 / 2 the 16-bit type.  The mean of half a standard deviation keeps the
    LayerNorm row that the bias dominates (the one scaled by 0.01) away from a zero mean."""
    if choice == 0:
        return None
    b = _randn(D, g, dev) * std + 0.5 * std
    return b if choice == 1 else b.to(dt)


# ---- 1. LayerNorm forward ---------------------------------------------------------------------
def _ln_inputs(T, D, dev, g, shift=0, with_scale=False):
    x = _randn((T, D), g, dev) * 2 + 0.5
    scale = torch.ones(T, 1, device=dev)
    for i in range(min(T, 3)):          # one tiny row, one large row, one offset row
        m = (i + shift) % 3
        if m == 0:
            x[i] *= 0.01
            scale[i] = 0.01
        elif m == 1:
            x[i] *= 30
            scale[i] = 30
        else:
            x[i] += 3
    gamma = torch.rand(D, generator=g).to(dev) + 0.5
    beta = torch.rand(D, generator=g).to(dev) * 0.4 - 0.2
    return (x, gamma, beta, scale) if with_scale else (x, gamma, beta)


def _ln_branch(x, scale, dt, g):
    """The branch output added in the fused path: a quarter of the stream's variance, scaled with
    its row, so that the tiny row stays tiny and the large row large after the add, and with the
    stream's mean, so that among 16401 rows of 256 none sums to a mean near zero (see
    _check_ln_fwd; x alone, mean 0.5 +- 0.125, gets there)."""
    return ((_randn(tuple(x.shape), g, x.device) * 0.5 + 0.5) * scale).to(dt)


def _ln_ref64(s, gamma, beta):
    s64 = s.double()
    mean = s64.mean(1)
    var = ((s64 - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + EPS)
    h = (s64 - mean[:, None]) * rstd[:, None]
    if gamma is not None:
        h = h * gamma.double() + beta.double()
    return h, mean, rstd


def _check_ln_fwd(x, a, bias, gamma, beta, dt, tag):
    s, h, mean, rstd = ops.native().ln_fwd(x, a, bias, gamma, beta, EPS, KIND[dt])
    T, D = x.shape
    assert h.dtype == dt and h.shape == x.shape and mean.shape == (T,) and rstd.shape == (T,)
    if a is None:
        assert s is None
        s = x
    else:
        assert s.dtype == torch.float32
        bf = 0.0 if bias is None else bias.float()
        s32 = x + (a.float() + bf)                 # the kernel's order: x += a + bias
        s64 = x.double() + a.double() + (0.0 if bias is None else bias.double())
        ok = (s == s32) | ((s.double() - s64).abs() <= _ulp32(s64))
        assert bool(ok.all()), f"{tag}: s off at {int((~ok).sum())} elements"
    h64, mean64, rstd64 = _ln_ref64(s, gamma, beta)
    # The mean's bound is relative to |mean|, which an fp32 sum can only meet while |mean| is not
    # far below the row's rms: summing D values of that size in fp32 is off by about
    # 2^-25 rms / sqrt(D) in the mean however it is ordered, i.e. by 1e-6 |mean| once |mean| / rms
    # falls to a few 1e-3.  The rows are fixed (CPU generator) and stay clear of that; make the
    # premise explicit so that a change of the inputs cannot pass for a kernel error.
    cond = (mean64.abs() * rstd64).min().item()
    assert cond > 0.01, f"{tag}: ill-conditioned input row for the relative mean check (|mean|/std = {cond:.2e})"
    em = ((mean.double() - mean64).abs() / mean64.abs()).max().item()
    er = ((rstd.double() - rstd64).abs() / rstd64).max().item()
    print(f"{tag}: mean rel err {em:.2e} rstd rel err {er:.2e}")
    assert em <= 1e-6 and er <= 1e-6, (tag, em, er)
    check16(h, h64, 2e-6 * h64.abs().clamp(min=1.0), inp=s, what=tag + " h")
    return s, mean64, rstd64


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", WIDTHS)
def test_ln_fwd_all_widths(cuda, D, dt):
    g = _cpu_gen(D + KIND[dt])
    for it, T in enumerate(ROWS):
        x, gamma, beta, scale = _ln_inputs(T, D, cuda, g, shift=it + D // 256, with_scale=True)
        _check_ln_fwd(x, None, None, gamma, beta, dt, f"plain D={D} T={T}")
        a = _ln_branch(x, scale, dt, g)
        choice = (it + D // 256 + KIND[dt]) % 3
        _check_ln_fwd(x, a, _bias(choice, D, dt, cuda, g), gamma, beta, dt, f"fused D={D} T={T} bias={choice}")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_ln_fwd_without_affine(cuda, dt):
    g = _cpu_gen(5)
    x, _, _, scale = _ln_inputs(17, 768, cuda, g, with_scale=True)
    _check_ln_fwd(x, None, None, None, None, dt, "plain no-affine")
    a = _ln_branch(x, scale, dt, g)
    _check_ln_fwd(x, a, _bias(1, 768, dt, cuda, g), None, None, dt, "fused no-affine")


# ---- 2. LayerNorm backward --------------------------------------------------------------------
RATIOS = {}      # output -> worst kernel_err / torch_fp32_err seen (printed under -s)


def _vs_torch32(out, t32, ref64, dim, tag, name):
    """kernel_err <= 4 * torch_fp32_err + 1e-7 * scale, errors and scale (max |ref|) taken along
    ``dim``.  The factor allows another, equally valid summation order; the floor covers exact
    torch results.  Returns the bound (for the 16-bit copies of the same values)."""
    ek = (out.double() - ref64).abs().amax(dim)
    et = (t32.double() - ref64).abs().amax(dim)
    scale = ref64.abs().amax(dim)
    bound = 4 * et + 1e-7 * scale
    live = et > 0
    ratio = (ek[live] / et[live]).max().item() if bool(live.any()) else 0.0
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print(f"{tag} {name}: kernel err/scale {(ek / scale.clamp(min=1e-300)).max().item():.2e} "
          f"torch fp32 err/scale {(et / scale.clamp(min=1e-300)).max().item():.2e} worst ratio {ratio:.2f}")
    bad = ~(ek <= bound)
    assert not bool(bad.any()), (f"{tag} {name}: kernel error {ek[bad].max().item():.3e} beyond 4x the fp32 torch "
                                 f"error + floor ({bound[bad].min().item():.3e})")
    return bound


def _check_ln_bwd(T, D, dt, has_gs, want_ga, bias_choice, g, dev, tag, want_dparams=True, affine=True):
    s, gamma, beta = _ln_inputs(T, D, dev, g, shift=D // 256)
    if not affine:
        gamma = beta = None
    gh = _randn((T, D), g, dev).to(dt)
    gs = _randn((T, D), g, dev) if has_gs else None
    bias_like = _bias(bias_choice, D, dt, dev, g)
    _, mean64, rstd64 = _ln_ref64(s, gamma, beta)
    gx, ga, dgamma, dbeta, dbias = ops.native().ln_bwd(gs, gh, s, mean64.float(), rstd64.float(), gamma, want_ga,
                                                       bias_like, want_dparams)

    def torch_ln(dtype):
        sr = s.to(dtype).clone().requires_grad_(True)
        w = (torch.ones(D, device=dev, dtype=dtype) if gamma is None else gamma.to(dtype).clone()).requires_grad_(True)
        b = (torch.zeros(D, device=dev, dtype=dtype) if beta is None else beta.to(dtype).clone()).requires_grad_(True)
        hr = F.layer_norm(sr, (D,), w, b, EPS)
        dx, dw, db = torch.autograd.grad(hr, (sr, w, b), gh.to(dtype))
        if gs is not None:
            dx = gs.to(dtype) + dx
        return dx, dw, db, dx.sum(0)

    r64, r32 = torch_ln(torch.float64), torch_ln(torch.float32)
    assert gx.dtype == torch.float32 and gx.shape == s.shape
    gx_bound = _vs_torch32(gx, r32[0], r64[0], 1, tag, "gx")
    if want_dparams:
        _vs_torch32(dgamma, r32[1], r64[1], 0, tag, "dgamma")
        _vs_torch32(dbeta, r32[2], r64[2], 0, tag, "dbeta")
    else:
        assert dgamma is None and dbeta is None
    if want_ga:
        assert ga.dtype == dt
        check16(ga, r64[0], gx_bound[:, None], what=tag + " ga")
    else:
        assert ga is None
    if want_ga and bias_like is not None:
        assert dbias.dtype == bias_like.dtype and dbias.shape == (D,)
        if dbias.dtype == torch.float32:
            _vs_torch32(dbias, r32[3], r64[3], 0, tag, "dbias")
        else:
            et = (r32[3].double() - r64[3]).abs().max()
            check16(dbias, r64[3], 4 * et + 1e-7 * r64[3].abs().max(), what=tag + " dbias")
    else:
        assert dbias is None


PATHS = [(False, False), (True, True), (True, False), (False, True)]      # (HAS_GS, WRITE_GA)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", WIDTHS)
def test_ln_bwd_all_paths(cuda, D, dt):
    """Each width runs all four template paths (one per T); over the widths each T meets each path."""
    g = _cpu_gen(100 + D + KIND[dt])
    for it, T in enumerate(ROWS):
        has_gs, want_ga = PATHS[(it + D // 256) % 4]
        choice = (it + D // 256 + KIND[dt]) % 3
        _check_ln_bwd(T, D, dt, has_gs, want_ga, choice, g, cuda,
                      f"D={D} T={T} gs={int(has_gs)} ga={int(want_ga)} bias={choice}")
    print("worst kernel_err / torch_fp32_err so far:", {k: round(v, 2) for k, v in RATIOS.items()})


def test_ln_bwd_without_dparams_or_affine(cuda):
    g = _cpu_gen(7)
    _check_ln_bwd(17, 512, torch.bfloat16, True, True, 2, g, cuda, "no dparams", want_dparams=False)
    _check_ln_bwd(17, 512, torch.float16, False, False, 0, g, cuda, "no dparams, no ga", want_dparams=False)
    _check_ln_bwd(19, 768, torch.float16, True, True, 1, g, cuda, "no affine", affine=False)


# ---- 3. LayerNorm at the caps -----------------------------------------------------------------
def test_ln_at_grid_caps(cuda):
    """T = 16401: the forward grid is capped at 2048 blocks x 4 rows (its grid-stride loop runs a
    third trip for the last 17 rows); the backward has 1024 blocks x 17 rows, the last 59 of which
    start beyond T and must contribute zero partials."""
    T, D, dt = 16401, 256, torch.bfloat16
    g = _cpu_gen(11)
    x, gamma, beta, scale = _ln_inputs(T, D, cuda, g, with_scale=True)
    a = _ln_branch(x, scale, dt, g)
    _check_ln_fwd(x, a, _bias(2, D, dt, cuda, g), gamma, beta, dt, "caps fwd")
    _check_ln_bwd(T, D, dt, True, True, 1, g, cuda, "caps bwd")
    print("worst kernel_err / torch_fp32_err so far:", {k: round(v, 2) for k, v in RATIOS.items()})


# ---- 4 / 5. GELU over every input -------------------------------------------------------------
_GELU_U = {}


def _gelu_inputs(dt, dev):
    """[T, 1024]: every finite value of |u| <= 16, every power of two above (both signs), randn
    filling the last row, shuffled so that every value meets some column's bias.  Cached."""
    if dt not in _GELU_U:
        v = all_finite16(dt, 16.0)
        allv = all_finite16(dt).float()
        m, _ = torch.frexp(allv.abs())
        big = allv[(allv.abs() > 16) & (m == 0.5)].to(dt)
        cpu = torch.Generator().manual_seed(3)
        n = v.numel() + big.numel()
        T = (n + 1023) // 1024
        pad = torch.randn(T * 1024 - n, generator=cpu).to(dt)
        u = torch.cat([v, big, pad])
        u = u[torch.randperm(u.numel(), generator=cpu)].view(T, 1024)
        assert bool(torch.isfinite(u.float()).all())
        _GELU_U[dt] = u.to(dev)
    return _GELU_U[dt]


def _gelu_bias(choice, Fd, dt, dev, seed=4):
    return _bias(choice, Fd, dt, dev, _gen(dev, seed), std=0.5)


def _z64(u, bias):
    return u.double() + (0.0 if bias is None else bias.double())


def _check_gelu_fwd(u, bias, tag):
    h = ops.native().gelu_fwd(u, bias)
    assert h.dtype == u.dtype and h.shape == u.shape
    z = _z64(u, bias)
    check16(h, gelu64(z), FWD_SLACK * z.abs().clamp(min=1.0), inp=z, what=tag + " gelu_fwd")
    return h


def _check_dbias(db, S, absum, coef, out_dt, tag):
    assert db.dtype == out_dt and db.shape == S.shape
    bound = coef * absum
    if out_dt != torch.float32:
        bound = bound + 0.5 * ulp16(S, out_dt)
    err = (db.double() - S).abs()
    bad = ~(err <= bound)
    assert not bool(bad.any()), (f"{tag}: {int(bad.sum())} columns off, worst err {err[bad].max().item():.3e} "
                                 f"at column {int((err - bound).argmax())} (bound {bound[(err - bound).argmax()].item():.3e})")


def _check_gelu_bwd(u, bias, gh, tag):
    gu, db = ops.native().gelu_bwd(gh, u, bias, True)
    assert gu.dtype == u.dtype and gu.shape == u.shape
    z = _z64(u, bias)
    ref = gh.double() * dgelu64(z)
    check16(gu, ref, BWD_SLACK * gh.double().abs(), inp=z, what=tag + " gelu_bwd")
    if bias is None:
        assert db is None
    else:
        # the kernel sums the unrounded fp32 products over <= ~16 rows per chunk, chunks in fp64
        _check_dbias(db, ref.sum(0), gh.double().abs().sum(0), 3e-6, bias.dtype, tag + " gelu dbias")
        gu2, none = ops.native().gelu_bwd(gh, u, bias, False)
        assert none is None and torch.equal(gu2, gu)


@pytest.mark.parametrize("bias_choice", [0, 1, 2], ids=["nobias", "bias32", "bias16"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_gelu_fwd_every_input(cuda, dt, bias_choice):
    u = _gelu_inputs(dt, cuda)
    h = _check_gelu_fwd(u, _gelu_bias(bias_choice, 1024, dt, cuda), f"{dt} bias={bias_choice}")
    if dt == torch.float16 and bias_choice == 0:
        # z below about -4.2: the exact result is an fp16 subnormal, which torch's .to(float16) keeps.
        # Down to 8e-6 (z about -4.7) it lies beyond the slack, so a flushed store cannot pass above;
        # say so explicitly.
        ref = gelu64(u.double())
        sub = (ref.abs() >= 8e-6) & (ref.abs() < 2.0 ** -14)
        tail = sub & (u.double() < -4)
        assert int(tail.sum()) > 100
        kept = h != 0
        print(f"fp16 subnormal GELU outputs kept: {int((kept & sub).sum())} of {int(sub.sum())}, "
              f"of them in the negative tail {int((kept & tail).sum())} of {int(tail.sum())}")
        assert bool(kept[sub].all()), "fp16 subnormal results were flushed to zero"


@pytest.mark.parametrize("bias_choice", [0, 1, 2], ids=["nobias", "bias32", "bias16"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_gelu_bwd_every_input(cuda, dt, bias_choice):
    u = _gelu_inputs(dt, cuda)
    gh = torch.randn(u.shape, device=cuda, generator=_gen(cuda, 6)).to(dt)
    _check_gelu_bwd(u, _gelu_bias(bias_choice, 1024, dt, cuda), gh, f"{dt} bias={bias_choice}")


# ---- 6. GELU / bias_grad16 partition edges ----------------------------------------------------
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("T,Fd", [(1, 8), (3, 8), (7, 1032), (9, 1032), (37, 3072), (807, 64)])
def test_gelu_partition_edges(cuda, T, Fd, dt):
    """F = 1032: a second column block with one live thread; T = 9, 37: the 4-row unroll tails and
    a short last chunk; T < 8: a single chunk; T = 807, F = 64: chunks that start beyond T."""
    g = _gen(cuda, T * 31 + Fd)
    u = (torch.randn(T, Fd, device=cuda, generator=g) * 3).to(dt)
    gh = torch.randn(T, Fd, device=cuda, generator=g).to(dt)
    for choice in ((T + KIND[dt]) % 2 + 1, 0):
        bias = _gelu_bias(choice, Fd, dt, cuda, seed=T)
        _check_gelu_fwd(u, bias, f"T={T} F={Fd} bias={choice}")
        _check_gelu_bwd(u, bias, gh, f"T={T} F={Fd} bias={choice}")
    S, absum = gh.double().sum(0), gh.double().abs().sum(0)
    for out_kind in (0, 1, 2):
        db = ops.native().bias_grad16(gh, out_kind)
        _check_dbias(db, S, absum, 2e-6, DTYPE[out_kind], f"T={T} F={Fd} bias_grad16 kind {out_kind}")


# ---- 7. sum_partials --------------------------------------------------------------------------
@pytest.mark.parametrize("out_kind", [0, 1, 2])
@pytest.mark.parametrize("S,n", [(1, 4), (2, 4), (16, 4), (1, 1028), (2, 1028), (16, 1028), (2, 2_097_156),
                                 (2, 4_194_312)])
def test_sum_partials_ordered_fp32(cuda, S, n, out_kind):
    """The kernel adds the S slices in order in fp32: the same adds in torch give the same bits.
    n = 2,097,156 makes the grid-stride loop run; n = 4,194,312 is past the 2048-block cap."""
    part = torch.randn(S, n // 4, 4, device=cuda, generator=_gen(cuda, S + n))
    out = ops.native().sum_partials(part, out_kind)
    acc = part[0].clone()
    for q in range(1, S):
        acc += part[q]
    assert out.dtype == DTYPE[out_kind] and out.shape == part.shape[1:]
    assert torch.equal(out, acc.to(DTYPE[out_kind]))


# ---- 8. colsum_rows unroll boundaries ---------------------------------------------------------
@pytest.mark.parametrize("out_kind", [0, 1, 2])
def test_colsum_rows_unroll_boundaries(cuda, out_kind):
    """n around the `r + 48 < n` unroll condition of each of the 16 waves; D = 72 leaves a second,
    mostly idle column block."""
    g = _gen(cuda, 8)
    dt = DTYPE[out_kind]
    for n in (1, 16, 17, 48, 49, 64, 65, 113):
        for D in (8, 64, 72):
            part = torch.randn(n, D, device=cuda, generator=g)
            out = ops.native().colsum_rows(part, out_kind)
            assert out.dtype == dt and out.shape == (D,)
            torch.testing.assert_close(out, part.double().sum(0).float().to(dt), rtol=0, atol=0, msg=f"n={n} D={D}")


# ---- 9. copy_rows16 ---------------------------------------------------------------------------
SENTINEL = 0x7B5A      # finite in both types


def _perm(nd):
    """Leading-dim permutation of the view (the last dim stays last): the head split for 5-D
    ([b,s,3,h,dh] -> [3,b,h,s,dh]), the head merge's transpose for 4-D and 3-D."""
    return {5: (2, 0, 3, 1), 4: (0, 2, 1), 3: (1, 0)}.get(nd, tuple(range(nd - 1)))


def _view_of(buf, shape, layout):
    """A view of ``shape`` inside the flat int16 buffer ``buf`` with 16-byte-aligned row starts."""
    nd, L = len(shape), shape[-1]
    if layout == "sliced":
        padded = [d + 1 for d in shape[:-1]] + [L + 16]
        full = buf[:math.prod(padded)].view(padded)
        return full[tuple(slice(1, None) for _ in shape[:-1]) + (slice(8, 8 + L),)]
    p = _perm(nd)
    base = [0] * (nd - 1)
    for i, pi in enumerate(p):
        base[pi] = shape[i]
    return buf[8:8 + math.prod(shape)].view(base + [L]).permute(*p, nd - 1)


def _buf_len(shape):
    return math.prod([d + 1 for d in shape[:-1]] + [shape[-1] + 16]) + 16


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(8,), (5, 16), (1, 1, 1, 8), (2, 3, 5, 8), (2, 2, 3, 5, 64)], ids=str)
def test_copy_rows16_writes_only_the_view(cuda, shape, dt):
    g = _gen(cuda, len(shape))
    for src_layout in ("permuted", "sliced"):
        for dst_layout in ("permuted", "sliced"):
            sbuf = torch.randint(-30000, 30000, (_buf_len(shape),), device=cuda, generator=g, dtype=torch.int16)
            dbuf = torch.full((_buf_len(shape),), SENTINEL, device=cuda, dtype=torch.int16)
            src, dst = _view_of(sbuf, shape, src_layout), _view_of(dbuf, shape, dst_layout)
            assert src.shape == shape and dst.shape == shape
            expect = dbuf.clone()
            _view_of(expect, shape, dst_layout).copy_(src)
            before = sbuf.clone()
            ops.native().copy_rows16(src.view(dt), dst.view(dt))
            tag = f"{shape} {src_layout}->{dst_layout}"
            assert torch.equal(dst, src), tag
            assert torch.equal(dbuf, expect), tag + ": wrote outside the view"
            assert int((dbuf == SENTINEL).sum()) >= dbuf.numel() - math.prod(shape), tag
            assert torch.equal(sbuf, before), tag
