"""Every stage of the fused BatchNorm kernels (csrc/kernels/bn_kernels.hip) against the fp64 oracle
and the derived rounding bounds of tests/bn_oracle.py, at the smallest shapes that reach each
branch of the launch geometry.  Each test drives the bindings directly and hands a stage the
oracle's inputs rounded to fp32, so errors do not compound across stages.

Run with ``-s`` to print the worst error / bound ratios (profiles/bn_error_bounds.md)."""
import time

import pytest
import torch

import bn_oracle as bo

pytestmark = pytest.mark.gpu

EPS = 1e-5
F = bo.FACTOR
_WORST = {}


def _dt(d):
    return str(d).replace("torch.", "")


dtypes = pytest.mark.parametrize("dtype", bo.DTYPES, ids=_dt)

# C, M, what the shape reaches (bn_geometry; tests/test_bn_oracle_cpu.py has the numbers)
TABLE = [
    (8, 2, "rpi256-one_chunk_of_2_rows"), (8, 255, "rpi256-one_chunk"), (8, 257, "rpi256-last_chunk_of_1_row"),
    (8, 513, "rpi256-3_chunks"), (16, 129, "rpi128-last_chunk_of_1_row"), (32, 65, "rpi64-last_chunk_of_1_row"),
    (64, 18, "fewer_rows_than_a_chunk"), (128, 100, "last_chunk_of_36_rows"), (512, 67, "rpi4-unroll_tails"),
    (1024, 131, "rpi2-lds_writeout_loop"), (2048, 3, "rpi1-lds_writeout_loop-3_rows"),
    (2048, 65, "rpi1-lds_writeout_loop-unroll_tails"), (64, 32769, "rows_per_chunk96-342_chunks-last_of_33"),
    (2048, 8193, "bwd_apply_2_reversed_iterations-rpi1"), (1024, 16385, "bwd_apply_2_reversed_iterations-rpi2-257_chunks"),
]
table = pytest.mark.parametrize("C,M", [pytest.param(c, m, id=f"C{c}-M{m}-{what}") for c, m, what in TABLE])


@pytest.fixture(scope="module")
def native(cuda):
    from distributed_pytorch_training_amd import ops
    return ops.native()


@pytest.fixture(scope="module")
def worst():
    yield _WORST
    if _WORST:
        print("\nBatchNorm kernels vs fp64 oracle on the GPU: worst error / bound, tie shares, seconds")
        for (stage, dt), (r, where) in sorted(_WORST.items()):
            print(f"{stage:26s} {dt:9s} {r:10.4g}  at {where}")


def _note(worst, stage, dtype, value, where):
    key = (stage, _dt(dtype))
    if value >= worst.get(key, (-1.0, ""))[0]:
        worst[key] = (value, where)


_CASE = {}


def _case(dev, C, M, dtype):
    """One case at a time stays alive (the large ones are tens of MB per tensor)."""
    key = (C, M, dtype)
    if key not in _CASE:
        _CASE.clear()
        k = bo.case(M, C, dtype, dev)
        s, q, e_s, e_q = bo.fwd_sums(k["x"], k["geo"])
        k["sums"] = (s, q, e_s, e_q)
        k["want"], k["bound"] = bo.fwd_finalize(s, q, e_s, e_q, M, k["gamma"], k["beta"], EPS, 0.1, k["rm0"], k["rv0"])
        # the fp32 numbers a later stage is handed: the oracle's, rounded
        for n in ("mean", "invstd", "a", "b"):
            k[n + "32"] = k["want"][n].float().contiguous()
        k["coef"] = torch.cat([k["a32"], k["b32"]]).contiguous()
        s2, q2, e_s2, e_q2 = bo.fwd_sums(k["x2"], k["geo"])
        w2, _ = bo.fwd_finalize(s2, q2, e_s2, e_q2, M, k["gamma2"], k["beta2"], EPS, 0.1, k["rm0"], k["rv0"])
        k["mean2_32"], k["invstd2_32"] = w2["mean"].float().contiguous(), w2["invstd"].float().contiguous()
        k["coef2"] = torch.cat([w2["a"].float(), w2["b"].float()]).contiguous()
        _CASE[key] = k
    return _CASE[key]


def _poison(like):
    """Fill the block the next same-sized output is most likely to get with NaN, so a row a kernel
    never writes cannot hold an earlier call's correct values."""
    t = torch.empty_like(like)
    t.fill_(float("nan"))
    del t


def _same_bits(got, want):
    """Equal to the bit, NaN matching any NaN (the payload is not specified)."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return torch.equal(gn, wn) and torch.equal(bo.bits(got)[~gn], bo.bits(want)[~wn])


def _slices(M, C):
    step = max(1, (1 << 23) // C)
    return [(r0, min(r0 + step, M)) for r0 in range(0, M, step)]


def _check_apply(got, k, a, b, res, a2, b2, relu, what, worst=None):
    """The apply rule, in row slices: every element between the I/O roundings of the band's ends
    (band widened by FACTOR); ties counted from the band itself."""
    M, C, dtype = k["M"], k["C"], k["dtype"]
    g = bo.rows(got)
    assert g.shape == (M, C) and got.dtype == dtype
    bad = ties = 0
    for r0, r1 in _slices(M, C):
        v, band = bo.apply_value(k["x"][r0:r1], a, b, None if res is None else res[r0:r1], a2, b2)
        bad += bo.check_interval(g[r0:r1], v, band, dtype, relu, F)[0]
        ties += bo.check_interval(g[r0:r1], v, band, dtype, relu, 1.0)[1]
        if dtype == torch.float32 and worst is not None:
            want = bo._relu(v) if relu else v
            _note(worst, "fwd apply (fp32: ratio)", dtype, bo.worst_ratio(g[r0:r1], want, band), what)
    n = M * C
    assert ties <= bo.ties_allowed(n), f"{what}: {ties} of {n} elements on a rounding boundary: the inputs are unfit"
    assert bad == 0, f"{what}: {bad} of {n} elements are not the rounding of the fp64 value (nor its neighbour at a tie)"
    if worst is not None and n >= 100000:
        _note(worst, "fwd apply tie share", dtype, ties / n, what)


def _check_stats(got, want, bound, names, what, worst, stage, dtype):
    for n in names:
        assert torch.isfinite(got[n]).all(), f"{what}: {n} is not finite"
        r = bo.worst_ratio(got[n], want[n], bound[n])
        _note(worst, f"{stage} {n}", dtype, r, what)
        assert r <= F, f"{what}: {n} error is {r:.3f} x its bound (allowed {F})"


# ---- forward -----------------------------------------------------------------------------------
@dtypes
@table
def test_forward_statistics(cuda, native, worst, C, M, dtype):
    k = _case(cuda, C, M, dtype)
    x4 = bo.as_nchw(k["x"])
    s, q, e_s, e_q = k["sums"]
    for mom in (0.1, 0.37):
        rm, rv = k["rm0"].clone(), k["rv0"].clone()
        nb = torch.full((), 4, dtype=torch.long, device=cuda)
        y, mean, invstd, coef = native.bn_fwd_train(x4, None, k["gamma"], k["beta"], rm, rv, nb, mom, EPS, False,
                                                    None, None, False)
        want, bound = bo.fwd_finalize(s, q, e_s, e_q, M, k["gamma"], k["beta"], EPS, mom, k["rm0"], k["rv0"])
        got = dict(mean=mean, invstd=invstd, a=coef[:C], b=coef[C:], running_mean=rm, running_var=rv)
        assert y.numel() == 0 and int(nb) == 5
        _check_stats(got, want, bound, list(got), f"C={C} M={M} momentum={mom}", worst, "fwd", dtype)


@dtypes
@table
def test_forward_apply(cuda, native, worst, C, M, dtype):
    k = _case(cuda, C, M, dtype)
    x4, r4, x24 = bo.as_nchw(k["x"]), bo.as_nchw(k["r"]), bo.as_nchw(k["x2"])
    what = f"C={C} M={M}"
    for relu, res in [(True, False), (True, True), (False, False), (False, True)]:
        # bn_fwd_train: y from the coefficients the kernel itself stored
        rm, rv = k["rm0"].clone(), k["rv0"].clone()
        _poison(x4)
        y, mean, invstd, coef = native.bn_fwd_train(x4, r4 if res else None, k["gamma"], k["beta"], rm, rv, None,
                                                    0.1, EPS, relu)
        _check_apply(y, k, coef[:C], coef[C:], k["r"] if res else None, None, None, relu,
                     f"{what} bn_fwd_train relu={relu} res={res}", worst)
        if relu and res:
            mask = torch.full((M, C // 8), 0xA5, dtype=torch.uint8, device=cuda)
            _poison(x4)
            ym, _, _, coefm = native.bn_fwd_train(x4, r4, k["gamma"], k["beta"], k["rm0"].clone(), k["rv0"].clone(),
                                                  None, 0.1, EPS, True, mask_out=mask)
            assert torch.equal(coefm, coef) and torch.equal(bo.bits(bo.rows(ym)), bo.bits(bo.rows(y)))
            _check_mask(mask, ym, f"{what} bn_fwd_train mask_out")
        del y
        # bn_apply: the oracle's coefficients
        _poison(x4)
        y = native.bn_apply(x4, r4 if res else None, k["a32"], k["b32"], relu)
        _check_apply(y, k, k["a32"], k["b32"], k["r"] if res else None, None, None, relu,
                     f"{what} bn_apply relu={relu} res={res}", worst)
        del y
    a2, b2 = k["coef2"][:C], k["coef2"][C:]
    _poison(x4)
    y = native.bn_apply_aff(x4, x24, k["coef"], k["coef2"])
    _check_apply(y, k, k["a32"], k["b32"], k["x2"], a2, b2, True, f"{what} bn_apply_aff", worst)
    mask = torch.full((M, C // 8), 0x5A, dtype=torch.uint8, device=cuda)
    _poison(x4)
    ym = native.bn_apply_aff(x4, x24, k["coef"], k["coef2"], mask_out=mask)
    assert torch.equal(bo.bits(bo.rows(ym)), bo.bits(bo.rows(y)))
    _check_mask(mask, ym, f"{what} bn_apply_aff mask_out")


def _check_mask(mask, y, what):
    """mask_out: bit k of byte (m, g) = (y[m, 8g + k] > 0) of the stored y."""
    pos = (bo.rows(y) > 0).view(mask.shape[0], mask.shape[1], 8).to(torch.int32)
    want = (pos << torch.arange(8, device=y.device, dtype=torch.int32)).sum(-1).to(torch.uint8)
    assert torch.equal(mask, want), f"{what}: {(mask != want).sum().item()} mask bytes differ from (y > 0)"


def test_forward_apply_second_grid_stride_iteration(cuda, native, worst):
    """C = 2048, M = 65537, bf16 (256 MB a tensor): the forward apply's grid is capped at 32768 blocks
    of 2 rows, so row 65536 is block 0's second iteration, alone (its pair would lie past the end),
    walked in reverse.  Reference in row slices."""
    C, M, dtype = 2048, 65537, torch.bfloat16
    assert bo.geometry(M, C)["fwd_apply_iters"] == 2
    t0 = time.time()
    gamma, beta, mu, sd = bo.channel_params(C, cuda)
    gamma2, beta2, mu2, sd2 = bo.channel_params(C, cuda, 1)
    k = dict(M=M, C=C, dtype=dtype, x=bo.activations(M, C, dtype, cuda, 1, mu, sd), r=bo.activations(M, C, dtype, cuda, 2))
    a = (gamma / sd).contiguous()
    b = (beta - mu * a).contiguous()
    a2 = (gamma2 / sd2).contiguous()
    b2 = (beta2 - mu2 * a2).contiguous()
    x4, r4 = bo.as_nchw(k["x"]), bo.as_nchw(k["r"])
    for relu, res in [(True, True), (False, False)]:
        _poison(x4)
        y = native.bn_apply(x4, r4 if res else None, a, b, relu)
        _check_apply(y, k, a, b, k["r"] if res else None, None, None, relu, f"C={C} M={M} bn_apply relu={relu} res={res}",
                     worst)
        del y
    mask = torch.full((M, C // 8), 0xA5, dtype=torch.uint8, device=cuda)
    _poison(x4)
    y = native.bn_apply_aff(x4, r4, torch.cat([a, b]), torch.cat([a2, b2]), mask_out=mask)
    _check_apply(y, k, a, b, k["r"], a2, b2, True, f"C={C} M={M} bn_apply_aff", worst)
    _check_mask(mask, y, f"C={C} M={M} bn_apply_aff mask_out")
    torch.cuda.synchronize()
    _note(worst, "256 MB fwd apply: seconds", dtype, time.time() - t0, f"C={C} M={M}")


# ---- backward ----------------------------------------------------------------------------------
def _check_bwd(native, worst, k, what, dy2, relu, want_dz, mx, want_dparams=True):
    """One dispatch arm of bn_bwd: dz to the bit, dgamma / dbeta / dx against the bounds."""
    M, C, dtype, geo = k["M"], k["C"], k["dtype"], k["geo"]
    nch = bo.as_nchw
    y = mask = None
    if relu and mx:
        mask, close = bo.mask_from_x(k["x"], k["coef"])
        assert close == 0.0
    elif relu:
        y = k["y_saved"]
        mask = y > 0
    _poison(nch(k["x"]))
    _poison(nch(k["x"]))
    dx, dg, db, dz = native.bn_bwd(nch(k["dy"]), None if dy2 is None else nch(dy2), None if y is None else nch(y),
                                   nch(k["x"]), k["gamma"], k["mean32"], k["invstd32"], relu, want_dz, want_dparams,
                                   k["coef"] if mx else None)
    dz_want = bo.dz_exact(k["dy"], dy2, mask)
    if want_dz or dy2 is not None:
        assert dz.dtype == dtype
        assert torch.equal(bo.bits(bo.rows(dz)), bo.bits(dz_want)), f"{what}: dz is not (dy [+ dy2]) * mask to the bit"
    else:
        assert dz is None
    s1, s2, e1, e2 = bo.bwd_sums(k["dy"], dy2, mask, k["x"], k["mean32"], geo)
    want, bound = bo.bwd_finalize(s1, s2, e1, e2, M, k["gamma"], k["invstd32"])
    if want_dparams:
        _check_stats(dict(dgamma=dg, dbeta=db), want, bound, ["dgamma", "dbeta"], what, worst, "bwd", dtype)
    else:
        assert dg is None and db is None
    g = bo.rows(dx)
    bad = 0
    for r0, r1 in _slices(M, C):
        v, e = bo.dx_value(dz_want[r0:r1], k["x"][r0:r1], k["mean32"], want, bound)
        bad += bo.check_interval(g[r0:r1], v, e, dtype, False, F)[0]
        if dtype == torch.float32:
            _note(worst, "bwd dx (fp32: ratio)", dtype, bo.worst_ratio(g[r0:r1], v, e), what)
    assert bad == 0, f"{what}: {bad} of {M * C} dx elements outside the bound"


@dtypes
@table
def test_backward(cuda, native, worst, C, M, dtype):
    k = _case(cuda, C, M, dtype)
    if "y_saved" not in k:   # the block tail's saved output relu(x*a + b + r), by the oracle
        k["y_saved"] = bo.model_apply(k["x"], k["a32"], k["b32"], k["r"], None, None, True).contiguous()
    arms = [  # name, dy2, relu, want_dz, mask recomputed from x (coef given, y None), want_dparams
        ("stats<relu,one,wdz> apply<from_dz>", None, True, True, False, True),
        ("stats<relu,two,wdz> apply<from_dz>", k["dy2"], True, False, False, True),
        ("stats<norelu,two,wdz> apply<from_dz>", k["dy2"], False, False, False, True),
        ("stats<norelu,one,wdz> apply<from_dz>", None, False, True, False, True),
        ("stats<relu,mx> apply<relu,mx>", None, True, False, True, True),
        ("stats<relu,y> apply<relu,y>", None, True, False, False, True),
        ("stats<norelu> apply<norelu>", None, False, False, False, True),
        ("stats<relu,mx> no dparams", None, True, False, True, False),
    ]
    for name, dy2, relu, want_dz, mx, want_dparams in arms:
        _check_bwd(native, worst, k, f"C={C} M={M} {name}", dy2, relu, want_dz, mx, want_dparams)


# ---- finalize variants on synthetic partitions ---------------------------------------------------
CHUNKS = [1, 31, 32, 33, 224, 225, 256, 257, 1792, 1793, 2048, 2049, 8192, 8193, 16384, 16385]
FIN_M, FIN_C = 16390, 16


def _fin_id(n):
    kind = "half_wave" if n <= 256 else ("wide256" if n <= 8192 else "wide1024_fwd-wide256_bwd")
    return f"{n}_partials-{kind}"


chunk_counts = pytest.mark.parametrize("chunks", CHUNKS, ids=_fin_id)


@chunk_counts
def test_forward_finalize_from_partials(cuda, native, worst, chunks):
    """bn_fwd_train(psum, psq, apply=False): half-wave sum up to 256 partials (unroll edge at
    k + 224 < chunks), 256-thread block sum up to 8192 (edge at multiples of 2048), 1024 threads
    above.  x only gives M and C; bf16."""
    M, C = FIN_M, FIN_C
    k = _case(cuda, C, M, torch.bfloat16)
    gid = bo.partition(M, chunks, cuda)
    xd = k["x"].double()
    ps, pq = bo.group_sums(xd, gid, chunks), bo.group_sums(xd * xd, gid, chunks)
    s, q, e_s, e_q = bo.partial_sums(ps, pq)
    want, bound = bo.fwd_finalize(s, q, e_s, e_q, M, k["gamma"], k["beta"], EPS, 0.1, k["rm0"], k["rv0"])
    rm, rv = k["rm0"].clone(), k["rv0"].clone()
    nb = torch.zeros((), dtype=torch.long, device=cuda)
    y, mean, invstd, coef = native.bn_fwd_train(bo.as_nchw(k["x"]), None, k["gamma"], k["beta"], rm, rv, nb, 0.1, EPS,
                                                False, ps, pq, False)
    got = dict(mean=mean, invstd=invstd, a=coef[:C], b=coef[C:], running_mean=rm, running_var=rv)
    assert int(nb) == 1
    _check_stats(got, want, bound, list(got), f"{chunks} partials", worst, "fwd finalize", torch.bfloat16)


@dtypes
@chunk_counts
def test_backward_finalize_from_partials(cuda, native, worst, chunks, dtype):
    """bn_bwd_partials with the mask recomputed from x (from_dz false) and with dz handed in, and
    bn2_bwd_partials with two different BatchNorms: narrow / wide finalize and finalize2."""
    M, C = FIN_M, FIN_C
    k = _case(cuda, C, M, dtype)
    nch = bo.as_nchw
    gid = bo.partition(M, chunks, cuda, seed=1)
    what = f"{chunks} partials"
    if "y_saved" not in k:
        k["y_saved"] = bo.model_apply(k["x"], k["a32"], k["b32"], k["r"], None, None, True).contiguous()
    xm = k["x"].double() - k["mean32"].double()
    for from_dz in (False, True):
        if from_dz:
            dz = bo.dz_exact(k["dy"], k["dy2"], k["y_saved"] > 0).contiguous()
        else:
            dz = bo.dz_exact(k["dy"], None, bo.mask_from_x(k["x"], k["coef"])[0])
        p1, p2 = bo.group_sums(dz.double(), gid, chunks), bo.group_sums(dz.double() * xm, gid, chunks)
        s1, s2, e1, e2 = bo.partial_sums(p1, p2)
        want, bound = bo.bwd_finalize(s1, s2, e1, e2, M, k["gamma"], k["invstd32"])
        _poison(nch(k["x"]))
        dx, dg, db = native.bn_bwd_partials(nch(dz if from_dz else k["dy"]), nch(k["x"]), k["gamma"], k["mean32"],
                                            k["invstd32"], None if from_dz else k["coef"], p1, p2, True, from_dz)
        w = f"{what} from_dz={from_dz}"
        _check_stats(dict(dgamma=dg, dbeta=db), want, bound, ["dgamma", "dbeta"], w, worst, "bwd finalize", dtype)
        v, e = bo.dx_value(dz, k["x"], k["mean32"], want, bound)
        bad = bo.check_interval(bo.rows(dx), v, e, dtype, False, F)[0]
        assert bad == 0, f"{w}: {bad} dx elements outside the bound"
    # two BatchNorms fed the same dz
    xm2 = k["x2"].double() - k["mean2_32"].double()
    p3 = bo.group_sums(dz.double() * xm2, gid, chunks)
    _, s3, _, e3 = bo.partial_sums(p1, p3)
    want2, bound2 = bo.bwd_finalize(s1, s3, e1, e3, M, k["gamma2"], k["invstd2_32"])
    _poison(nch(k["x"]))
    _poison(nch(k["x"]))
    dx, dx2, dg, db, dg2, db2 = native.bn2_bwd_partials(nch(dz), nch(k["x"]), nch(k["x2"]), k["gamma"], k["gamma2"],
                                                        k["mean32"], k["invstd32"], k["mean2_32"], k["invstd2_32"],
                                                        p1, p2, p3, True)
    _check_stats(dict(dgamma=dg, dbeta=db), want, bound, ["dgamma", "dbeta"], what + " bn2 tail", worst, "bwd finalize",
                 dtype)
    _check_stats(dict(dgamma=dg2, dbeta=db2), want2, bound2, ["dgamma", "dbeta"], what + " bn2 downsample", worst,
                 "bwd finalize", dtype)
    for got, xx, mm, ww, bb, n in ((dx, k["x"], k["mean32"], want, bound, "dx"),
                                   (dx2, k["x2"], k["mean2_32"], want2, bound2, "dx2")):
        v, e = bo.dx_value(dz, xx, mm, ww, bb)
        bad = bo.check_interval(bo.rows(got), v, e, dtype, False, F)[0]
        assert bad == 0, f"{what} bn2: {bad} {n} elements outside the bound"


# ---- conditioning ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=_dt)
def test_statistics_at_the_stem_conditioning(cuda, native, worst, dtype):
    """|mean| / std from 1 up to 60 (mean 3, std down to 0.05), M = 32769, C = 64: var (read back
    through running_var with momentum 1 from zero) and invstd held to the derived bound."""
    k, ratio = bo.cond_case(dtype, cuda)
    M, C = k["M"], k["C"]
    s, q, e_s, e_q = bo.fwd_sums(k["x"], k["geo"])
    zero = torch.zeros(C, device=cuda)
    want, bound = bo.fwd_finalize(s, q, e_s, e_q, M, k["gamma"], k["beta"], EPS, 1.0, zero, zero)
    rm, rv = zero.clone(), zero.clone()
    _, mean, invstd, coef = native.bn_fwd_train(bo.as_nchw(k["x"]), None, k["gamma"], k["beta"], rm, rv, None, 1.0, EPS,
                                                False, None, None, False)
    got = dict(mean=mean, invstd=invstd, a=coef[:C], b=coef[C:], running_mean=rm, running_var=rv)
    _check_stats(got, want, bound, list(got), f"C={C} M={M} |mean|/std up to 60", worst, "fwd ill-conditioned", dtype)
    var = rv.double() * (M - 1.0) / M
    rel = ((var - want["var"]).abs() / want["var"])
    _note(worst, "ill-conditioned var: measured relative error", dtype, rel.max().item(), f"|mean|/std = {ratio[rel.argmax()]:.1f}")
    _note(worst, "ill-conditioned var: bound, relative", dtype, (bound["var"] / want["var"]).max().item(), "|mean|/std = 60")
    _note(worst, "ill-conditioned invstd: measured relative error", dtype,
          ((invstd.double() - want["invstd"]).abs() / want["invstd"]).max().item(), "")


# ---- special values --------------------------------------------------------------------------------
def _specials(dtype, dev):
    fi = torch.finfo(dtype)
    return torch.tensor([0.0, -0.0, fi.smallest_normal * fi.eps, fi.smallest_normal, float("inf"), float("-inf"),
                         float("nan"), -1.0], dtype=dtype, device=dev)


@dtypes
def test_relu_mask_of_special_values_in_y(cuda, native, dtype):
    """y in {+0, -0, smallest subnormal, smallest normal, +inf, -inf, NaN, -1}: dz is dy exactly
    where y > 0 (IEEE compare) and +0 elsewhere - BF16::pos16's bit test, F16 / F32::pos8."""
    C, M = 8, 24
    k = bo.case(M, C, dtype, cuda, seed=5)
    sp = _specials(dtype, cuda)
    idx = (torch.arange(M, device=cuda)[:, None] + torch.arange(C, device=cuda)[None, :]) % 8
    y = sp[idx].contiguous()
    k["dy"][0, :4] = -0.0
    nch = bo.as_nchw
    mean, invstd = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
    for dy2 in (None, k["dy2"]):
        dx, dg, db, dz = native.bn_bwd(nch(k["dy"]), None if dy2 is None else nch(dy2), nch(y), nch(k["x"]), k["gamma"],
                                       mean, invstd, True, True, True, None)
        want = bo.dz_exact(k["dy"], dy2, y > 0)
        assert (y > 0).sum().item() == 3 * M * C // 8
        assert torch.equal(bo.bits(bo.rows(dz)), bo.bits(want))
        assert torch.isfinite(dx).all() and torch.isfinite(dg).all() and torch.isfinite(db).all()


@dtypes
def test_mask_out_of_special_values_in_y(cuda, native, dtype):
    """The 1-bit mask the forward apply writes (store8m: BF16::pos16 on the stored bits): y =
    relu(x + -0) over the same special values, -0 and NaN included, must give bit = (y > 0)."""
    C, M = 8, 24
    sp = _specials(dtype, cuda)
    idx = (torch.arange(M, device=cuda)[:, None] + torch.arange(C, device=cuda)[None, :]) % 8
    x = sp[idx].contiguous()
    x2 = torch.full_like(x, -0.0)
    coef = torch.cat([torch.ones(C, device=cuda), torch.full((C,), -0.0, device=cuda)]).contiguous()
    mask = torch.full((M, C // 8), 0xA5, dtype=torch.uint8, device=cuda)
    y = native.bn_apply_aff(bo.as_nchw(x), bo.as_nchw(x2), coef, coef, mask_out=mask)
    want = bo.model_apply(x, coef[:C], coef[C:], x2, coef[:C], coef[C:], True)
    assert _same_bits(bo.rows(y).contiguous(), want)
    yb = bo.bits(bo.rows(y))
    assert (yb[idx == 1] == bo.bits(sp)[1]).all() and torch.isnan(bo.rows(y)[idx == 6]).all()   # -0 and NaN kept
    _check_mask(mask, y, f"{_dt(dtype)} special values")
    assert (bo.rows(y) > 0).sum().item() == 3 * M


@dtypes
def test_relu_mask_recomputed_from_x_at_exact_zero(cuda, native, worst, dtype):
    """The MX arm: fmaf(x, a, b) exactly 0, just above and just below, for both signs of a; a zero
    or negative pre-activation passes no gradient (seen through dx, dgamma and dbeta)."""
    C, M = 8, 24
    k = bo.case(M, C, dtype, cuda, seed=6)
    ulp = torch.finfo(dtype).eps
    a = torch.tensor([2.0, -2.0, 2.0, -2.0, 0.5, -0.5, 4.0, -4.0], device=cuda)
    x0 = torch.tensor([0.5, 0.5, 1.0, 1.0, 2.0, 2.0, 0.25, 0.25], device=cuda)
    b = -(a * x0)                                              # x0 * a + b == 0 exactly
    step = torch.tensor([0.0, 1.0, -1.0], device=cuda).repeat(M // 3)[:, None] * (x0 * ulp)[None, :]
    x = (x0[None, :] + step).to(dtype).contiguous()
    k["x"] = x
    k["coef"] = torch.cat([a, b]).contiguous()
    v = x.double() * a.double() + b.double()
    assert (v == 0).sum().item() == M * C // 3 and (v > 0).sum().item() == M * C // 3
    k["dy"] = (k["dy"].float().abs() + 4.0).to(dtype).contiguous()           # a wrong mask bit moves dbeta by > 4
    k["mean32"], k["invstd32"] = torch.full((C,), 0.125, device=cuda), torch.ones(C, device=cuda)
    _check_bwd(native, worst, k, f"{_dt(dtype)} fma(x, a, b) at 0", None, True, False, True)
    # the forward at the same points: +0 at the exact zero, with and without ReLU
    for relu in (True, False):
        y = native.bn_apply(bo.as_nchw(x), None, a.contiguous(), b.contiguous(), relu)
        want = bo.model_apply(x, a, b, None, None, None, relu)
        assert torch.equal(bo.bits(bo.rows(y)), bo.bits(want))
        assert (bo.bits(bo.rows(y))[v == 0] == 0).all()


@dtypes
def test_nan_and_inf_in_x_stay_in_their_channel(cuda, native, worst, dtype):
    """One NaN and one inf in x: that channel's statistics and outputs are NaN (ReLU does not turn
    the NaN into 0 - the AMP overflow check reads it), every other channel stays within bounds."""
    C, M = 16, 40
    k = bo.case(M, C, dtype, cuda, seed=7)
    clean = k["x"].clone()
    k["x"][3, 5] = float("nan")
    k["x"][7, 11] = float("inf")
    bad = torch.zeros(C, dtype=torch.bool, device=cuda)
    bad[5] = bad[11] = True
    rm, rv = k["rm0"].clone(), k["rv0"].clone()
    y, mean, invstd, coef = native.bn_fwd_train(bo.as_nchw(k["x"]), None, k["gamma"], k["beta"], rm, rv, None, 0.1, EPS,
                                                True)
    got = dict(mean=mean, invstd=invstd, a=coef[:C], b=coef[C:], running_mean=rm, running_var=rv)
    s, q, e_s, e_q = bo.fwd_sums(clean, k["geo"])
    want, bound = bo.fwd_finalize(s, q, e_s, e_q, M, k["gamma"], k["beta"], EPS, 0.1, k["rm0"], k["rv0"])
    for n in ("invstd", "a", "b", "running_var"):
        assert torch.isnan(got[n][bad]).all(), n
    assert torch.isnan(mean[5]) and mean[11] == float("inf")
    assert torch.isnan(bo.rows(y)[:, bad]).all()
    ok = ~bad
    _check_stats({n: t[ok] for n, t in got.items()}, {n: t[ok] for n, t in want.items()},
                 {n: t[ok] for n, t in bound.items()}, list(got), "NaN / inf in two channels", worst, "fwd", dtype)
    kk = dict(M=M, C=int(ok.sum()), dtype=dtype, x=clean[:, ok])
    _check_apply(bo.rows(y)[:, ok], kk, coef[:C][ok], coef[C:][ok], None, None, None, True, "NaN / inf in two channels")


# ---- unsupported widths --------------------------------------------------------------------------
def test_supported_widths_and_the_unfused_path(cuda, native):
    for c in (4, 12, 24, 2056, 4096):
        assert not native.bn_supported(c) and not bo.supported(c)
    for c in bo.WIDTHS:
        assert native.bn_supported(c)
    assert len(bo.WIDTHS) == 9
    from distributed_pytorch_training_amd.models.layers import FusedBatchNorm2d, bn_act

    C, shape = 24, (6, 24, 5, 7)
    x = torch.randn(shape, device=cuda, generator=torch.Generator(device=cuda).manual_seed(9)) * 1.7 + 0.3
    x = x.contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="unsupported channel count"):
        native.bn_fwd_train(x, None, None, None, None, None, None, 0.1, EPS, True)
    bn = FusedBatchNorm2d(C).to(cuda)
    gamma, beta, _, _ = bo.channel_params(C, cuda)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    y = bn_act(bn, x, relu=True)
    x2 = bo.rows(x)
    M = x2.shape[0]
    s, q = x2.double().sum(0), (x2.double() ** 2).sum(0)
    zero = torch.zeros(C, dtype=torch.float64, device=cuda)
    want, _ = bo.fwd_finalize(s, q, zero, zero, M, gamma, beta, bn.eps, bn.momentum, torch.zeros(C, device=cuda),
                              torch.ones(C, device=cuda))
    v = torch.relu(x2.double() * want["a"] + want["b"])
    # the stock fp32 BatchNorm's summation order is not ours to model: an fp32 sum of M = 210 terms
    # is good to 210 u = 1.3e-5 relative in the worst case
    torch.testing.assert_close(bo.rows(y).double(), v, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(bn.running_mean.double(), want["running_mean"], rtol=2e-5, atol=2e-6)
    torch.testing.assert_close(bn.running_var.double(), want["running_var"], rtol=2e-5, atol=2e-6)
    assert int(bn.num_batches_tracked) == 1
