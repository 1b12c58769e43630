"""The BatchNorm error bounds of tests/bn_oracle.py hold, at 1.0x, for a CPU emulation of the
kernels' summation order (fp32 per thread, fp32 across the rpi threads of a channel, fp64 across
chunks, fp64 finalize with one fp32 rounding per stored number): the bounds the GPU tests hold the
kernels to are reachable by the arithmetic the kernels state.  Also: the geometry mirror against
rows computed by hand from bn_geometry, and the share of elements on a rounding boundary of the
apply rule (a condition of the GPU tests, computed from the oracle alone).

Run with ``-s`` to print the worst error / bound ratios (the CPU-model column of
profiles/bn_error_bounds.md)."""
import pytest
import torch

import bn_oracle as bo

CPU = torch.device("cpu")
SHAPES = [(8, 257), (32, 65), (64, 18), (128, 100), (512, 67), (2048, 65), (64, 32769)]
_WORST = {}


@pytest.fixture(scope="module")
def worst():
    yield _WORST
    if _WORST:
        print("\nBatchNorm CPU model vs fp64 oracle, worst error / bound")
        for (stage, dt), (r, where) in sorted(_WORST.items()):
            print(f"{stage:14s} {dt:9s} {r:7.3f}  at {where}")


def _note(worst, stage, dtype, ratio, where):
    key = (stage, str(dtype).replace("torch.", ""))
    if ratio >= worst.get(key, (-1.0, ""))[0]:
        worst[key] = (ratio, where)


# bn_geometry by hand: rpi = 256 / (C/8); rows = max(ceil(M/512), 64) rounded up to a multiple of
# rpi; chunks = ceil(M/rows); forward apply blocks = min(ceil(M / 2rpi), 32768), backward apply
# blocks = min(2 * forward, 8192).
GEOMETRY = [  # C, M, rpi, rows_per_chunk, chunks, last chunk's rows, fwd apply iters, bwd apply iters
    (8, 2, 256, 256, 1, 2, 1, 1), (8, 255, 256, 256, 1, 255, 1, 1), (8, 257, 256, 256, 2, 1, 1, 1),
    (8, 513, 256, 256, 3, 1, 1, 1), (16, 129, 128, 128, 2, 1, 1, 1), (32, 65, 64, 64, 2, 1, 1, 1),
    (64, 18, 32, 64, 1, 18, 1, 1), (128, 100, 16, 64, 2, 36, 1, 1), (512, 67, 4, 64, 2, 3, 1, 1),
    (1024, 131, 2, 64, 3, 3, 1, 1), (2048, 3, 1, 64, 1, 3, 1, 1), (2048, 65, 1, 64, 2, 1, 1, 1),
    (64, 32769, 32, 96, 342, 33, 1, 1), (2048, 8193, 1, 64, 129, 1, 1, 2), (1024, 16385, 2, 64, 257, 1, 1, 2),
    (2048, 65537, 1, 129, 509, 5, 2, 9),
    (64, 802816, 32, 1568, 512, 1568, 1, 4),      # ResNet-50 stem BN at batch 64
    (256, 802816, 8, 1568, 512, 1568, 2, 13),     # ResNet-50 layer1 at batch 256
]


@pytest.mark.parametrize("row", GEOMETRY, ids=lambda r: f"C{r[0]}-M{r[1]}")
def test_geometry_mirror_matches_hand_computed_rows(row):
    C, M, rpi, rpc, chunks, last, fi, bi = row
    g = bo.geometry(M, C)
    assert (g["rpi"], g["rows_per_chunk"], g["chunks"], g["last_rows"]) == (rpi, rpc, chunks, last)
    assert (g["fwd_apply_iters"], g["bwd_apply_iters"]) == (fi, bi)
    assert g["n_t"] * rpi == rpc


def test_supported_widths():
    assert [c for c in range(1, 4100) if bo.supported(c)] == list(bo.WIDTHS)


def _cond_case(dtype):
    return bo.cond_case(dtype, CPU)


def _cases(C, M, dtype):
    if (C, M) == (64, 32769):
        return _cond_case(dtype)[0]
    return bo.case(M, C, dtype, CPU)


@pytest.mark.parametrize("dtype", bo.DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("C,M", SHAPES, ids=lambda v: str(v))
def test_model_stays_inside_the_bounds(worst, C, M, dtype):
    k = _cases(C, M, dtype)
    geo, where = k["geo"], f"C={C} M={M}"
    # forward statistics + finalize
    s, q, e_s, e_q = bo.fwd_sums(k["x"], geo)
    want, bound = bo.fwd_finalize(s, q, e_s, e_q, M, k["gamma"], k["beta"], 1e-5, 0.1, k["rm0"], k["rv0"])
    got = bo.model_fwd(k["x"], geo, k["gamma"], k["beta"], 1e-5, 0.1, k["rm0"], k["rv0"])
    for n in ("mean", "var", "invstd", "a", "b", "running_mean", "running_var"):
        r = bo.worst_ratio(got[n], want[n], bound[n])
        _note(worst, "fwd " + n, dtype, r, where)
        assert r <= 1.0, f"{where}: {n} error is {r:.3f} x its bound"
    # forward apply from the model's own fp32 coefficients
    for relu, res, aff in [(True, False, False), (True, True, False), (False, False, False), (False, True, False),
                           (True, True, True)]:
        r_ = (k["x2"] if aff else k["r"]) if res else None
        a2, b2 = (got["a"].flip(0), got["b"].flip(0)) if aff else (None, None)
        v, band = bo.apply_value(k["x"], got["a"], got["b"], r_, a2, b2)
        y = bo.model_apply(k["x"], got["a"], got["b"], r_, a2, b2, relu)
        bad, ties, n = bo.check_interval(y, v, band, dtype, relu)
        assert bad == 0, f"{where}: apply relu={relu} res={res} aff={aff}: {bad} elements outside the band"
        assert ties <= bo.ties_allowed(n), f"{where}: {ties} of {n} elements on a rounding boundary"
        if n > 100000:
            _note(worst, "apply tie share", dtype, ties / n, where + f" relu={relu} res={res} aff={aff}")
    # backward: ReLU mask from the model's output, both gradients
    y = bo.model_apply(k["x"], got["a"], got["b"], k["r"], None, None, True)
    for dy2, mask in [(None, None), (None, y > 0), (k["dy2"], y > 0), (k["dy2"], None)]:
        s1, s2, e1, e2 = bo.bwd_sums(k["dy"], dy2, mask, k["x"], got["mean"], geo)
        bw, bb = bo.bwd_finalize(s1, s2, e1, e2, M, k["gamma"], got["invstd"])
        m = bo.model_bwd(k["dy"], dy2, mask, k["x"], got["mean"], k["gamma"], got["invstd"], geo)
        assert torch.equal(bo.bits(m["dz"]), bo.bits(bo.dz_exact(k["dy"], dy2, mask)))
        for n in ("dgamma", "dbeta", "k1", "k2", "k3"):
            r = bo.worst_ratio(m[n], bw[n], bb[n])
            _note(worst, "bwd " + n, dtype, r, where)
            assert r <= 1.0, f"{where}: {n} error is {r:.3f} x its bound"
        v, e = bo.dx_value(m["dz"], k["x"], got["mean"], bw, bb)
        bad = bo.check_interval(m["dx"], v, e, dtype)[0]
        assert bad == 0, f"{where}: {bad} dx elements outside the bound"


@pytest.mark.parametrize("chunks", [1, 33, 257, 2049, 16385])
def test_finalize_from_partials_is_good_to_a_few_ulps(chunks):
    """Partials handed in as fp32 numbers: the bound is the finalize's own, a few fp32 ulps."""
    M, C = 16390, 8
    k = bo.case(M, C, torch.bfloat16, CPU)
    gid = bo.partition(M, chunks, CPU)
    assert gid.max().item() + 1 == (chunks - 1 if chunks > 1 else 1) and torch.all(gid[1:] >= gid[:-1])
    sizes = torch.bincount(gid, minlength=chunks)
    assert sizes.sum().item() == M and (chunks == 1 or (sizes[-1] == 0 and sizes[:-1].min() >= 1))
    assert chunks < 4 or sizes[:-1].max() > sizes[:-1].min()
    xd = k["x"].double()
    ps, pq = bo.group_sums(xd, gid, chunks), bo.group_sums(xd * xd, gid, chunks)
    assert ps.shape == (C, chunks)
    s, q, e_s, e_q = bo.partial_sums(ps, pq)
    want, bound = bo.fwd_finalize(s, q, e_s, e_q, M, k["gamma"], k["beta"], 1e-5, 0.1, k["rm0"], k["rv0"])
    ulps = {"mean": 1.01, "invstd": 1.01, "a": 2.01, "b": 6.0, "running_mean": 5.0, "running_var": 5.0}
    for n, u in ulps.items():
        scale = want[n].abs() if n != "b" else want[n].abs() + (want["mean"] * want["a"]).abs()
        if n.startswith("running"):
            scale = scale + (k["rm0"] if n == "running_mean" else k["rv0"]).double().abs()
        assert torch.all(bound[n] <= u * bo.U * scale), n


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=lambda d: str(d).replace("torch.", ""))
def test_conditioning_bound_at_the_stem_statistics(dtype, capsys):
    """|mean| / std up to 60: what the worst-case bound leaves of var and invstd, at the test's
    geometry and at the stem's real one (M = 64*112*112: rows_per_chunk 1568, rpi 32)."""
    k, ratio = _cond_case(dtype)
    for geo in (k["geo"], bo.geometry(64 * 112 * 112, 64)):
        s, q, e_s, e_q = bo.fwd_sums(k["x"], geo)
        want, bound = bo.fwd_finalize(s, q, e_s, e_q, k["M"], k["gamma"], k["beta"], 1e-5, 0.1, k["rm0"], k["rv0"])
        rel_var = (bound["var"] / want["var"])
        rel_inv = (bound["invstd"] / want["invstd"])
        with capsys.disabled():
            print(f"\n{dtype} rows_per_chunk={geo['rows_per_chunk']} rpi={geo['rpi']}: bound on var, relative, at "
                  f"|mean|/std = 1: {rel_var[0]:.2e}, 60: {rel_var[-1]:.2e}; on invstd at 60: {rel_inv[-1]:.2e}")
        # the bound grows as (mean/std)^2 and still leaves invstd two digits at the test's geometry
        assert rel_var[-1] > 100 * rel_var[0]
    got = bo.model_fwd(k["x"], k["geo"], k["gamma"], k["beta"], 1e-5, 0.1, k["rm0"], k["rv0"])
    s, q, e_s, e_q = bo.fwd_sums(k["x"], k["geo"])
    want, bound = bo.fwd_finalize(s, q, e_s, e_q, k["M"], k["gamma"], k["beta"], 1e-5, 0.1, k["rm0"], k["rv0"])
    assert (bound["invstd"] / want["invstd"]).max().item() < 2e-2
    assert bo.worst_ratio(got["var"], want["var"], bound["var"]) <= 1.0
    assert bo.worst_ratio(got["invstd"], want["invstd"], bound["invstd"]) <= 1.0


def test_special_values_of_the_mask_rule():
    """dz_exact / mask rules on the values the GPU test feeds: y > 0 is an IEEE compare."""
    for dtype in bo.DTYPES:
        fi = torch.finfo(dtype)
        y = torch.tensor([0.0, -0.0, fi.smallest_normal, fi.smallest_normal * fi.eps, float("inf"), float("-inf"), float("nan"), -1.0],
                         dtype=dtype)
        assert (y > 0).tolist() == [False, False, True, True, True, False, False, False]
        dy = torch.full((8,), -0.75, dtype=dtype)
        dz = bo.dz_exact(dy, None, y > 0)
        assert dz.tolist() == [0, 0, -0.75, -0.75, -0.75, 0, 0, 0]
        assert not torch.signbit(dz[0]) and not torch.signbit(dz[6])
