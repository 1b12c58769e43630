"""Every launch path of the 16-bit implicit-GEMM convolutions (csrc/kernels/conv_kernels.hip) against
the exact-integer oracle of tests/conv_oracle.py: outputs and BatchNorm partials compared BIT FOR
BIT with one fp64 CPU reference, in three operand regimes (sharp / rounded / one-hot, see the
oracle's docstring), at the tile edges (M = 25, 128, 129, 147, 300, a tile across two images; C =
64 / 128 / 192; Cout = 64 / 128 / 192 / 256) and geometries (1x1, strided, 3x3 with every tap on a
border, 5x5, 7x7 / 2, the narrow stem inputs with an explicit output size).

Every test that names a path asserts from the launch trace (``conv_trace`` / ``conv_trace_take``)
that this kernel, with these template arguments, is what ran - a knob that silently falls back to
another kernel fails here.  Pinned that way: ``conv_set_variant`` 7 / 8 / 14 and
``conv_set_fwd_shape_policy`` bits 4 / 8 name the BK = 32 pipelined K loops but run the 256-row
LDS-epilogue tile (conv_fwd_dispatch tests ``variant >= 5`` first).  ``conv_fwd_pipe_kernel`` is
therefore unreachable from every binding and UNTESTED, here and anywhere else.

The eager split-K policy would split several of these small grids on its own, so every test runs
with ``conv_set_splitk(0)`` unless split-K is the path under test (``conv_set_splitk(2)``).
Out of scope: the tail-fused 1x1 kernels, conv_f32_kernels.hip and the DGELU epilogue.
"""
import functools

import pytest
import torch

import conv_oracle as co
from distributed_pytorch_training_amd import ops

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = [BF16, F16]
DT_ID = {BF16: "bf16", F16: "f16"}.get
INT_REGIMES = ("sharp", "rounded")
FLAG_ORDER = ["kLdsEpi", "kBkn", "kStats", "kBnb", "kBnr", "kRemap", "kZsib", "kBnr2", "kF16", "kSplit", "kHalo",
              "kSk", "kDgelu", "kBreg", "kDir", "kRs2"]

# shapes only the knobs below need (N, C, H, W, Cout, k, stride, pad)
EXTRA_FWD = {
    "k2048-n512": (1, 2048, 5, 5, 512, 1, 1, 0),      # conv_set_big(1) -> 256 x 128 8-wave tile
    "k1024-n256": (1, 1024, 5, 5, 256, 1, 1, 0),      # conv_set_big(2) -> 128 x 256, 3 stages
    "k512-n256": (1, 512, 5, 5, 256, 1, 1, 0),        # conv_set_big(3)
    # The one workload-sized shape (67 MB operand, ~2 s of fp64 reference): policy bit 2 and conv_set_big(1)
    # select their 256 x 256 tile only at M >= 32768 with C = Cout = 256 (fwd_shape_variant, conv_big_auto), so
    # no smaller shape reaches that path.  Sharp regime only; its fp64 reference is dropped once y is built.
    "3x3s2-m32768": (8, 256, 128, 128, 256, 3, 2, 1),
    "sk-264tiles": (2, 192, 64, 66, 512, 1, 1, 0),    # smallest stream-K grid that cuts tiles (66 x 4 tiles, 3 K-steps)
}
DGRAD_BN_SHAPES = {
    "1x1-m300": co.FWD_SHAPES["m300-1x1"],            # dx C = 128: 256 x 128 8-wave tiles; splits in two
    "3x3-m147": co.FWD_SHAPES["3x3-m147"],            # dx C = 64: halo K loop, 18 K-steps
    "1x1-c256": (3, 256, 10, 10, 64, 1, 1, 0),        # dx C = 256: the 256-wide 8-wave tiles
}
WGRAD_LONG = (2, 64, 32, 32, 64, 1, 1, 0)             # 32 K-steps, one tile: 1 .. 16 splits
WGRAD_V20 = (1, 256, 6, 6, 256, 1, 1, 0)


def flags(*names):
    got = [f for f in FLAG_ORDER if f in names]
    assert len(got) == len(set(names)), names
    return "|".join(got) or "0"


def parse(trace):
    """Trace lines -> dicts of their fields; "op" is the record's first word."""
    return [dict([("op", line.split()[0])] + [t.split("=", 1) for t in line.split()[1:]]) for line in trace]


def expect(trace, op, count=1, **kw):
    """The trace holds exactly ``count`` records of ``op``, all with these fields."""
    recs = [r for r in parse(trace) if r["op"] == op]
    assert len(recs) == count, (op, count, trace)
    for r in recs:
        for k, v in kw.items():
            assert r[k] == str(v), (k, v, trace)
    return recs


@pytest.fixture(autouse=True)
def n(cuda):
    """The extension with tracing on and split-K off; every knob back to its value afterwards."""
    C_ = ops.native()
    old = (C_.conv_get_splitk(), C_.conv_get_streamk(), C_.conv_get_breg())
    C_.conv_set_splitk(0)
    C_.conv_trace(True)
    C_.conv_trace_take()
    yield C_
    torch.cuda.synchronize()
    C_.conv_trace(False)
    C_.conv_trace_take()
    C_.conv_set_variant(0)
    C_.conv_set_halo(1)
    C_.conv_set_big(0)
    C_.conv_set_fwd_shape_policy(0)
    C_.conv_set_wgrad_stages(0)
    C_.conv_set_wgrad_halo(5)
    C_.conv_set_splitk(old[0])
    C_.conv_set_streamk(old[1])
    C_.conv_set_breg(old[2])


# ---- expected tensors: built on the CPU once per (pass, shape, regime, dtype) ---------------------------
def _shape(name):
    if name in co.NARROW_SHAPES:
        return co.NARROW_SHAPES[name]
    for d in (co.FWD_SHAPES, EXTRA_FWD, DGRAD_BN_SHAPES, co.DGRAD_S2_SHAPES):
        if name in d:
            return d[name], 0, 0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def fwd_case(name, regime, dtype):
    shape, oh, ow = _shape(name)
    case = co.fwd_case(shape, regime, dtype, seed=1, out_h=oh, out_w=ow)
    if name == "3x3s2-m32768":
        del case["ref"]  # the cache lives as long as the session
    return case


@functools.lru_cache(maxsize=None)
def dgrad_case(name, regime, dtype):
    return co.dgrad_case(_shape(name)[0], regime, dtype, seed=2)


@functools.lru_cache(maxsize=None)
def wgrad_case(name, regime, dtype):
    if name == "long":
        return co.wgrad_case(WGRAD_LONG, regime, dtype, seed=3)
    if name == "v20":
        return co.wgrad_case(WGRAD_V20, regime, dtype, seed=3)
    shape, oh, ow = _shape(name)
    return co.wgrad_case(shape, regime, dtype, seed=3, out_h=oh, out_w=ow)


def run_fwd(n, cuda, name, regime, dtype, stats, split=False):
    """conv_fwd on the case's operands: y (and the partials where they are exact) bit for bit;
    returns the launch trace."""
    shape, oh, ow = _shape(name)
    case = fwd_case(name, regime, dtype)
    n.conv_trace_take()
    y, ps, pq = n.conv_fwd(case["x"].to(cuda), case["w"].to(cuda), shape[6], shape[7], stats, oh, ow)
    trace = n.conv_trace_take()
    what = f"conv_fwd {name} {regime} {DT_ID(dtype)} stats={stats} {trace}"
    co.assert_bits(y, case["y"], what + " y", bn=128 if shape[4] % 128 == 0 else 64)
    if stats:
        M = y.shape[0] * y.shape[2] * y.shape[3]
        cols = co.split_cols(M) if split else co.m_tiles(M)
        assert ps.shape == pq.shape == (shape[4], cols), (ps.shape, cols)
        if case["psum_exact"]:  # (fp16 / rounded: the squares pass 2^24, psum alone is exact)
            eps, epq = co.stat_partials(case["y"], co.SPLIT_ROWS if split else co.BM, want_sq=case["psq_exact"])
            co.assert_bits(ps, eps, what + " psum")
            if case["psq_exact"]:
                co.assert_bits(pq, epq, what + " psq")
    return trace


def bn_of(shape):
    return 128 if shape[4] % 128 == 0 else 64


def is_halo(shape, oh=0):
    N, C, H, W, Cout, k, s, p = shape
    return k == 3 and s == 1 and p == 1 and C % 64 == 0 and not oh


def all_regimes(fn):
    """Run fn(regime, stats) over the four regimes: the integer ones with and without statistics."""
    for regime in co.REGIMES:
        for stats in ((True, False) if regime in INT_REGIMES else (False,)):
            fn(regime, stats)


# ---- forward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("regime", co.REGIMES)
@pytest.mark.parametrize("name", list(co.FWD_SHAPES) + list(co.NARROW_SHAPES))
def test_fwd_production_tile(n, cuda, name, regime, dtype):
    """Variant 0: the 128-row 1-stage LDS-epilogue tile, the halo K loop (all three B taps per
    phase on these small grids) for 3x3 / stride 1 / pad 1."""
    shape, oh, ow = _shape(name)
    for stats in (True, False):
        trace = run_fwd(n, cuda, name, regime, dtype, stats)
        halo = is_halo(shape, oh)
        f = ["kLdsEpi"] + ["kStats"] * stats + ["kF16"] * (dtype == F16) + ["kHalo"] * halo
        expect(trace, "fwd", BM=128, BN=bn_of(shape), STAGES=1, F=flags(*f), NT=256, HB=3 if halo else 1, carry=0)
        assert len(trace) == 1, trace


VARIANT_SHAPES = ["m25-1x1", "m129-1x1", "m147-1x1", "m300-1x1", "3x3-m300", "3x3s2"]
BIG_TILES = {9: (256, 256, 2), 10: (256, 128, 2), 11: (128, 256, 2), 12: (256, 128, 3), 13: (128, 256, 3)}


def _variant_record(v, shape, stats):
    """What conv_fwd launches under conv_set_variant(v) (bf16), from conv_fwd_impl / conv_fwd_dispatch
    / conv_fwd_big: the fields of its trace record."""
    bn, cout = bn_of(shape), shape[4]
    if v in BIG_TILES and cout % BIG_TILES[v][1] == 0:
        bm, bnb, st = BIG_TILES[v]
        return dict(BM=bm, BN=bnb, STAGES=st, NT=512, F=flags("kLdsEpi", *["kStats"] * stats))
    if v >= 5:  # 5 - 8, 14, and 9 - 13 where the wide tile does not divide Cout: 256-row blocks
        return dict(BM=256, BN=bn, STAGES=1, NT=256, F=flags("kStats") if v == 5 else flags("kLdsEpi", "kStats"))
    if v == 4:
        halo = is_halo(shape)
        return dict(BM=128, BN=bn, STAGES=1, NT=256, HB=3 if halo else 1,
                    F=flags("kLdsEpi", *["kStats"] * stats, *["kHalo"] * halo))
    return dict(BM=128, BN=bn, NT=256, STAGES=1 if v == 3 else 2,
                F=flags("kStats") if v in (2, 3) else flags("kLdsEpi", "kStats"))


@pytest.mark.parametrize("v,name", [(v, s) for v in (1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13) for s in VARIANT_SHAPES]
                         + [(8, "m300-1x1"), (14, "m300-1x1")])   # one shape pins the two aliases of 7
def test_fwd_variants(n, cuda, v, name):
    """conv_set_variant 1 - 6 and the 8-wave tiles 9 - 13; Cout = 192 (3x3-m300, m129-1x1) is
    divided by no 128- or 256-wide tile: the documented fallback to the 256-row block.  7, 8 and
    14 run the same 256-row LDS-epilogue kernel as 6 (module docstring)."""
    n.conv_set_variant(v)

    def one(regime, stats):
        trace = run_fwd(n, cuda, name, regime, BF16, stats)
        expect(trace, "fwd", carry=0, **_variant_record(v, _shape(name)[0], stats))
        assert len(trace) == 1, trace

    all_regimes(one)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("name", ["3x3-h1", "3x3-h2", "3x3-5x6", "3x3-m147", "3x3-m300"])
@pytest.mark.parametrize("halo", [0, 2, 3])
def test_fwd_halo_modes(n, cuda, halo, name, dtype):
    n.conv_set_halo(halo)

    def one(regime, stats):
        trace = run_fwd(n, cuda, name, regime, dtype, stats)
        f = ["kLdsEpi"] + ["kStats"] * stats + ["kF16"] * (dtype == F16) + ["kHalo"] * (halo != 0)
        expect(trace, "fwd", BM=128, STAGES=1, F=flags(*f), HB=3 if halo == 3 else 1)

    all_regimes(one)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("name", ["3x3-m147", "3x3-5x6", "m147-1x1", "m129-1x1", "3x3s2", "7x7s2"])
@pytest.mark.parametrize("breg", [1, 2, 3])
def test_fwd_b_operand_in_registers(n, cuda, breg, name, dtype):
    """conv_set_breg: bit 0 the halo convs, bit 1 the others."""
    n.conv_set_breg(breg)
    halo = is_halo(_shape(name)[0])

    def one(regime, stats):
        trace = run_fwd(n, cuda, name, regime, dtype, stats)
        on = bool(breg & (1 if halo else 2))
        f = (["kLdsEpi"] + ["kStats"] * stats + ["kF16"] * (dtype == F16) + ["kHalo"] * halo + ["kBreg"] * on)
        expect(trace, "fwd", BM=128, STAGES=1, F=flags(*f), HB=1 if on or not halo else 3)

    all_regimes(one)


@pytest.mark.parametrize("bits,name,rec", [
    (1, "m300-1x1", dict(BM=256, STAGES=1, NT=256, F="kLdsEpi|kStats")),
    (2, "3x3s2-m32768", dict(BM=256, BN=256, STAGES=2, NT=512, F="kLdsEpi|kStats")),
    # 4 / 8 ask for the pipelined K loops (codes 14 / 7): conv_fwd_dispatch runs the 256-row tile
    (4, "m147-1x1", dict(BM=256, STAGES=1, NT=256, F="kLdsEpi|kStats")),
    (8, "m147-1x1", dict(BM=256, STAGES=1, NT=256, F="kLdsEpi|kStats")),
    (16, "c16-4x4", dict(BM=128, STAGES=2, NT=256, F="kLdsEpi|kStats")),
], ids=lambda v: str(v) if isinstance(v, (int, str)) else "")
def test_fwd_shape_policy_bits(n, cuda, bits, name, rec):
    """Each bit selects its tile at a shape that meets its rule, and only with the statistics
    epilogue where the rule says so (bits 1, 4, 8)."""
    n.conv_set_fwd_shape_policy(bits)
    regimes = ("sharp",) if name == "3x3s2-m32768" else ("sharp", "rounded", "one-hot-b")
    for regime in regimes:
        trace = run_fwd(n, cuda, name, regime, BF16, True)
        expect(trace, "fwd", **rec)
    if bits in (1, 4, 8):
        trace = run_fwd(n, cuda, name, "sharp", BF16, False)
        expect(trace, "fwd", BM=128, STAGES=1, NT=256, F="kLdsEpi")


@pytest.mark.parametrize("big,name,tile", [
    (1, "k2048-n512", (256, 128, 2)), (1, "3x3s2-m32768", (256, 256, 2)),
    (2, "k1024-n256", (128, 256, 3)), (3, "k512-n256", (128, 256, 3)),
], ids=lambda v: str(v) if isinstance(v, (int, str)) else "")
def test_fwd_big_auto(n, cuda, big, name, tile):
    """conv_set_big 1 - 3 (conv_big_auto); one step below its rule (big = 2 at K = 512) the
    production tile runs."""
    n.conv_set_big(big)
    for regime in (("sharp",) if name == "3x3s2-m32768" else ("sharp", "rounded", "one-hot-a", "one-hot-b")):
        stats = regime in INT_REGIMES
        trace = run_fwd(n, cuda, name, regime, BF16, stats)
        expect(trace, "fwd", BM=tile[0], BN=tile[1], STAGES=tile[2], NT=512, F=flags("kLdsEpi", *["kStats"] * stats))
    if big == 2:
        expect(run_fwd(n, cuda, "k512-n256", "sharp", BF16, True), "fwd", BM=128, BN=128, STAGES=1, NT=256)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("name", ["3x3-m147", "3x3-5x6", "3x3-m300", "5x5", "7x7s2", "3x3-h1"])
def test_fwd_split_k(n, cuda, name, dtype):
    """conv_set_splitk(2): the in-graph policy everywhere.  3x3-m147: 9 K-steps in 5 splits of 2 (the
    last holds one), M = 147 is no multiple of the 16-row slabs; 3x3-m300: 64-wide tiles."""
    shape = _shape(name)[0]
    N, C, H, W, Cout, k, s, p = shape
    Ho, Wo = co.out_hw(H, W, k, s, p)
    n.conv_set_splitk(2)
    splits = n.conv_fwd_splits(N * Ho * Wo, Cout, k * k * C, True)
    assert splits > 1, splits
    if name == "3x3-m147":
        assert splits == 5 and (N * Ho * Wo) % 16 != 0

    def one(regime, stats):
        trace = run_fwd(n, cuda, name, regime, dtype, stats, split=True)
        f16 = ["kF16"] * (dtype == F16)
        expect(trace, "fwd", BM=128, BN=bn_of(shape), STAGES=1, NT=256, F=flags("kLdsEpi", "kSplit", *f16),
               splits=splits)
        expect(trace, "split_epilogue", F=flags(*["kStats"] * stats, *f16), splits=splits)
        assert [r["op"] for r in parse(trace)] == ["fwd", "split_epilogue"]

    all_regimes(one)


def test_fwd_stream_k(n, cuda):
    """conv_set_streamk(2) at the smallest grid whose tiles are cut between blocks: 264 tiles of 3
    K-steps over 512 blocks."""
    shape = EXTRA_FWD["sk-264tiles"]
    tiles, nk = co.m_tiles(shape[0] * shape[2] * shape[3]) * (shape[4] // 128), shape[1] // 64
    assert tiles == 264 and n.conv_sk_blocks(tiles, nk, 128, 2) == 512 and n.conv_sk_blocks(255, nk, 128, 2) == 0
    n.conv_sk_prepare()
    n.conv_set_streamk(2)

    def one(regime, stats):
        trace = run_fwd(n, cuda, "sk-264tiles", regime, BF16, stats)
        expect(trace, "fwd", BM=128, BN=128, STAGES=1, F=flags("kLdsEpi", *["kStats"] * stats, "kSk"), skG=512,
               grid="512x1")

    all_regimes(one)
    assert n.conv_sk_errors() == 0


# ---- backward-data, stride 1 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("regime", co.REGIMES)
@pytest.mark.parametrize("name", list(co.DGRAD_SHAPES))
def test_dgrad_three_bindings_same_bits(n, cuda, name, regime, dtype):
    """conv_dgrad (flip folded into the B addressing), conv_dgrad_flip (explicit flipped copy) and
    conv_dgrad_preflipped, unsplit and through split-K where the policy splits."""
    shape = _shape(name)[0]
    N, C, H, W, Cout, k, s, p = shape
    case = dgrad_case(name, regime, dtype)
    dy, w = case["dy"].to(cuda), case["w"].to(cuda)
    bn = 128 if C % 128 == 0 else 64
    f16 = ["kF16"] * (dtype == F16)
    halo = k == 3 and p == 1
    what = f"{name} {regime} {DT_ID(dtype)}"

    n.conv_trace_take()
    dx = n.conv_dgrad(dy, w, p)
    expect(n.conv_trace_take(), "fwd", BM=128, BN=bn, STAGES=1, NT=256, F=flags("kLdsEpi", "kBkn", "kStats", *f16))
    co.assert_bits(dx, case["dx"], "conv_dgrad " + what, bn)

    for mode in (0, 2):
        n.conv_set_splitk(mode)
        split = mode == 2 and n.conv_fwd_splits(N * H * W, C, k * k * Cout, True) > 1
        if mode == 2 and not split:
            continue
        dx2, wt = n.conv_dgrad_flip(dy, w, p)
        t2 = n.conv_trace_take()
        dx3 = n.conv_dgrad_preflipped(dy, wt, p)
        t3 = n.conv_trace_take()
        assert torch.equal(wt, w.flip(2, 3).transpose(0, 1).contiguous(memory_format=co.CL))
        for t in (t2, t3):
            if split:
                expect(t, "fwd", BM=128, BN=bn, F=flags("kLdsEpi", "kSplit", *f16))
                expect(t, "split_epilogue", F=flags(*f16))
            else:
                expect(t, "fwd", BM=128, BN=bn, STAGES=1, F=flags("kLdsEpi", *f16, *["kHalo"] * halo))
        co.assert_bits(dx2, case["dx"], f"conv_dgrad_flip splitk={mode} " + what, bn)
        co.assert_bits(dx3, case["dx"], f"conv_dgrad_preflipped splitk={mode} " + what, bn)


EPILOGUES = {
    # name: (bn_epilogue_inputs kwargs, flags of the epilogue, use bn_mask)
    "plain": (dict(), ["kBnb"], False),
    "bnr": (dict(res=True), ["kBnb", "kBnr"], False),
    "bnr-mask": (dict(res=True), ["kBnb", "kBnr"], True),
    "bnr2": (dict(res=True, x2=True), ["kBnb", "kBnr", "kBnr2"], False),
    "rs2": (dict(res=True, res_s2=True), ["kBnb", "kBnr", "kRs2"], False),
}


def _bnstats(n, cuda, name, epi, dtype, regime):
    """Call conv_dgrad_bnstats on the regime's case with the epilogue's inputs; returns (trace,
    checker of the outputs, the epilogue's flags).  Integer regimes: dx and every partial; rounded
    with a residual: g + res is mostly not representable, and the partials expected (summed from the
    fp32 dz) must differ from those of the stored dz, so the case tells the two readings apart;
    one-hot: dx alone (the sums of arbitrary patterns are not exact)."""
    shape = _shape(name)[0]
    N, C, H, W, Cout, k, s, p = shape
    case = dgrad_case(name, regime, dtype)
    kw, fl, use_mask = EPILOGUES[epi]
    bn = co.bn_epilogue_inputs((N, C, H, W), dtype, seed=7, **kw)
    d = {key: v.to(cuda) for key, v in bn.items()}
    n.conv_trace_take()
    out = n.conv_dgrad_bnstats(case["dy"].to(cuda), case["w"].to(cuda), p, d["bn_x"], d["bn_mean"], d["bn_coef"],
                               bn_y=d.get("bn_y"), bn_res=d.get("bn_res"), bn_x2=d.get("bn_x2"),
                               bn_mean2=d.get("bn_mean2"), bn_mask=d["bn_mask"] if use_mask else None,
                               bn_res_s2=bool(kw.get("res_s2")))
    trace = n.conv_trace_take()

    def check(rows_per_col, block_rows=None):
        rs2, stats = bool(kw.get("res_s2")), regime in INT_REGIMES
        dx, p1, p2, p3 = co.dgrad_bn_expected(case["dx"], bn, dtype, rows_per_col, block_rows, rs2, stats=stats)
        what = f"conv_dgrad_bnstats {name} {epi} {regime} {DT_ID(dtype)} {trace}"
        co.assert_bits(out[0], dx, what + " dx", 128 if C % 128 == 0 else 64)
        if not stats:
            return
        if regime == "rounded" and "bn_y" in bn:
            other = co.dgrad_bn_expected(case["dx"], bn, dtype, rows_per_col, block_rows, rs2, from_stored=True)
            assert torch.equal(other[0], dx) and not torch.equal(other[1], p1) and not torch.equal(other[2], p2)
        co.assert_bits(out[1], p1, what + " p1")
        co.assert_bits(out[2], p2, what + " p2")
        if p3 is not None:
            co.assert_bits(out[3], p3, what + " p3")
        else:
            assert out[3].numel() == 0

    return trace, check, fl


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("mode,name", [("unsplit", k) for k in DGRAD_BN_SHAPES] + [("split", "1x1-m300"),
                                                                                    ("split", "3x3-m147")])
def test_dgrad_bnstats_epilogues(n, cuda, mode, name, epi, dtype):
    """dx and every partial of the BNB / BNR / BNR2 / RS2 epilogues in every regime, from the 128-row
    tile (128-row partials) and from the split-K epilogue kernel (16-row slabs; 1x1-c256 has one
    K-step and never splits).  The rounded regime pins that the plain epilogue sums the ROUNDED g
    and that BNR sums the fp32 g + res before its rounding for the store."""
    shape = _shape(name)[0]
    N, C, H, W, Cout, k, s, p = shape
    f16 = ["kF16"] * (dtype == F16)
    if mode == "split":
        n.conv_set_splitk(2)
        assert n.conv_fwd_splits(N * H * W, C, k * k * Cout, True) > 1
    for regime in co.REGIMES:
        trace, check, fl = _bnstats(n, cuda, name, epi, dtype, regime)
        expect(trace, "fwd", count=1)
        if mode == "split":
            expect(trace, "fwd", F=flags("kLdsEpi", "kSplit", *f16))
            expect(trace, "split_epilogue", F=flags(*fl, *f16))
            check(co.SPLIT_ROWS)
        else:
            halo = k == 3 and p == 1 and "kRs2" not in fl
            expect(trace, "fwd", BM=128, STAGES=1, NT=256, F=flags("kLdsEpi", *fl, *f16, *["kHalo"] * halo))
            check(co.BM)


@pytest.mark.parametrize("epi", ["plain", "bnr", "bnr-mask", "bnr2"])
@pytest.mark.parametrize("v,name", [(10, "1x1-m300"), (12, "1x1-m300"), (9, "1x1-c256"), (13, "1x1-c256")])
def test_dgrad_bnstats_eight_wave_tiles(n, cuda, v, name, epi):
    """conv_set_variant 9, 10, 12, 13 (bf16; RS2 stays on the 4-wave tile): a 256-row block writes
    its whole sum into its first 128-row column and zero into its second."""
    n.conv_set_variant(v)
    bm, bnw, st = BIG_TILES[v]
    for regime in co.REGIMES:
        trace, check, fl = _bnstats(n, cuda, name, epi, BF16, regime)
        expect(trace, "fwd", BM=bm, BN=bnw, STAGES=st, NT=512, F=flags("kLdsEpi", *fl))
        check(co.BM, block_rows=bm)


def test_dgrad_bnstats_rs2_ignores_eight_wave_variant(n, cuda):
    n.conv_set_variant(10)
    for regime in INT_REGIMES:
        trace, check, fl = _bnstats(n, cuda, "1x1-m300", "rs2", BF16, regime)
        expect(trace, "fwd", BM=128, BN=128, STAGES=1, NT=256, F=flags("kLdsEpi", *fl))
        check(co.BM)


# ---- backward-data, stride 2 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("regime", co.REGIMES)
@pytest.mark.parametrize("name", list(co.DGRAD_S2_SHAPES))
def test_dgrad_s2(n, cuda, name, regime, dtype):
    """One REMAP launch per non-empty parity class; a 1x1 kernel has one class, whose launch also
    writes the zeros of the three classes without taps (ZSIB) - up to the border on odd images - and
    its compact form is that class as it leaves the GEMM."""
    N, C, H, W, Cout, k, s, p = _shape(name)[0]
    case = dgrad_case(name, regime, dtype)
    dy, w = case["dy"].to(cuda), case["w"].to(cuda)
    f16 = ["kF16"] * (dtype == F16)
    classes = co.s2_classes(H, W, k, k, p)
    assert len(classes) == (1 if k == 1 else 4)
    n.conv_trace_take()
    dx = n.conv_dgrad_s2(dy, w, p, H, W)[0]
    trace = n.conv_trace_take()
    expect(trace, "fwd", count=len(classes), BM=128, STAGES=1,
           F=flags("kLdsEpi", "kBkn", "kRemap", *["kZsib"] * (k == 1), *f16))
    co.assert_bits(dx, case["dx"], f"conv_dgrad_s2 {name} {regime} {DT_ID(dtype)}", 128 if C % 128 == 0 else 64)
    if k == 1:
        dxc = n.conv_dgrad_s2(dy, w, p, H, W, compact=True)[0]
        expect(n.conv_trace_take(), "fwd", F=flags("kLdsEpi", "kBkn", *f16))
        co.assert_bits(dxc, case["dx"][:, :, ::2, ::2].contiguous(memory_format=co.CL), f"compact {name} {regime}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("regime", co.REGIMES)
@pytest.mark.parametrize("mode", [0, 2], ids=["unsplit", "splitk"])
@pytest.mark.parametrize("name", ["3x3-oddeven", "3x3-even", "7x7"])
def test_dgrad_s2_bn_statistics(n, cuda, name, mode, regime, dtype):
    """The plain BNB epilogue per class: the classes' partials fill consecutive column ranges of one
    array (128-row columns, 16-row columns for a class that split-K took).  Rounded regime: the
    statistics come from the rounded gradient; one-hot: dx alone."""
    N, C, H, W, Cout, k, s, p = _shape(name)[0]
    case = dgrad_case(name, regime, dtype)
    bn = co.bn_epilogue_inputs((N, C, H, W), dtype, seed=9)
    n.conv_set_splitk(mode)
    split = (lambda M, taps: n.conv_fwd_splits(M, C, taps * Cout, True) > 1) if mode == 2 else None
    cols, total = co.dgrad_s2_chunks(N, H, W, k, k, p, split)
    if mode == 2:
        assert any(c[4] == co.SPLIT_ROWS for c in cols), cols
    n.conv_trace_take()
    dx, p1, p2 = n.conv_dgrad_s2(case["dy"].to(cuda), case["w"].to(cuda), p, H, W, bn["bn_x"].to(cuda),
                                 bn["bn_mean"].to(cuda), bn["bn_coef"].to(cuda))
    trace = n.conv_trace_take()
    f16 = ["kF16"] * (dtype == F16)
    n_split = sum(c[4] == co.SPLIT_ROWS for c in cols)
    expect(trace, "split_epilogue", count=n_split, F=flags("kBkn", "kBnb", "kRemap", *f16))
    recs = [r for r in parse(trace) if r["op"] == "fwd"]
    assert len(recs) == len(cols), trace
    for r, c in zip(recs, cols):
        want = ("kLdsEpi", "kBkn", "kSplit") if c[4] == co.SPLIT_ROWS else ("kLdsEpi", "kBkn", "kBnb", "kRemap")
        assert r["F"] == flags(*want, *f16), trace
    what = f"conv_dgrad_s2 bnstats {name} {regime} splitk={mode} {DT_ID(dtype)} {cols}"
    co.assert_bits(dx, case["dx"], what + " dx")
    assert p1.shape == p2.shape == (C, total)
    if regime not in INT_REGIMES:
        return
    e1, e2 = torch.zeros(C, total), torch.zeros(C, total)
    for ph, pw, off, ncol, rpc in cols:
        sub = {key: (v[:, :, ph::2, pw::2] if v.dim() == 4 else v) for key, v in bn.items()}
        _, q1, q2, _ = co.dgrad_bn_expected(case["dx"][:, :, ph::2, pw::2], sub, dtype, rpc)
        e1[:, off:off + ncol], e2[:, off:off + ncol] = q1, q2
    co.assert_bits(p1, e1, what + " p1")
    co.assert_bits(p2, e2, what + " p2")


# ---- backward-weight -----------------------------------------------------------------------------------------
def check_dw(dw, case, fp32_out, what):
    co.assert_bits(dw, case["dw32"] if fp32_out else case["dw16"], what)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("regime", co.REGIMES)
@pytest.mark.parametrize("name", list(co.WGRAD_SHAPES) + list(co.NARROW_SHAPES))
def test_wgrad(n, cuda, name, regime, dtype):
    """conv_wgrad with fp32 and 16-bit output, single-stage and (bf16) double-buffered K loop; the
    output size comes from dy (the narrow stem shapes pad on the top and left only)."""
    shape, oh, ow = _shape(name)
    N, C, H, W, Cout, k, s, p = shape
    case = wgrad_case(name, regime, dtype)
    dy, x = case["dy"].to(cuda), case["x"].to(cuda)
    halo = k == 3 and s == 1 and p == 1 and C == 64  # conv_set_wgrad_halo's default: 64-channel strips
    # the per-tap tile as conv_wgrad_plan states it: 128 output channels where Cout allows; columns =
    # 128 input channels of a tap, two taps of a 64-channel input, all 16 taps of the 16-channel stem
    bmw = 128 if Cout % 128 == 0 else 64
    bnw = 128 if C % 128 == 0 or (C == 64 and k > 1) else 256 if (C == 16 and k * k * C >= 256 and bmw == 64) else 64
    direct = k == 1 and s == 1 and p == 0
    for stages in ((0, 2) if dtype == BF16 else (0,)):
        n.conv_set_wgrad_stages(stages)
        for fp32_out in (True, False):
            n.conv_trace_take()
            dw = n.conv_wgrad(dy, x, case["wshape"], s, p, fp32_out)
            trace = n.conv_trace_take()
            if halo:
                rec = expect(trace, "wgrad_halo", BNW=64, STAGES=1)[0]
            else:
                two = stages == 2 and bnw <= 128
                f = ["kF16"] if dtype == F16 else ["kDir"] if direct and not two else []
                rec = expect(trace, "wgrad", BMW=bmw, BNW=bnw, NT=256, STAGES=2 if two else 1, F=flags(*f))[0]
            expect(trace, "wgrad_reduce", count=0 if (rec["splits"] == "1" and fp32_out) else 1)
            check_dw(dw, case, fp32_out,
                     f"conv_wgrad {name} {regime} {DT_ID(dtype)} stages={stages} fp32={fp32_out} {trace}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("name", ["3x3-m147", "3x3-m300"])  # C = 64 and 128
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_wgrad_halo_modes(n, cuda, mode, name, dtype):
    """conv_set_wgrad_halo 0 - 4: modes 1 / 2 take 128-channel strips (C = 64 stays on the per-tap
    kernel), 3 / 4 64-channel strips; even modes double-buffer."""
    N, C, H, W, Cout, k, s, p = _shape(name)[0]
    n.conv_set_wgrad_halo(mode)
    for regime in co.REGIMES:
        case = wgrad_case(name, regime, dtype)
        n.conv_trace_take()
        dw = n.conv_wgrad(case["dy"].to(cuda), case["x"].to(cuda), case["wshape"], s, p, True)
        trace = n.conv_trace_take()
        if mode == 0 or (mode in (1, 2) and C % 128):
            expect(trace, "wgrad")
            expect(trace, "wgrad_halo", count=0)
        else:
            expect(trace, "wgrad_halo", BNW=128 if mode in (1, 2) else 64, STAGES=2 if mode in (2, 4) else 1,
                   F=flags(*["kF16"] * (dtype == F16)))
        check_dw(dw, case, True, f"wgrad_halo mode {mode} {name} {regime} {DT_ID(dtype)} {trace}")


@pytest.mark.parametrize("fp32_out", [True, False], ids=["f32", "16bit"])
@pytest.mark.parametrize("target,splits,ph", [(1, 1, 1), (2, 2, 1), (4, 4, 4), (512, 16, 16)])
def test_wgrad_split_counts_and_reduce_phases(n, cuda, target, splits, ph, fp32_out):
    """target_blocks forcing 1, 2, 4 and 16 splits of a 32-step K loop: the reduce runs 1, 4 and 16
    phases per block (reduce_phases), and not at all for one split written in place."""
    N, C, H, W, Cout, k, s, p = WGRAD_LONG
    for regime in co.REGIMES:
        case = wgrad_case("long", regime, BF16)
        n.conv_trace_take()
        dw = n.conv_wgrad(case["dy"].to(cuda), case["x"].to(cuda), case["wshape"], s, p, fp32_out, target)
        trace = n.conv_trace_take()
        expect(trace, "wgrad", splits=splits)
        if splits == 1 and fp32_out:
            expect(trace, "wgrad_reduce", count=0)
        else:
            expect(trace, "wgrad_reduce", PH=ph, splits=splits, kind=0 if fp32_out else 1)
        check_dw(dw, case, fp32_out, f"conv_wgrad target {target} {regime} {trace}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID)
@pytest.mark.parametrize("name", ["3x3-m147", "m300-1x1"])
def test_wgrad_deferred_reduce(n, cuda, name, dtype):
    """conv_wgrad_deferred: the reduce taken into the tail of the conv's backward-data launch (carry
    blocks in the trace, pending.done set, both results still exact), and flushed on its own."""
    N, C, H, W, Cout, k, s, p = _shape(name)[0]
    for regime in INT_REGIMES:
        wc, dc = wgrad_case(name, regime, dtype), dgrad_case(name, regime, dtype)
        dy, x, w = wc["dy"].to(cuda), wc["x"].to(cuda), dc["w"].to(cuda)
        n.conv_trace_take()
        dw, pending = n.conv_wgrad_deferred(dy, x, wc["wshape"], s, p)
        assert pending is not None and not pending.done
        expect(n.conv_trace_take(), "wgrad_reduce", count=0)
        dx = n.conv_dgrad_flip(dc["dy"].to(cuda), w, p, pending)[0]
        trace = n.conv_trace_take()
        blocks = expect(trace, "carry_reduce", splits=pending.splits, kind=2 if dtype == F16 else 1)[0]["blocks"]
        assert int(blocks) > 0
        expect(trace, "fwd", carry=blocks)
        expect(trace, "wgrad_reduce", count=0)
        assert pending.done
        check_dw(dw, wc, False, f"deferred+carried {name} {regime} {DT_ID(dtype)}")
        co.assert_bits(dx, dc["dx"], f"dgrad carrying the reduce {name} {regime} {DT_ID(dtype)}")

        dw, pending = n.conv_wgrad_deferred(dy, x, wc["wshape"], s, p)
        n.conv_trace_take()
        n.conv_reduce_flush(pending)
        expect(n.conv_trace_take(), "wgrad_reduce", splits=pending.splits)
        assert pending.done
        check_dw(dw, wc, False, f"deferred+flushed {name} {regime} {DT_ID(dtype)}")


def test_wgrad_variant_20(n, cuda):
    """conv_set_variant(20): the 8-wave 256 x 256 backward-weight tile; the forward stays on the
    production tile."""
    N, C, H, W, Cout, k, s, p = WGRAD_V20
    n.conv_set_variant(20)
    for regime in co.REGIMES:
        case = wgrad_case("v20", regime, BF16)
        for fp32_out in (True, False):
            n.conv_trace_take()
            dw = n.conv_wgrad(case["dy"].to(cuda), case["x"].to(cuda), case["wshape"], s, p, fp32_out)
            expect(n.conv_trace_take(), "wgrad", BMW=256, BNW=256, STAGES=2, NT=512)
            check_dw(dw, case, fp32_out, f"variant 20 {regime} fp32={fp32_out}")
    expect(run_fwd(n, cuda, "m300-1x1", "sharp", BF16, True), "fwd", BM=128, STAGES=1, NT=256)
