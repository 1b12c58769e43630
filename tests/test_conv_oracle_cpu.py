"""The exact-integer conv oracle (tests/conv_oracle.py) checked without a GPU: the generators meet
their regime conditions at every shape tests/test_conv_exact_gpu.py uses, the partial-layout
mirrors agree with hand-computed rows, and the oracle catches each kernel fault it claims to - a
CPU model of the kernel's arithmetic (fp32 accumulation in a shuffled order, one rounding) with one
fault injected must fail ``assert_bits`` in the regime named for that fault, and pass unmutated in
every summation order tried."""
import pytest
import torch

import conv_oracle as co
import test_conv_exact_gpu as gpu

BF16, F16 = torch.bfloat16, torch.float16


# ---- generators at the GPU file's shapes ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("regime", co.REGIMES)
def test_forward_generators_meet_their_conditions(regime, dtype):
    for name in list(co.FWD_SHAPES) + list(co.NARROW_SHAPES):
        c = gpu.fwd_case(name, regime, dtype)  # asserts inside; the cache is the GPU tests' own
        assert c["y"].dtype == dtype and c["y"].is_contiguous(memory_format=co.CL)
        assert c["x"].is_contiguous(memory_format=co.CL) and c["w"].is_contiguous(memory_format=co.CL)
        if regime in ("sharp", "rounded"):
            assert c["psum_exact"] and c["psq_exact"] == (not (regime == "rounded" and dtype == F16)), name
        if regime == "sharp":
            assert torch.equal(c["y"].double(), c["ref"])
        if regime == "rounded":
            assert (c["y"].double() != c["ref"]).double().mean() >= 0.01


@pytest.mark.parametrize("regime", co.REGIMES)
def test_knob_shape_generators(regime):
    for name in gpu.EXTRA_FWD:
        if name == "3x3s2-m32768" and regime != "sharp":
            continue  # (the GPU test runs the large shape in the sharp regime only)
        gpu.fwd_case(name, regime, BF16)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("regime", co.REGIMES)
def test_backward_generators_meet_their_conditions(regime, dtype):
    for name in list(co.DGRAD_SHAPES) + list(co.DGRAD_S2_SHAPES) + ["1x1-c256"]:
        c = gpu.dgrad_case(name, regime, dtype)
        N, C, H, W = gpu._shape(name)[0][:4]
        assert tuple(c["dx"].shape) == (N, C, H, W)
    for name in list(co.WGRAD_SHAPES) + list(co.NARROW_SHAPES) + ["long", "v20"]:
        if name in ("long", "v20") and dtype == F16:
            continue
        c = gpu.wgrad_case(name, regime, dtype)
        assert c["dw32"].dtype == torch.float32 and c["dw16"].dtype == dtype
        assert torch.equal(c["dw32"].double(), c["ref"])


def test_one_hot_is_a_gather():
    """Every one-hot output is zero or one pattern element times a power of two."""
    c = gpu.fwd_case("3x3-m147", "one-hot-b", BF16)
    nz = c["ref"][c["ref"] != 0]
    assert nz.numel() > 0.02 * c["ref"].numel()
    src = set(c["x"].double().abs().flatten().tolist())
    for v in nz[:200].abs().tolist():
        assert any(v * 2.0 ** j in src for j in range(-2, 3)), v


def test_generators_refuse_a_regime_they_cannot_meet():
    with pytest.raises(AssertionError):   # sigma of the rounded regime in a "sharp" check
        a, b = co.int_operands((2, 64, 8, 8), (64, 64, 1, 1), 64, 200.0, 15, 11, 0)
        co.check_regime(co.ref_fwd(a, b, 1, 0), "sharp", BF16, 64, 15, 11)
    with pytest.raises(AssertionError):   # and the other way round
        a, b = co.int_operands((2, 64, 8, 8), (64, 64, 1, 1), 64, 20.0, 3, 2, 0)
        co.check_regime(co.ref_fwd(a, b, 1, 0), "rounded", BF16, 64, 3, 2)
    with pytest.raises(AssertionError):   # two products in one output
        co.check_one_hot(torch.tensor([0.0, 2.0, 1.0]), torch.tensor([0.0, 1.0, 1.0]), BF16)


# ---- layout mirrors against hand-computed rows ------------------------------------------------------------------
def test_tile_and_slab_counts():
    assert [co.m_tiles(m) for m in (1, 25, 128, 129, 147, 256, 257, 300)] == [1, 1, 1, 2, 2, 2, 3, 3]
    assert [co.split_cols(m) for m in (1, 16, 17, 147, 300)] == [1, 1, 2, 10, 19]


def test_stride2_classes_by_hand():
    # 1x1, pad 0: only the even rows and columns receive gradient
    assert co.s2_classes(9, 7, 1, 1, 0) == [(0, 0, 5, 4, 1, 1)]
    # 3x3, pad 1 on 11 x 12: even positions see tap 1 only, odd positions taps 0 and 2
    assert co.s2_classes(11, 12, 3, 3, 1) == [(0, 0, 6, 6, 1, 1), (0, 1, 6, 6, 1, 2), (1, 0, 5, 6, 2, 1),
                                              (1, 1, 5, 6, 2, 2)]
    # 7x7, pad 3 on 12 x 13: even positions taps 1, 3, 5, odd positions 0, 2, 4, 6
    assert co.s2_classes(12, 13, 7, 7, 3) == [(0, 0, 6, 7, 3, 3), (0, 1, 6, 6, 3, 4), (1, 0, 6, 7, 4, 3),
                                              (1, 1, 6, 6, 4, 4)]
    # a one-row image has no odd row
    assert [c[:2] for c in co.s2_classes(1, 4, 3, 3, 1)] == [(0, 0), (0, 1)]
    # N = 2 on 11 x 12: 72, 72, 60, 60 rows -> one 128-row column each; N = 5: 180, 180, 150, 150 -> two each
    assert co.dgrad_s2_chunks(2, 11, 12, 3, 3, 1) == ([(0, 0, 0, 1, 128), (0, 1, 1, 1, 128), (1, 0, 2, 1, 128),
                                                       (1, 1, 3, 1, 128)], 4)
    assert co.dgrad_s2_chunks(5, 11, 12, 3, 3, 1)[1] == 8
    # the classes with more than one tap split: 72 rows -> 5 slabs, 60 rows -> 4
    cols, total = co.dgrad_s2_chunks(2, 11, 12, 3, 3, 1, split=lambda M, taps: taps > 1)
    assert cols == [(0, 0, 0, 1, 128), (0, 1, 1, 5, 16), (1, 0, 6, 4, 16), (1, 1, 10, 4, 16)] and total == 14


def test_partial_columns_by_hand():
    v = torch.arange(300, dtype=torch.float64).view(300, 1).repeat(1, 2)
    v[:, 1] = 1.0
    s = lambda a, b: float(sum(range(a, b)))  # noqa: E731
    assert co.partials(v, 128).tolist() == [[s(0, 128), s(128, 256), s(256, 300)], [128.0, 128.0, 44.0]]
    # a 256-row block: its whole sum in its first 128-row column, zero in its second
    assert co.partials(v, 128, block_rows=256).tolist() == [[s(0, 256), 0.0, s(256, 300)], [256.0, 0.0, 44.0]]
    assert co.partials(v[:130], 128, block_rows=256).tolist() == [[s(0, 130), 0.0], [130.0, 0.0]]
    assert co.partials(v[:40], 16).tolist() == [[s(0, 16), s(16, 32), s(32, 40)], [16.0, 16.0, 8.0]]
    y = torch.tensor([1.0, -2.0, 3.0]).view(3, 1, 1, 1).to(BF16)
    ps, pq = co.stat_partials(y)
    assert ps.tolist() == [[2.0]] and pq.tolist() == [[14.0]] and ps.dtype == torch.float32
    with pytest.raises(AssertionError):
        co.stat_partials(torch.full((128, 1, 1, 1), 400.0).to(BF16))  # 128 * 400^2 > 2^24


def test_bn_epilogue_semantics_by_hand():
    """One pixel, eight channels: masks, what is stored, and the three sums."""
    g16 = torch.tensor([5.0, 5.0, 5.0, -4.0, 7.0, 7.0, 1.0, 2.0]).view(1, 8, 1, 1).to(BF16)
    x = torch.tensor([1.0, -1.0, 2.0, 2.0, 0.0, 3.0, 1.0, 1.0]).view(1, 8, 1, 1).to(BF16)
    mean = torch.tensor([0.25, 0.25, -0.5, 0.0, 0.0, 1.0, 0.0, 0.0])
    a = torch.tensor([1.0, 1.0, -0.5, 1.0, 1.0, 1.0, 1.0, 1.0])
    b = torch.tensor([0.0, 0.0, 1.0, -2.0, 0.25, 0.0, 0.0, 0.0])
    bn = dict(bn_x=x, bn_mean=mean, bn_coef=torch.cat([a, b]))
    dx, p1, p2, p3 = co.dgrad_bn_expected(g16, bn, BF16)
    # masks: x a + b = 1, -1, 0, 0, 0.25, 3, 1, 1  ->  on, off, off (not > 0), off, on, on, on, on
    assert torch.equal(dx, g16) and p3 is None                       # plain: dx is the unmasked gradient
    assert p1.flatten().tolist() == [5.0, 0.0, 0.0, 0.0, 7.0, 7.0, 1.0, 2.0]
    assert p2.flatten().tolist() == [5 * 0.75, 0.0, 0.0, 0.0, 0.0, 14.0, 1.0, 2.0]
    y = torch.tensor([1.0, 0.0, -1.0, 2.0, 2.0, 0.0, 1.0, 1.0]).view(1, 8, 1, 1).to(BF16)
    res = torch.tensor([1.0, 1.0, 1.0, 1.0, -7.0, 1.0, 2.0, 3.0]).view(1, 8, 1, 1).to(BF16)
    x2 = torch.ones(1, 8, 1, 1).to(BF16)
    bn.update(bn_y=y, bn_res=res, bn_x2=x2, bn_mean2=torch.full((8,), 0.5))
    dx, p1, p2, p3 = co.dgrad_bn_expected(g16, bn, BF16)
    assert dx.flatten().tolist() == [6.0, 0.0, 0.0, -3.0, 0.0, 0.0, 3.0, 5.0]   # (g + res) * (y > 0), stored
    assert p1.flatten().tolist() == [6.0, 0.0, 0.0, -3.0, 0.0, 0.0, 3.0, 5.0]
    assert p2.flatten().tolist() == [4.5, 0.0, 0.0, -6.0, 0.0, 0.0, 3.0, 5.0]
    assert p3.flatten().tolist() == [3.0, 0.0, 0.0, -1.5, 0.0, 0.0, 1.5, 2.5]
    # g + res not representable: 258 + 1 = 259 is stored as 260 (tie to even), and summed as 259
    big = dict(bn, bn_res=torch.ones(1, 8, 1, 1).to(BF16), bn_y=torch.ones(1, 8, 1, 1).to(BF16))
    g258 = torch.full((1, 8, 1, 1), 258.0).to(BF16)
    dx, p1, _, _ = co.dgrad_bn_expected(g258, big, BF16)
    assert dx.flatten().tolist() == [260.0] * 8 and p1.flatten().tolist() == [259.0] * 8
    assert co.dgrad_bn_expected(g258, big, BF16, from_stored=True)[1].flatten().tolist() == [260.0] * 8
    assert co.dgrad_bn_expected(g258, big, BF16, stats=False)[1] is None
    # the 1-bit mask: bit c % 8 of byte (row C + c) / 8
    inp = co.bn_epilogue_inputs((1, 16, 2, 1), BF16, seed=0, res=True)
    pos = co.rows(inp["bn_y"].double() > 0)
    for r in range(2):
        for c in range(16):
            assert bool((int(inp["bn_mask"][r, c // 8]) >> (c % 8)) & 1) == bool(pos[r, c])
    # RS2: the compact residual lands on the even rows and columns
    g = torch.ones(1, 8, 3, 3).to(BF16)
    bn2 = dict(bn_x=torch.zeros(1, 8, 3, 3).to(BF16), bn_mean=torch.zeros(8), bn_coef=torch.zeros(16),
               bn_y=torch.ones(1, 8, 3, 3).to(BF16), bn_res=torch.full((1, 8, 2, 2), 2.0).to(BF16))
    dx = co.dgrad_bn_expected(g, bn2, BF16, res_s2=True)[0]
    assert dx[0, 0].tolist() == [[3.0, 1.0, 3.0], [1.0, 1.0, 1.0], [3.0, 1.0, 3.0]]


def test_references_by_hand():
    x = torch.arange(16.0).view(1, 1, 4, 4)
    w = torch.ones(1, 1, 2, 2)
    # explicit 2 x 2 output of a pad-1 conv: padding on the top and left only
    assert co.ref_fwd(x, w, 2, 1, 2, 2)[0, 0].tolist() == [[0.0, 3.0], [12.0, 30.0]]
    dy = torch.ones(1, 1, 2, 2)
    # backward-weight with dy's size: dw[r, s] = sum of the x pixels tap (r, s) read
    assert co.ref_wgrad(dy, x, (1, 1, 2, 2), 2, 1)[0, 0].tolist() == [[5.0, 4 + 6.0], [1 + 9.0, 0 + 2 + 8 + 10.0]]
    assert co.ref_dgrad_s2(dy, torch.ones(1, 1, 1, 1), 0, 3, 3, compact=True).shape == (1, 1, 2, 2)
    assert co.ref_dgrad_s2(dy, torch.ones(1, 1, 1, 1), 0, 3, 3)[0, 0].tolist() == [[1, 0, 1], [0, 0, 0], [1, 0, 1]]
    assert co.ref_dgrad(dy, torch.ones(1, 1, 3, 3), 1).shape == (1, 1, 2, 2)


def test_assert_bits_reports_and_ignores_zero_signs():
    a = torch.zeros(1, 2, 2, 2, dtype=BF16)
    b = -a
    co.assert_bits(a, b, "signed zeros")
    b = a.clone()
    b[0, 1, 1, 0] = 2 ** -100   # far below any tolerance, still a different number
    with pytest.raises(AssertionError, match=r"1 of 8 .*\n.*n=0, h=1, w=0, c=1.*m_tile=0, row=2, n_tile=0, col=1"):
        co.assert_bits(a, b, "tiny")
    with pytest.raises(AssertionError, match="dtype"):
        co.assert_bits(a, a.to(F16), "dtype")


# ---- the oracle catches what it claims to --------------------------------------------------------------------
MODEL_SHAPE = (2, 64, 9, 8, 64, 3, 1, 1)   # M = 144: two partial columns, borders on every side


@pytest.fixture(scope="module")
def model_cases():
    return {(r, d): co.fwd_case(MODEL_SHAPE, r, d, seed=5) for r in co.REGIMES for d in (BF16, F16)}


def _check(case, out, stats):
    y, ps, pq = out
    co.assert_bits(y.contiguous(memory_format=co.CL), case["y"], "y", bn=64)
    if stats and case["psum_exact"]:
        eps, epq = co.stat_partials(case["y"], want_sq=case["psq_exact"])
        co.assert_bits(ps, eps, "psum")
        if case["psq_exact"]:
            co.assert_bits(pq, epq, "psq")


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("regime", co.REGIMES)
def test_unmutated_model_passes_in_every_order(model_cases, regime, dtype):
    case = model_cases[regime, dtype]
    for order in range(3):
        out = co.model_fwd(case["x"], case["w"], 1, 1, dtype, order_seed=order)
        _check(case, out, True)


@pytest.mark.parametrize("mutation,regime", [
    ("drop", "sharp"), ("double", "sharp"),
    ("pad_row", "sharp"), ("pad_row", "one-hot-a"), ("pad_row", "one-hot-b"),
    ("tap_shift", "one-hot-a"), ("tap_shift", "one-hot-b"),
    ("clear_lsb", "one-hot-a"), ("clear_lsb", "one-hot-b"),
    ("truncate", "rounded"), ("stats_unrounded", "rounded"), ("partial_shift", "sharp"),
])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_mutation_is_caught_in_its_regime(model_cases, mutation, regime, dtype):
    case = model_cases[regime, dtype]
    out = co.model_fwd(case["x"], case["w"], 1, 1, dtype, order_seed=1, mutation=mutation)
    stats_only = mutation in ("stats_unrounded", "partial_shift")
    if stats_only:
        _check(case, out, False)     # y is untouched: only the statistics can tell
    with pytest.raises(AssertionError, match="differ in bits"):
        _check(case, out, stats_only)


def test_every_mutation_is_in_the_table():
    import inspect
    src = inspect.getsource(test_mutation_is_caught_in_its_regime)
    assert all(f'"{m}"' in src for m in co.MUTATIONS)


def test_single_dropped_product_is_inside_the_old_tolerance(model_cases):
    """Why the tolerance test could not see it: one product of a 576-term sum moves the output by at
    most 6, relative 1e-2 of nothing - on O(1) data the same fault is about 0.015, inside
    rtol = atol = 1e-2 of tests/test_conv_gpu.py; here it is a bit mismatch."""
    case = model_cases["sharp", BF16]
    good = co.model_fwd(case["x"], case["w"], 1, 1, BF16)[0]
    bad = co.model_fwd(case["x"], case["w"], 1, 1, BF16, mutation="drop")[0]
    assert int((good != bad).sum()) == 1 and (good.double() - bad.double()).abs().max().item() <= 6
