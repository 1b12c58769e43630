"""Exact-integer oracle for the 16-bit implicit-GEMM convolutions (csrc/kernels/conv_kernels.hip).
A helper, not a test: plain torch on the CPU, nothing imported from the extension.

Why the result is predictable to the bit.  Let every operand element be an integer multiple of a
common quantum (1 here).  A 16-bit x 16-bit product is then an exact integer in fp32, and an fp32
sum of integers is exact as long as every partial sum stays below 2^24 in magnitude - whatever the
order.  With ``K * max|a| * max|b| < 2^24`` that holds for every subset and every sign pattern, so
the accumulated value IS the exact integer for the MFMA's internal order, 1- and 2-stage K loops,
the halo loop, B in registers, 256-row and 8-wave tiles, split-K and stream-K partial tiles and
the backward-weight split-K with its reduce.  What is stored is the one round-to-nearest-even of
that integer to bf16 (8 significant bits: integers up to 256 exact, ties at odd integers in
(256, 512), ...) or fp16 (11 bits: up to 2048).  One fp64 reference therefore predicts every
output bit of every path; no tolerance exists.

Statistics.  The forward epilogue sums y and y^2 of the ROUNDED outputs per 128-row tile (16-row
slab after split-K) in fp32; these are sums of integers too, exact while ``sum round(ref)^2``
over a partial's rows is below 2^24 (which also bounds the plain sum).  In the rounded regime the
sums of the rounded and of the unrounded values differ, which pins "statistics from the rounded
values".  fp16 cannot meet the condition on the SQUARES in the rounded regime: an
fp16-unrepresentable integer has more than 11 significant bits, its square more than 22, and a
128-row column with the required share of them passes 2^24.  Its plain sum stays far below 2^24
(``sum |round(ref)|`` per partial, asserted), so there fp16 is checked on y and psum and only psq is
left out (``psum_exact`` / ``psq_exact`` of a case say which).

Regimes (every generator asserts its conditions on the fp64 reference, so no test passes
vacuously):

  sharp    small integers x in +-{1,2,3}, w in +-{1,2} (fp16: +-{1..7}), thinned to the density
           that gives the output a standard deviation ``sigma`` over the terms an output really
           sums; max|ref| <= 256 (bf16) / 2048 (fp16): every output representable; per-partial
           sum ref^2 < 2^24.
  rounded  larger sigma (larger integer ranges where K is small): >= 1 % of the outputs not
           representable, >= 16 exact ties, K max|x| max|w| < 2^24, per-partial
           sum round(ref)^2 < 2^24 (bf16).
  one-hot  one operand holds isolated +-2^j (j in [-2, 2]) so that every output is AT MOST ONE
           product; the other holds random normal 16-bit patterns, all mantissa bits random,
           |v| in [2^-8, 2^8].  The conv is a scaled gather: each output is representable and
           names the element that must have been read.  y bits only.

Zeros compare equal whatever their sign (``assert_bits`` maps -0 to +0).

BN epilogues of the stride-1 backward-data (``conv_dgrad_bnstats``; kernel header "BNB / BNR /
BNR2 / RS2", binding comment), g = the 16-bit rounded conv output:

  plain  dx = g;  dz = g * [fma(x, a, b) > 0];  s1 = sum dz, s2 = sum dz (x - mean)
  BNR    dz = (g + res) * [y > 0] in fp32 (bn_mask: the same predicate, 1 bit per element, bit
         c % 8 of byte (row C + c) / 8);  dx = round16(dz);  s1, s2 from the fp32 dz BEFORE that
         second rounding - as bn_bwd_stats_kernel, the pass the epilogue replaces, sums the dz it
         stores (``from_stored=True`` computes the other reading, which the kernels do NOT follow)
  BNR2   s3 = sum dz (x2 - mean2) as well
  RS2    res is the compact [N, C, ceil(H/2), ceil(W/2)] tensor, read at even h and w, 0 elsewhere

With bn_x, bn_x2, bn_res small integers, means and b multiples of 1/4 and a in {+-1, +-1/2} the
mask, x - mean and every product are exact, and the sums are exact while
``4 sum|dz (x - mean)| < 2^24`` per partial.  In the sharp regime g + res is representable and the
two readings of BNR coincide; in the rounded regime g is a multiple of 2 or 4 above 256, g + res is
mostly not representable, and the sums of the fp32 and of the stored dz differ: that case tells
them apart.  The plain epilogue there pins "statistics from the ROUNDED g".  In the one-hot regimes
only dx is predictable (one fp32 add of two 16-bit values, then one rounding).
"""
import math

import torch
import torch.nn.functional as F

CL = torch.channels_last
BM = 128            # conv::BM: rows of a statistics partial
SPLIT_ROWS = 16     # kSplitRows: rows of a partial after split-K
LIMIT = 2.0 ** 24
EXACT_MAX = {torch.bfloat16: 256.0, torch.float16: 2048.0}


# ---- partial layouts (mirrors of conv_kernels.hip; tests/test_conv_oracle_cpu.py holds them to
# ---- hand-computed rows) ---------------------------------------------------------------------
def m_tiles(M):
    """conv_m_tiles: columns of an unsplit launch's partials, whatever the block rows are."""
    return (M + BM - 1) // BM


def split_cols(M):
    """conv_split_cols: columns when split-K ran (conv_split_epilogue_kernel's 16-row slabs)."""
    return (M + SPLIT_ROWS - 1) // SPLIT_ROWS


def s2_classes(H, W, R, S, pad):
    """Mirror of s2_classes: the non-empty parity classes (ph, pw, Ha, Wa, taps_r, taps_s) of a
    stride-2 backward-data in launch order; class (ph, pw) owns dx[:, :, ph::2, pw::2]."""
    out = []
    J = {}
    for par in (0, 1):
        r0 = (par + pad) % 2
        J[par] = ((R - 1 - r0) // 2 + 1 if r0 < R else 0, (S - 1 - r0) // 2 + 1 if r0 < S else 0)
    for ph in (0, 1):
        for pw in (0, 1):
            Ha, Wa = (H - ph + 1) // 2, (W - pw + 1) // 2
            if Ha <= 0 or Wa <= 0 or J[ph][0] == 0 or J[pw][1] == 0:
                continue
            out.append((ph, pw, Ha, Wa, J[ph][0], J[pw][1]))
    return out


def dgrad_s2_chunks(N, H, W, R, S, pad, split=None):
    """conv_dgrad_s2_chunks (split=None) / conv_dgrad_s2_plan().chunks: the classes' column ranges
    [(ph, pw, first column, columns, rows per column)], consecutive in one [C][chunks] array.
    ``split(M_class, K_class_taps)`` says whether that class runs split-K (16-row columns)."""
    cols, off = [], 0
    for ph, pw, Ha, Wa, jr, js in s2_classes(H, W, R, S, pad):
        M = N * Ha * Wa
        sp = bool(split(M, jr * js)) if split is not None else False
        n = split_cols(M) if sp else m_tiles(M)
        cols.append((ph, pw, off, n, SPLIT_ROWS if sp else BM))
        off += n
    return cols, off


def rows(t):
    """[N, C, H, W] -> the GEMM's row-major [M, C] matrix (channels_last order)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def partials(vals, rows_per_col, block_rows=None):
    """[M, C] per-element terms (fp64) -> [C][ceil(M / rows_per_col)] column sums.
    block_rows = 256 (BNB epilogue of a 256-row block): the block's whole sum lands in its first
    128-row column and zero in its second (when that column exists)."""
    M, C = vals.shape
    n = (M + rows_per_col - 1) // rows_per_col
    pad = n * rows_per_col - M
    v = torch.cat([vals, vals.new_zeros(pad, C)]) if pad else vals
    p = v.reshape(n, rows_per_col, C).sum(1).t().contiguous()
    if block_rows is not None and block_rows != rows_per_col:
        assert block_rows == 2 * rows_per_col
        q = torch.zeros_like(p)
        q[:, 0::2] = p[:, 0::2]
        q[:, 0:2 * (n // 2):2] += p[:, 1::2]
        p = q
    return p


def stat_partials(y16, rows_per_col=BM, want_sq=True):
    """(psum, psq) fp32 [C][cols] of a stored output [N, C, H, W], asserting they are exact
    (want_sq=False: psum alone, psq is None)."""
    v = rows(y16.double())
    assert partials(v.abs(), rows_per_col).max().item() < LIMIT, "per-partial sum of |y| reaches 2^24"
    ps = partials(v, rows_per_col).float()
    if not want_sq:
        return ps, None
    pq = partials(v * v, rows_per_col)
    assert pq.max().item() < LIMIT, "per-partial sum of squares reaches 2^24: the fp32 sums are not exact"
    return ps, pq.float()


# ---- fp64 references --------------------------------------------------------------------------
def ref_fwd(x, w, stride, pad, out_h=0, out_w=0):
    """y = conv2d(x, w); an explicit out_h / out_w keeps the first rows / columns: padding on the
    top and left only (the space-to-depth stem)."""
    y = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    return y[:, :, :out_h or None, :out_w or None]


def ref_dgrad(dy, w, pad):
    N, _, Ho, Wo = dy.shape
    R, S = w.shape[2:]
    shape = (N, w.shape[1], Ho + R - 1 - 2 * pad, Wo + S - 1 - 2 * pad)
    return torch.nn.grad.conv2d_input(shape, w.double(), dy.double(), stride=1, padding=pad)


def ref_dgrad_s2(dy, w, pad, H, W, compact=False):
    dx = torch.nn.grad.conv2d_input((dy.shape[0], w.shape[1], H, W), w.double(), dy.double(), stride=2, padding=pad)
    return dx[:, :, ::2, ::2] if compact else dx


def ref_wgrad(dy, x, wshape, stride, pad):
    """dw [Cout, C, R, S]; the output size is dy's: x is padded on the top / left by ``pad`` and on
    the bottom / right by exactly what dy's rows / columns read."""
    R, S = wshape[2:]
    H, W = x.shape[2:]
    Ho, Wo = dy.shape[2:]
    pb, pr = (Ho - 1) * stride + R - H - pad, (Wo - 1) * stride + S - W - pad
    xp = F.pad(x.double(), (pad, pr, pad, pb))
    return torch.nn.grad.conv2d_weight(xp, tuple(wshape), dy.double(), stride=stride, padding=0)


# ---- rounding, bit comparison ----------------------------------------------------------------
def round_to(ref, dtype):
    """One RNE rounding of an fp64 tensor (exact in fp32 first: asserted)."""
    f = ref.float()
    assert torch.equal(f.double(), ref), "reference not representable in fp32"
    return f if dtype == torch.float32 else f.to(dtype)


def _bits(t):
    t = t.detach().cpu().contiguous()
    t = torch.where(t == 0, torch.zeros_like(t), t)  # -0 -> +0
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_bits(out, expected, what, bn=128):
    """Bit equality (zeros of either sign equal).  On failure: the count, and the first mismatches
    decoded to (n, h, w, c) and to (m_tile, row, n_tile, col) of the 128 x bn tiling."""
    assert out.shape == expected.shape, f"{what}: shape {tuple(out.shape)} != {tuple(expected.shape)}"
    assert out.dtype == expected.dtype, f"{what}: dtype {out.dtype} != {expected.dtype}"
    bad = _bits(out) != _bits(expected)
    n_bad = int(bad.sum())
    if n_bad == 0:
        return
    lines = []
    o, e = out.detach().cpu(), expected.detach().cpu()
    for idx in bad.nonzero()[:8].tolist():
        if out.dim() == 4:
            n, c, h, w = idx
            m = (n * out.shape[2] + h) * out.shape[3] + w
            where = f"(n={n}, h={h}, w={w}, c={c}) = (m_tile={m // BM}, row={m % BM}, n_tile={c // bn}, col={c % bn})"
        else:
            where = "index " + str(tuple(idx))
        lines.append(f"  {where}: got {o[tuple(idx)].item()!r}, expected {e[tuple(idx)].item()!r}")
    raise AssertionError(f"{what}: {n_bad} of {bad.numel()} elements differ in bits\n" + "\n".join(lines))


# ---- operand generators ------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def sparse_ints(shape, amax, density, g):
    """Integers uniform in +-{1..amax}, each kept with probability ``density`` (else 0), fp64."""
    mag = torch.randint(1, amax + 1, shape, generator=g).double()
    sign = torch.randint(0, 2, shape, generator=g).double() * 2 - 1
    keep = (torch.rand(shape, generator=g) < density).double()
    return mag * sign * keep


def _e2(amax):
    return (amax + 1) * (2 * amax + 1) / 6.0  # mean square of uniform {1..amax}


def int_operands(shape_a, shape_b, K, sigma, amax_a, amax_b, seed):
    """Two integer operands whose K-term products sum to a standard deviation of about ``sigma``:
    sigma^2 = K d^2 E[a^2] E[b^2] with both operands thinned to the density d (capped at 1)."""
    g = _gen(seed)
    d = min(1.0, sigma / math.sqrt(K * _e2(amax_a) * _e2(amax_b)))
    return sparse_ints(shape_a, amax_a, d, g), sparse_ints(shape_b, amax_b, d, g)


def amplitudes(regime, K, dtype):
    """(sigma, amax_a, amax_b) of the integer regimes.  sharp: +-{1,2,3} x +-{1,2}, sigma 40 (fp16,
    exact up to 2048: weights +-{1..7}, sigma 150).  rounded: sigma near the first inexact binade
    (bf16 200 against 256, fp16 1800 against 2048), with larger integers where K terms of 3 x 2
    cannot reach it."""
    if regime == "sharp":
        return (40.0 if dtype == torch.bfloat16 else 150.0), 3, (2 if dtype == torch.bfloat16 else 7)
    sigma = 200.0 if dtype == torch.bfloat16 else 1800.0
    a, b = 3, 2
    while K * _e2(a) * _e2(b) < 4 * sigma * sigma:  # keep the density at or under 1/2
        a, b = 2 * a + 1, 2 * b + 1
    return sigma, a, b


def check_regime(ref, regime, dtype, K, amax_a, amax_b, stat_rows=(BM, SPLIT_ROWS), want_stats=True):
    """Assert the regime's conditions on the fp64 reference [N, C, H, W]; returns (psum_exact,
    psq_exact): whether the sums of the stored values and of their squares are exact in fp32 (psq:
    False only for fp16 / rounded)."""
    assert K * amax_a * amax_b < LIMIT, "K max|a| max|b| reaches 2^24"
    assert torch.equal(ref, ref.round()), "reference is not integer valued"
    lim = EXACT_MAX[dtype] if dtype in EXACT_MAX else LIMIT
    stored = ref.float().to(dtype).double() if dtype in EXACT_MAX else ref
    inexact = stored != ref
    assert ref.abs().max().item() > 0, "all-zero reference"
    if regime == "sharp":
        assert ref.abs().max().item() <= lim, f"sharp: max|ref| {ref.abs().max().item()} > {lim}"
        assert not inexact.any()
    else:
        share = inexact.double().mean().item()
        assert share >= 0.01, f"rounded: only {share:.4f} of the outputs are not representable"
        # a tie: the reference is exactly half way between the stored value and its neighbour in
        # the output type on the reference's side (the bit pattern one step up / down in magnitude)
        s16 = ref.float().to(dtype)
        step = torch.where(ref.abs() > stored.abs(), 1, -1).to(torch.int16)
        nb = (s16.contiguous().view(torch.int16) + step).view(dtype).double()
        ties = inexact & ((ref - stored).abs() == (nb - ref).abs())
        assert int(ties.sum()) >= 16, f"rounded: {int(ties.sum())} exact ties"
    if not want_stats:
        return False, False
    assert all(partials(rows(stored.abs()), r).max().item() < LIMIT for r in stat_rows), \
        "per-partial sum of |round(ref)| reaches 2^24"
    sq = rows(stored * stored)
    exact = all(partials(sq, r).max().item() < LIMIT for r in stat_rows)
    if not (regime == "rounded" and dtype == torch.float16):
        assert exact, "per-partial sum of squares reaches 2^24"
    return True, exact


def random_patterns(shape, dtype, seed):
    """Random normal 16-bit patterns: sign and every mantissa bit random, |v| in [2^-8, 2^8)."""
    g = _gen(seed)
    mbits = 7 if dtype == torch.bfloat16 else 10
    bias = 127 if dtype == torch.bfloat16 else 15
    sign = torch.randint(0, 2, shape, generator=g)
    exp = torch.randint(-8, 8, shape, generator=g) + bias
    man = torch.randint(0, 1 << mbits, shape, generator=g)
    u = (sign << 15) | (exp << mbits) | man
    u = torch.where(u >= 1 << 15, u - (1 << 16), u).to(torch.int16)
    v = u.view(dtype)
    a = v.double().abs()
    assert a.min().item() >= 2.0 ** -8 and a.max().item() < 2.0 ** 8
    return v.double()


def pow2_lattice(shape, step_h, step_w, seed):
    """[N, C, H, W] holding +-2^j, j in [-2, 2], at one random channel of every pixel of the lattice
    (h % step_h == oh, w % step_w == ow): no step_h x step_w window sees two of them."""
    g = _gen(seed)
    N, C, H, W = shape
    t = torch.zeros(shape, dtype=torch.float64)
    oh = int(torch.randint(0, min(step_h, H), (1,), generator=g))
    ow = int(torch.randint(0, min(step_w, W), (1,), generator=g))
    hs, ws = torch.arange(oh, H, step_h), torch.arange(ow, W, step_w)
    n, h, w = torch.meshgrid(torch.arange(N), hs, ws, indexing="ij")
    c = torch.randint(0, C, n.shape, generator=g)
    j = torch.randint(-2, 3, n.shape, generator=g).double()
    sg = torch.randint(0, 2, n.shape, generator=g).double() * 2 - 1
    t[n, c, h, w] = sg * torch.pow(torch.tensor(2.0, dtype=torch.float64), j)
    return t


def pow2_per_row(shape, seed):
    """[A, B, R, S] holding exactly one +-2^j per index of dim 0 (a weight: one tap of one input
    channel per output channel; for backward-weight dy permuted: one pixel per output channel)."""
    g = _gen(seed)
    A = shape[0]
    t = torch.zeros(shape, dtype=torch.float64)
    idx = [torch.randint(0, s, (A,), generator=g) for s in shape[1:]]
    j = torch.randint(-2, 3, (A,), generator=g).double()
    sg = torch.randint(0, 2, (A,), generator=g).double() * 2 - 1
    t[torch.arange(A), idx[0], idx[1], idx[2]] = sg * torch.pow(torch.tensor(2.0, dtype=torch.float64), j)
    return t


def check_one_hot(count, ref, dtype):
    """count: the reference of the operands' non-zero indicators = products per output."""
    assert count.max().item() <= 1, "one-hot: an output sums more than one product"
    assert (count == 1).double().mean().item() >= 0.02, "one-hot: almost no output reads anything"
    if dtype in EXACT_MAX:
        assert torch.equal(ref.float().to(dtype).double(), ref), "one-hot: an output is not representable"


def to16(t, dtype):
    """fp64 operand -> the 16-bit channels_last tensor the bindings take (exact: asserted)."""
    o = t.float().to(dtype)
    assert torch.equal(o.double(), t), "operand not representable in the 16-bit type"
    return o.contiguous(memory_format=CL)


# ---- cases: operands and expected outputs of one (pass, shape, regime, dtype) -----------------------
def out_hw(H, W, k, stride, pad, out_h=0, out_w=0):
    return out_h or (H + 2 * pad - k) // stride + 1, out_w or (W + 2 * pad - k) // stride + 1


def _pair(kind, sa, sb, K, regime, dtype, seed, ref_fn, step=None):
    """Operands (a, b) of shapes sa / sb for reference ref_fn(a, b), checked for the regime.
    one-hot-a / one-hot-b: which operand holds the isolated powers of two."""
    if regime in ("sharp", "rounded"):
        # the terms an output really sums (padding takes taps away: H = W = 1 keeps 1 of 9)
        keff = max(1.0, ref_fn(torch.ones(sa, dtype=torch.float64), torch.ones(sb, dtype=torch.float64)).mean().item())
        sigma, ma, mb = amplitudes(regime, keff, dtype)
        a, b = int_operands(sa, sb, keff, sigma, ma, mb, seed)
        ref = ref_fn(a, b)
        return a, b, ref, (ma, mb)
    if regime == "one-hot-b":
        a, b = random_patterns(sa, dtype, seed), pow2_per_row(sb, seed + 1)
    else:
        a, b = pow2_lattice(sa, step[0], step[1], seed + 1), random_patterns(sb, dtype, seed)
    ref = ref_fn(a, b)
    check_one_hot(ref_fn((a != 0).double(), (b != 0).double()), ref, dtype)
    return a, b, ref, None


def fwd_case(shape, regime, dtype, seed=0, out_h=0, out_w=0):
    """Forward: x, w (16-bit, channels_last), ref (fp64), y (expected bits), psum_exact, psq_exact."""
    N, C, H, W, Cout, k, s, p = shape
    K = C * k * k
    fn = lambda a, b: ref_fwd(a, b, s, p, out_h, out_w)  # noqa: E731
    x, w, ref, am = _pair("fwd", (N, C, H, W), (Cout, C, k, k), K, regime, dtype, seed, fn, step=(k, k))
    exact = check_regime(ref, regime, dtype, K, *am) if am else (False, False)
    return dict(x=to16(x, dtype), w=to16(w, dtype), ref=ref, y=round_to(ref, dtype).contiguous(memory_format=CL),
                psum_exact=exact[0], psq_exact=exact[1])


def dgrad_case(shape, regime, dtype, seed=0):
    """Backward-data of the conv ``shape`` (stride 1 or 2): dy, w, ref dx (full), dx bits."""
    N, C, H, W, Cout, k, s, p = shape
    Ho, Wo = out_hw(H, W, k, s, p)
    taps = k * k if s == 1 else ((k + 1) // 2) ** 2
    K = Cout * taps
    if s == 1:
        assert (Ho + k - 1 - 2 * p, Wo + k - 1 - 2 * p) == (H, W)
        fn = lambda a, b: ref_dgrad(a, b, p)  # noqa: E731
    else:
        fn = lambda a, b: ref_dgrad_s2(a, b, p, H, W)  # noqa: E731
    if regime == "one-hot-b":  # one tap of one output channel per INPUT channel (the GEMM's N)
        dy = random_patterns((N, Cout, Ho, Wo), dtype, seed)
        w = pow2_per_row((C, Cout, k, k), seed + 1).transpose(0, 1).contiguous()
        ref = fn(dy, w)
        check_one_hot(fn((dy != 0).double(), (w != 0).double()), ref, dtype)
        am = None
    else:
        dy, w, ref, am = _pair("dgrad", (N, Cout, Ho, Wo), (Cout, C, k, k), K, regime, dtype, seed, fn,
                               step=((k + s - 1) // s, (k + s - 1) // s))
    exact = check_regime(ref, regime, dtype, K, *am) if am else (False, False)
    return dict(dy=to16(dy, dtype), w=to16(w, dtype), ref=ref, dx=round_to(ref, dtype).contiguous(memory_format=CL),
                psum_exact=exact[0], psq_exact=exact[1])


def wgrad_case(shape, regime, dtype, seed=0, out_h=0, out_w=0):
    """Backward-weight: dy, x, ref dw (fp64), dw16 / dw32 expected bits.  K = N Ho Wo.  The integer
    regimes bound the reference by the 16-bit output type, so one case serves both output kinds."""
    N, C, H, W, Cout, k, s, p = shape
    Ho, Wo = out_hw(H, W, k, s, p, out_h, out_w)
    K = N * Ho * Wo
    wshape = (Cout, C, k, k)
    fn = lambda a, b: ref_wgrad(a, b, wshape, s, p)  # noqa: E731
    if regime == "one-hot-a":  # one non-zero pixel of dy per output channel
        dy = pow2_per_row((Cout, N, Ho, Wo), seed + 1).transpose(0, 1).contiguous()
        x = random_patterns((N, C, H, W), dtype, seed)
        ref = fn(dy, x)
        check_one_hot(fn((dy != 0).double(), (x != 0).double()), ref, dtype)
        am = None
    elif regime == "one-hot-b":  # one non-zero pixel of x per input channel
        dy = random_patterns((N, Cout, Ho, Wo), dtype, seed)
        x = pow2_per_row((C, N, H, W), seed + 1).transpose(0, 1).contiguous()
        ref = fn(dy, x)
        check_one_hot(fn((dy != 0).double(), (x != 0).double()), ref, dtype)
        am = None
    else:
        dy, x, ref, am = _pair("wgrad", (N, Cout, Ho, Wo), (N, C, H, W), K, regime, dtype, seed, fn)
    if am:
        check_regime(ref, regime, dtype, K, *am, want_stats=False)
    return dict(dy=to16(dy, dtype), x=to16(x, dtype), ref=ref, wshape=list(wshape),
                dw16=round_to(ref, dtype).contiguous(memory_format=CL),
                dw32=round_to(ref, torch.float32).contiguous(memory_format=CL))


# ---- BN epilogues of the stride-1 backward-data ---------------------------------------------------------
def bn_epilogue_inputs(shape_x, dtype, seed, res=False, x2=False, res_s2=False):
    """Inputs that keep the BNB / BNR / BNR2 / RS2 epilogues exact (module docstring)."""
    g = _gen(seed)
    N, C, H, W = shape_x
    d = {}
    d["bn_x"] = to16(torch.randint(-3, 4, shape_x, generator=g).double(), dtype)
    d["bn_mean"] = (torch.randint(-8, 9, (C,), generator=g).double() / 4).float()
    a = torch.tensor([1.0, -1.0, 0.5, -0.5])[torch.randint(0, 4, (C,), generator=g)]
    b = torch.randint(-8, 9, (C,), generator=g).float() / 4
    d["bn_coef"] = torch.cat([a, b])
    if res:
        rs = (N, C, (H + 1) // 2, (W + 1) // 2) if res_s2 else shape_x
        d["bn_res"] = to16(torch.randint(-3, 4, rs, generator=g).double(), dtype)
        y = torch.randint(-2, 3, shape_x, generator=g).double()  # zeros and both signs
        d["bn_y"] = to16(y, dtype)
        pos = rows(y > 0).reshape(-1, C // 8, 8).to(torch.int32)
        d["bn_mask"] = (pos << torch.arange(8, dtype=torch.int32)).sum(-1).to(torch.uint8)
    if x2:
        d["bn_x2"] = to16(torch.randint(-3, 4, shape_x, generator=g).double(), dtype)
        d["bn_mean2"] = (torch.randint(-8, 9, (C,), generator=g).double() / 4).float()
    return d


def dgrad_bn_expected(g16, bn, dtype, rows_per_col=BM, block_rows=None, res_s2=False, stats=True,
                      from_stored=False):
    """What conv_dgrad_bnstats returns for the rounded conv output g16 [N, C, H, W] and the inputs
    ``bn``: (dx bits, p1, p2, p3 or None), the partials fp32 [C][cols] (stats=False: dx alone, for
    operands whose sums are not exact).  from_stored=True: the partials summed from the stored
    16-bit dz instead - NOT what the kernels do; tests use it to show a case tells the two apart."""
    gd = g16.double()
    x = bn["bn_x"].double()
    C = x.shape[1]
    cv = lambda t: t.double().view(1, C, 1, 1)  # noqa: E731
    if "bn_y" in bn:
        r = bn["bn_res"].double()
        if res_s2:
            full = torch.zeros_like(gd)
            full[:, :, ::2, ::2] = r
            r = full
        dz32 = torch.where(bn["bn_y"].double() > 0, gd + r, torch.zeros_like(gd)).float()  # one fp32 add
        dx = dz32.to(dtype)
        dz = dx.double() if from_stored else dz32.double()
    else:
        a, b = bn["bn_coef"][:C], bn["bn_coef"][C:]
        dz = torch.where(x * cv(a) + cv(b) > 0, gd, torch.zeros_like(gd))
        dx = g16
    if not stats:
        return dx.contiguous(memory_format=CL), None, None, None
    t2 = dz * (x - cv(bn["bn_mean"]))
    terms = [dz, t2]
    if "bn_x2" in bn:
        terms.append(dz * (bn["bn_x2"].double() - cv(bn["bn_mean2"])))
    out = []
    for t in terms:
        assert 4 * partials(rows(t.abs()), rows_per_col, block_rows).max().item() < LIMIT
        out.append(partials(rows(t), rows_per_col, block_rows).float())
    return dx.contiguous(memory_format=CL), out[0], out[1], (out[2] if len(out) > 2 else None)


# ---- a CPU model of the kernel's arithmetic, with the mutations the oracle must catch -----------------
MUTATIONS = ("drop", "double", "pad_row", "tap_shift", "clear_lsb", "truncate", "stats_unrounded", "partial_shift")


def _truncate(f, dtype):
    """Round toward zero: RNE, then one step back in magnitude where that went past the value."""
    y = f.to(dtype).contiguous()
    over = (y.float().abs() > f.abs()).to(torch.int16)
    return (y.view(torch.int16) - over).view(dtype)


def model_fwd(x, w, stride, pad, dtype, order_seed=0, mutation=None):
    """conv_fwd as the kernels compute it: 16-bit operands, every product and partial sum in fp32,
    the K terms added one after the other in a shuffled order, one rounding, statistics of the
    rounded values per 128-row tile.  Returns (y [N, Cout, Ho, Wo], psum, psq)."""
    assert mutation is None or mutation in MUTATIONS
    N, C, H, W = x.shape
    Cout, _, R, S = w.shape
    Ho, Wo = out_hw(H, W, R, stride, pad)
    xf, wf = x.float(), w.float()
    g = _gen(1000 + order_seed)
    if mutation == "clear_lsb":
        # one element with its lowest mantissa bit set that some output multiplies by a non-zero, in
        # the denser operand (one-hot: the random patterns)
        ones = torch.ones(N, Cout, Ho, Wo, dtype=torch.float64)
        in_x = (xf != 0).double().mean() >= (wf != 0).double().mean()
        if in_x:
            used = torch.nn.grad.conv2d_input(x.shape, (wf != 0).double(), ones, stride=stride, padding=pad) > 0
        else:
            used = torch.nn.grad.conv2d_weight((xf != 0).double(), w.shape, ones, stride=stride, padding=pad) > 0
        bits = (x if in_x else w).contiguous().view(torch.int16).clone()
        i = tuple((((bits & 1) == 1) & used).nonzero()[0].tolist())
        bits[i] = bits[i] & -2
        if in_x:
            xf = bits.view(dtype).float()
        else:
            wf = bits.view(dtype).float()
    xp = F.pad(xf, (pad, pad, pad, pad))
    if mutation == "pad_row" and pad > 0:
        xp[:, :, pad - 1, :] = xp[:, :, pad, :]  # the last padding row above the image holds data
        xp[:, :, pad - 1, pad:pad + W] += (xp[:, :, pad - 1, pad:pad + W] == 0).float()
    if mutation == "tap_shift":
        wf = torch.roll(wf, 1, dims=3) if S > 1 else torch.roll(wf, 1, dims=1)  # 1x1: the next channel
    A = F.unfold(xp, (R, S), stride=stride).transpose(1, 2).reshape(N * Ho * Wo, C * R * S)  # [M, K]
    B = wf.reshape(Cout, C * R * S)
    M, K = A.shape
    acc = torch.zeros(M, Cout, dtype=torch.float32)
    hit = None
    if mutation in ("drop", "double"):
        nz = ((A != 0).float() @ (B != 0).float().t())
        m_, c_ = (nz > 0).nonzero()[0].tolist()
        k_ = int(((A[m_] != 0) & (B[c_] != 0)).nonzero()[0])
        hit = (m_, c_, k_)
    for k in torch.randperm(K, generator=g).tolist():
        term = A[:, k:k + 1] * B[None, :, k].expand(M, Cout)
        if hit is not None and k == hit[2]:
            term = term.clone()
            term[hit[0], hit[1]] *= 0.0 if mutation == "drop" else 2.0
        acc += term
    y = _truncate(acc, dtype) if mutation == "truncate" else acc.to(dtype)
    src = acc.double() if mutation == "stats_unrounded" else y.double()
    ps, pq = partials(src, BM).float(), partials(src * src, BM).float()
    if mutation == "partial_shift":
        ps = ps.clone()
        j = int(ps[0].ne(0).nonzero()[0]) if ps.shape[1] == 1 else 0
        if ps.shape[1] == 1:
            ps[0, j] = 0.0  # a single column: the partial went somewhere else
        else:
            ps[0, 1] = ps[0, 0]
            ps[0, 0] = 0.0
    y4 = y.reshape(N, Ho, Wo, Cout).permute(0, 3, 1, 2)
    return y4, ps, pq


# ---- the shapes of tests/test_conv_exact_gpu.py (tests/test_conv_oracle_cpu.py checks the generators on each) ------
# (N, C, H, W, Cout, k, stride, pad)
FWD_SHAPES = {
    "m25-1x1": (1, 64, 5, 5, 64, 1, 1, 0),             # below one wave's 32-row sub-tile
    "m128-1x1": (2, 128, 8, 8, 128, 1, 1, 0),          # exactly one tile
    "m129-1x1": (1, 64, 3, 43, 192, 1, 1, 0),          # one row into the second tile; Cout = 3 x 64
    "m147-1x1": (3, 192, 7, 7, 256, 1, 1, 0),          # a tile straddles two images; 3 K-steps
    "m300-1x1": (3, 128, 10, 10, 256, 1, 1, 0),        # three 128-row tiles: half-empty 256-row block
    "1x1s2-odd": (2, 64, 9, 7, 128, 1, 2, 0),
    "3x3-h1": (24, 64, 1, 1, 64, 3, 1, 1),              # every tap but the centre in the padding
    "3x3-h2": (6, 64, 2, 2, 64, 3, 1, 1),
    "3x3-5x6": (1, 192, 5, 6, 64, 3, 1, 1),
    "3x3-m147": (3, 64, 7, 7, 128, 3, 1, 1),
    "3x3-m300": (3, 128, 10, 10, 192, 3, 1, 1),
    "3x3-p0": (2, 64, 9, 8, 64, 3, 1, 0),
    "3x3s2": (2, 64, 11, 12, 128, 3, 2, 1),            # odd x even
    "5x5": (1, 64, 9, 9, 64, 5, 1, 2),
    "7x7s2": (1, 64, 13, 12, 64, 7, 2, 3),
}
# narrow inputs with the explicit output size of the space-to-depth stem: (shape, out_h, out_w)
NARROW_SHAPES = {
    "c16-4x4": ((2, 16, 12, 12, 64, 4, 1, 2), 12, 12),
    "c32-s2": ((2, 32, 9, 10, 64, 2, 1, 1), 9, 10),
}
DGRAD_SHAPES = {k: FWD_SHAPES[k] for k in ("m25-1x1", "m129-1x1", "m300-1x1", "3x3-h1", "3x3-5x6", "3x3-m147",
                                           "3x3-m300", "3x3-p0", "5x5")}
DGRAD_S2_SHAPES = {
    "1x1-odd": (3, 64, 9, 7, 64, 1, 2, 0),             # zero classes stop at the border
    "1x1-even": (2, 128, 8, 8, 64, 1, 2, 0),
    "3x3-oddeven": (2, 64, 11, 12, 128, 3, 2, 1),
    "3x3-even": (2, 128, 8, 8, 128, 3, 2, 1),
    "7x7": (2, 64, 12, 13, 64, 7, 2, 3),
}
WGRAD_SHAPES = {k: FWD_SHAPES[k] for k in ("m25-1x1", "m147-1x1", "m300-1x1", "1x1s2-odd", "3x3-h2", "3x3-5x6",
                                           "3x3-m147", "3x3-m300", "3x3s2", "7x7s2")}
REGIMES = ("sharp", "rounded", "one-hot-a", "one-hot-b")
