"""fp64 oracle, first-order rounding bounds and a CPU model of the fused BatchNorm kernels
(csrc/kernels/bn_kernels.hip, finalize helpers in csrc/kernels/carry.h).  A helper, not a test:
plain torch, CPU or GPU tensors, nothing imported from the extension.

Activations are row-major ``[M, C]`` matrices (``rows`` turns a channels_last 4-D tensor into one);
16-bit inputs are exact in fp64.  ``u = 2^-24`` is fp32's unit round-off.  Every bound below is a
worst case of the arithmetic the kernel states (every rounding at its limit, all of one sign);
second-order terms are left to the caller's ``FACTOR``.

Forward statistics (``bn_fwd_stats_kernel``): per chunk of ``rows_per_chunk`` rows a thread adds
its ``n_t = ceil(rows_per_chunk / rpi)`` rows in fp32, one after the other, then ``rpi`` threads'
sums are added in fp32 across LDS, then the chunks' fp32 partials are summed in fp64:

    |sum   - exact| <= (n_t + rpi)     u sum|x|       = E_s
    |sumsq - exact| <= (n_t + rpi + 1) u sum x^2      = E_q   (one more rounding per term)

Finalize (fp64 from the sums, one fp32 rounding per stored number; ``eps`` and ``momentum`` are
fp32 values):

    mean   = s/M                        E_mean = E_s/M                      (+ u|mean| stored)
    var    = max(q/M - mean^2, 0)       E_var  = E_q/M + 2|mean| E_mean + E_mean^2
    invstd = (var + eps)^-1/2           E_inv  = invstd(var - E_var) - invstd(var) + u invstd
                                        (exact, not first order: invstd is convex decreasing)
    a = fl(g * invstd32)                E_a    = |g| E_inv + u|a|
    b = fl(beta - fl(mean32 * a))       E_b    = E_mean32 |a| + |mean| E_a + u(|mean a| + |b|)
    run  = fl(fl(fl(1-m) r0) + fl(m v)) E_run  = m E_v32 + u(2|(1-m) r0| + |m v| + |run|)
                                        v = mean, or var M/(M-1) (each cast to fp32 first)

From partials handed in as fp32 numbers (the conv epilogues' path) E_s and E_q are the fp64
summation's own ``chunks * 2^-53 * sum|p|``: every output is then good to the few fp32 ulps the
formulas above leave (1 for mean and invstd, 2 for a, about 4 for b and the running statistics).

Forward apply (``bn_fwd_apply_kernel``): ``fmaf(x, a, b)`` is one rounding, ``+ r`` a second,
``+ fmaf(x2, a2, b2)`` a second and a third; ReLU is exact; then one rounding to the I/O type.
Each rounding is relative to its own result, so the fp32 value is within
``u(|x a + b| [+ |x2 a2 + b2|] [+ |sum|])`` of the fp64 value (never more than the
``3u (|x||a| + |b| + |r| ...)`` one would write without looking at the signs), and the stored
number lies between the I/O roundings of the two ends of that band - it IS the rounding of the
fp64 value unless a rounding boundary (or zero, under ReLU) falls inside the band, where either
neighbour is accepted.  For fp32 I/O the band is an absolute bound.  The share of elements with a
boundary inside the band is a property of the inputs alone; ``ties_allowed`` caps it.

Backward statistics (``bn_bwd_stats_kernel``): ``dz = (dy [+ dy2]) * mask`` is predictable to the
bit (fp32 add, then one rounding to a 16-bit I/O type).  ``s1 = sum dz`` and
``s2 = sum dz (x - mean)`` are summed like the forward sums:

    E_s1 = (n_t + rpi + two)     u sum|dz|                    (two: the fp32 add dy + dy2)
    E_s2 = (n_t + rpi + two + 2) u sum|dz||x - mean|          (x - mean, and the product)

Backward finalize (``bn_bwd_fin_store``), fp64 then one fp32 rounding each:

    dgamma = s2 invstd                  E = |invstd| E_s2 + u|dgamma|
    dbeta  = s1                         E = E_s1 + u|dbeta|
    k1 = g invstd,  k2 = -k1 invstd^2 s2/M,  k3 = -k1 s1/M
                                        E_k1 = u|k1|, E_k2 = |k1| invstd^2 E_s2/M + u|k2|,
                                        E_k3 = |k1| E_s1/M + u|k3|

Backward apply: ``dx = k1 dz + k2 (x - mean) + k3`` in fp32, possibly contracted: at most four
roundings touch any term, so

    E_dx = |dz| E_k1 + |x - mean| E_k2 + E_k3 + 4u(|k1 dz| + |k2 (x - mean)| + |k3|)

and the stored number lies between the I/O roundings of ``dx -+ E_dx`` (absolute for fp32 I/O).
"""
import math

import torch

U = 2.0 ** -24          # fp32 unit round-off
U64 = 2.0 ** -53
FACTOR = 1.25           # the GPU tests' allowance over the first-order bounds (second-order terms)
TIE_CAP = 1e-3          # largest share of elements that may sit on a rounding / ReLU boundary
TINY = 1e-37            # below fp32's normal range a relative bound says nothing (flush to zero)
DTYPES = (torch.bfloat16, torch.float16, torch.float32)

# ---- launch geometry -----------------------------------------------------------------------
# Mirror of bn_geometry() and the constants above it (csrc/kernels/bn_kernels.hip: kBnMaxChunks
# = 512, kBnApplyMax = 32768, kBnBwdApplyMax = 4 * kMaxBlocks = 8192, kBlock = 256 threads, and
# bwd_dispatch's grid of min(2 * apply_blocks, kBnBwdApplyMax) blocks).  No binding exposes the
# geometry; tests/test_bn_oracle_cpu.py holds this mirror to hand-computed rows.
K_BLOCK, K_MAX_CHUNKS, K_APPLY_MAX, K_BWD_APPLY_MAX = 256, 512, 32768, 8192
WIDTHS = (8, 16, 32, 64, 128, 256, 512, 1024, 2048)


def supported(C):
    return C >= 8 and C % 8 == 0 and C <= 8 * K_BLOCK and K_BLOCK % (C // 8) == 0


def geometry(M, C):
    rpi = K_BLOCK // (C // 8)
    rpc = max(-(-M // K_MAX_CHUNKS), 64)
    rpc = -(-rpc // rpi) * rpi
    chunks = max(-(-M // rpc), 1)
    apply_blocks = min(max(-(-M // (2 * rpi)), 1), K_APPLY_MAX)
    bwd_blocks = min(2 * apply_blocks, K_BWD_APPLY_MAX)
    return dict(rpi=rpi, rows_per_chunk=rpc, chunks=chunks, n_t=rpc // rpi, last_rows=M - (chunks - 1) * rpc,
                apply_blocks=apply_blocks, bwd_apply_blocks=bwd_blocks,
                fwd_apply_iters=-(-M // (2 * rpi * apply_blocks)), bwd_apply_iters=-(-M // (rpi * bwd_blocks)))


# ---- small helpers -------------------------------------------------------------------------
def rows(t):
    """channels_last [N, C, H, W] (or [M, C]) -> the [M, C] matrix the kernels see (a view)."""
    return t if t.dim() == 2 else t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def as_nchw(t2d):
    """[M, C] contiguous -> channels_last [M, C, 1, 1] view of the same memory."""
    m, c = t2d.shape
    return t2d.view(m, 1, 1, c).permute(0, 3, 1, 2)


def f32(v):
    """A python float / fp64 tensor rounded to fp32, as fp64."""
    if not torch.is_tensor(v):
        return float(torch.tensor(v, dtype=torch.float32))
    return v.float().double()


def round_io(v, dtype):
    """fp64 -> the I/O type (through fp32, as the kernels' conversions do) -> fp64."""
    return v.float().to(dtype).double()


def worst_ratio(got, want, bound):
    """max |got - want| / bound (NaNs must have been dealt with by the caller)."""
    err = ((got.double() - want).abs() - TINY).clamp(min=0)
    return (err / bound.clamp(min=1e-300)).max().item() if err.numel() else 0.0


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- forward ---------------------------------------------------------------------------------
def fwd_sums(x, geo):
    """Exact per-channel sum and sum of squares of x [M, C] and the kernel's summation bounds."""
    xd = x.double()
    s, q = xd.sum(0), (xd * xd).sum(0)
    k = geo["n_t"] + geo["rpi"]
    return s, q, k * U * xd.abs().sum(0), (k + 1) * U * q


def partial_sums(ps, pq):
    """fp32 partials [C, chunks] taken as exact inputs: fp64 sums and the fp64 summation's bound."""
    n = ps.shape[1]
    return (ps.double().sum(1), pq.double().sum(1), n * U64 * ps.double().abs().sum(1),
            n * U64 * pq.double().abs().sum(1))


def _running(r0, v, e_v32, mom):
    run = (1.0 - mom) * r0 + mom * v
    return run, mom * e_v32 + U * (2 * ((1.0 - mom) * r0).abs() + (mom * v).abs() + run.abs())


def fwd_finalize(s, q, e_s, e_q, M, gamma, beta, eps, momentum, run_mean, run_var):
    """-> (want, bound): dicts of fp64 per-channel tensors for mean, var, invstd, a, b,
    running_mean, running_var (the module docstring has the formulas)."""
    eps, mom = f32(eps), f32(momentum)
    g, bt, rm0, rv0 = gamma.double(), beta.double(), run_mean.double(), run_var.double()
    mean = s / M
    e_mean = e_s / M
    var = (q / M - mean * mean).clamp(min=0)
    e_var = e_q / M + 2 * mean.abs() * e_mean + e_mean * e_mean
    invstd = (var + eps).rsqrt()
    e_inv = ((var - e_var).clamp(min=0) + eps).rsqrt() - invstd + U * invstd
    e_mean32 = e_mean + U * mean.abs()
    a = g * invstd
    e_a = g.abs() * e_inv + U * a.abs()
    b = bt - mean * a
    e_b = e_mean32 * a.abs() + mean.abs() * e_a + U * ((mean * a).abs() + b.abs())
    unb = var * (M / (M - 1.0)) if M > 1 else var
    e_unb32 = (e_var * (M / (M - 1.0)) if M > 1 else e_var) + U * unb
    rm, e_rm = _running(rm0, mean, e_mean32, mom)
    rv, e_rv = _running(rv0, unb, e_unb32, mom)
    want = dict(mean=mean, var=var, invstd=invstd, a=a, b=b, running_mean=rm, running_var=rv)
    bound = dict(mean=e_mean32, var=e_var, invstd=e_inv, a=e_a, b=e_b, running_mean=e_rm, running_var=e_rv)
    return want, bound


def apply_value(x, a, b, res=None, a2=None, b2=None, relu=False):
    """fp64 value and fp32-arithmetic band of y = relu(x*a + b [+ r | + x2*a2 + b2]); a, b are the
    fp32 coefficients as the kernel reads them.  NaN propagates through the ReLU.  Each rounding is
    relative to its own result (u|x a + b| for the fma, u|sum| for an add), which is never more than
    the u(|x||a| + |b| + ...) per rounding of the module docstring and much less under no
    cancellation; the band is the sum over the roundings the variant has."""
    v = x.double() * a.double() + b.double()
    band = U * v.abs()
    if res is not None and a2 is not None:
        v2 = res.double() * a2.double() + b2.double()
        v = v + v2
        band = band + U * v2.abs() + U * v.abs()
    elif res is not None:
        v = v + res.double()
        band = band + U * v.abs()
    return v, band


def _relu(v):
    return torch.where(v < 0, torch.zeros_like(v), v)       # keeps NaN, like the kernel


def interval(v, band, dtype, relu=False, factor=1.0):
    """The I/O-type numbers the kernel may store for an fp32 value within factor*band of v: (lo, hi,
    exact), exact = the rounding of v itself.  For fp32 I/O lo/hi are v -+ factor*band."""
    lo, hi = v - factor * band, v + factor * band
    if relu:
        lo, hi, v = _relu(lo), _relu(hi), _relu(v)
    if dtype == torch.float32:
        return lo, hi, v
    return round_io(lo, dtype), round_io(hi, dtype), round_io(v, dtype)


def check_interval(got, v, band, dtype, relu=False, factor=1.0):
    """-> (violations, ties, elements): elements of ``got`` outside the accepted interval, and the
    elements whose interval holds more than one I/O number (none for fp32).  NaN matches NaN."""
    lo, hi, _ = interval(v, band, dtype, relu, factor)
    g = got.double()
    nan = torch.isnan(v)
    ok = ((g >= lo) & (g <= hi)) | (nan & torch.isnan(g))
    ties = int(((lo != hi) & ~nan).sum()) if dtype != torch.float32 else 0
    return int((~ok).sum()), ties, v.numel()


def ties_allowed(elements):
    """TIE_CAP of the elements, as a count.  The share is a property of the input distribution and a
    test sees a sample of it, so the count may exceed TIE_CAP * n by two standard deviations of a
    Poisson count of that mean, plus two elements (1e-3 of n is less than one element below a
    thousand).  A tie is still held to its two neighbours; it is not left out."""
    mean = TIE_CAP * elements
    return mean + 2.0 * math.sqrt(mean) + 2.0


# ---- backward --------------------------------------------------------------------------------
def dz_exact(dy, dy2, mask):
    """The masked gradient the statistics pass stores, to the bit (I/O type of dy)."""
    g = dy.float() if dy2 is None else dy.float() + dy2.float()
    if mask is not None:
        g = torch.where(mask, g, torch.zeros_like(g))
    return g.to(dy.dtype)


def mask_from_x(x, coef):
    """fmaf(x, a, b) > 0 decided in fp64 (a correctly rounded fma has the sign of the exact value
    wherever it does not underflow) -> (mask, share of elements too close to 0 to call)."""
    c = x.shape[1]
    v = x.double() * coef[:c].double() + coef[c:].double()
    return v > 0, ((v.abs() < TINY) & (v != 0)).double().mean().item()


def bwd_sums(dy, dy2, mask, x, mean, geo):
    """Exact s1, s2 (fp64, from the fp64 sum dy + dy2) and the kernel's summation bounds."""
    g = dy.double() if dy2 is None else dy.double() + dy2.double()
    if mask is not None:
        g = torch.where(mask, g, torch.zeros_like(g))
    xm = x.double() - mean.double()
    k = geo["n_t"] + geo["rpi"] + (0 if dy2 is None else 1)
    t = g * xm
    return g.sum(0), t.sum(0), k * U * g.abs().sum(0), (k + 2) * U * t.abs().sum(0)


def bwd_finalize(s1, s2, e_s1, e_s2, M, gamma, invstd):
    """-> (want, bound) for dgamma, dbeta, k1, k2, k3 from the fp32 invstd the kernel reads."""
    g, inv = gamma.double(), invstd.double()
    k1 = g * inv
    dgamma, k2, k3 = s2 * inv, -k1 * inv * inv * s2 / M, -k1 * s1 / M
    want = dict(dgamma=dgamma, dbeta=s1, k1=k1, k2=k2, k3=k3)
    bound = dict(dgamma=inv.abs() * e_s2 + U * dgamma.abs(), dbeta=e_s1 + U * s1.abs(), k1=U * k1.abs(),
                 k2=k1.abs() * inv * inv * e_s2 / M + U * k2.abs(), k3=k1.abs() * e_s1 / M + U * k3.abs())
    return want, bound


def dx_value(dz, x, mean, want, bound):
    """fp64 dx = k1 dz + k2 (x - mean) + k3 and its bound before the I/O rounding."""
    g, xm = dz.double(), x.double() - mean.double()
    t1, t2 = want["k1"] * g, want["k2"] * xm
    v = t1 + t2 + want["k3"]
    e = (g.abs() * bound["k1"] + xm.abs() * bound["k2"] + bound["k3"]
         + 4 * U * (t1.abs() + t2.abs() + want["k3"].abs()))
    return v, e


# ---- the kernels' summation order on the CPU (tests/test_bn_oracle_cpu.py) ---------------------
def model_chunk_sums(terms, geo):
    """fp32 [M, C] terms -> fp32 partials [C, chunks] summed as the statistics kernels do: each
    thread its rows one after the other, then the rpi threads of a channel one after the other."""
    m, c = terms.shape
    rpi, rpc, chunks = geo["rpi"], geo["rows_per_chunk"], geo["chunks"]
    pad = torch.zeros(chunks * rpc, c, dtype=torch.float32)       # adding +0 is exact
    pad[:m] = terms.float()
    t = pad.view(chunks, rpc // rpi, rpi, c)
    acc = torch.zeros(chunks, rpi, c, dtype=torch.float32)
    for j in range(rpc // rpi):
        acc = acc + t[:, j]
    out = torch.zeros(chunks, c, dtype=torch.float32)
    for j in range(rpi):
        out = out + acc[:, j]
    return out.t().contiguous()


def model_fwd(x, geo, gamma, beta, eps, momentum, run_mean, run_var):
    """Forward statistics and finalize with the kernels' rounding points -> dict of fp32 tensors."""
    m = x.shape[0]
    xf = x.float()
    ps, pq = model_chunk_sums(xf, geo), model_chunk_sums(xf * xf, geo)
    s, q = ps.double().sum(1), pq.double().sum(1)
    eps32, mom = f32(eps), torch.tensor(momentum, dtype=torch.float32)
    mean = s / m
    var = (q / m - mean * mean).clamp(min=0)
    invstd = (var + eps32).rsqrt().float()
    a = gamma.float() * invstd
    mean32 = mean.float()
    b = beta.float() - mean32 * a
    unb = (var * m / (m - 1) if m > 1 else var).float()
    rm = (1.0 - mom) * run_mean.float() + mom * mean32
    rv = (1.0 - mom) * run_var.float() + mom * unb
    return dict(mean=mean32, invstd=invstd, a=a, b=b, running_mean=rm, running_var=rv, var=var)


def _fma(x, a, b):
    return (x.double() * a.double() + b.double()).float()


def model_apply(x, a, b, res=None, a2=None, b2=None, relu=False):
    o = _fma(x, a, b)
    if res is not None and a2 is not None:
        o = o + _fma(res, a2, b2)
    elif res is not None:
        o = o + res.float()
    if relu:
        o = _relu(o)
    return o.to(x.dtype)


def model_bwd(dy, dy2, mask, x, mean, gamma, invstd, geo):
    """Backward statistics, finalize and apply with the kernels' rounding points."""
    m = x.shape[0]
    g = dy.float() if dy2 is None else dy.float() + dy2.float()
    if mask is not None:
        g = torch.where(mask, g, torch.zeros_like(g))
    xm = x.float() - mean.float()
    p1, p2 = model_chunk_sums(g, geo), model_chunk_sums(g * xm, geo)
    s1, s2 = p1.double().sum(1), p2.double().sum(1)
    inv, gm = invstd.double(), gamma.double()
    k1 = gm * inv
    out = dict(dgamma=(s2 * inv).float(), dbeta=s1.float(), k1=k1.float(), k2=(-k1 * inv * inv * s2 / m).float(),
               k3=(-k1 * s1 / m).float(), dz=g.to(dy.dtype))
    # the apply pass reads dz back in the I/O type when the statistics pass stored it (the same
    # number unless dy + dy2 had to be rounded)
    out["dx"] = (out["k1"] * out["dz"].float() + out["k2"] * xm + out["k3"]).to(x.dtype)
    return out


# ---- inputs ------------------------------------------------------------------------------------
def channel_params(C, device, seed=0):
    """Per-channel gamma (both signs), beta, data mean and scale, all distinct, so a channel-index
    slip cannot cancel."""
    g = torch.Generator().manual_seed(1000 + seed)
    i = torch.arange(C, dtype=torch.float64)
    sign = torch.where(torch.rand(C, generator=g) < 0.35, -1.0, 1.0).double()
    gamma = sign * (0.5 + 1.0 * (i + 1) / C + 0.003 * torch.rand(C, generator=g).double())
    beta = -0.5 + 1.0 * ((i * 7) % C) / C + 0.001 * i / C
    mu = -1.0 + 2.0 * ((i * 5 + 3) % C) / C + 0.3
    sd = 0.7 + 1.5 * ((i * 3 + 1) % C) / C
    return [t.float().to(device) for t in (gamma, beta, mu, sd)]


def activations(M, C, dtype, device, seed, mu=None, sd=None):
    """[M, C] contiguous Gaussian data in ``dtype`` (channel c: mean mu[c], scale sd[c]; default the
    existing BN tests' 0.3 and 1.7)."""
    g = torch.Generator(device=device).manual_seed(seed)
    t = torch.randn(M, C, device=device, generator=g)
    t = t * (sd if sd is not None else 1.7) + (mu if mu is not None else 0.3)
    return t.to(dtype).contiguous()


def case(M, C, dtype, device, seed=0, mu=None, sd=None):
    """The tensors one BatchNorm layer's forward and backward see, as a dict: x, a residual r, a
    second BatchNorm's input x2 and parameters, two output gradients, parameters, running stats."""
    gamma, beta, cmu, csd = channel_params(C, device, seed)
    gamma2, beta2, cmu2, csd2 = channel_params(C, device, seed + 1)
    rm0 = (0.1 * beta + 0.05).contiguous()
    rv0 = (1.0 + 0.5 * beta).contiguous()
    s = 100 * seed
    return dict(M=M, C=C, dtype=dtype, geo=geometry(M, C), gamma=gamma, beta=beta, gamma2=gamma2, beta2=beta2,
                rm0=rm0, rv0=rv0,
                x=activations(M, C, dtype, device, s + 1, cmu if mu is None else mu, csd if sd is None else sd),
                r=activations(M, C, dtype, device, s + 2), x2=activations(M, C, dtype, device, s + 5, cmu2, csd2),
                dy=activations(M, C, dtype, device, s + 3), dy2=activations(M, C, dtype, device, s + 4))


def cond_case(dtype, device):
    """The stem's statistics: per-channel |mean| / std from 1 up to 60 (mean +-3, std 3 .. 0.05),
    M = 32769, C = 64 -> (case, ratios)."""
    C = 64
    ratio = torch.logspace(0, math.log10(60.0), C)
    sign = torch.where(torch.arange(C) % 3 == 0, -1.0, 1.0)
    return case(32769, C, dtype, device, seed=3, mu=(3.0 * sign).to(device), sd=(3.0 / ratio).to(device)), ratio


def partition(M, chunks, device, seed=0):
    """Group index [M] splitting rows 0..M-1 into exactly ``chunks`` contiguous groups of uneven
    sizes; the last group is empty when chunks > 1 (and more are when chunks > M)."""
    g = torch.Generator().manual_seed(77 + seed)
    n = chunks - 1 if chunks > 1 else 1                      # non-empty groups wanted
    n = min(n, M)
    cuts = torch.randperm(M - 1, generator=g)[: n - 1].sort().values + 1     # n - 1 distinct cut rows
    gid = torch.zeros(M, dtype=torch.long)
    gid[cuts] = 1
    return gid.cumsum(0).to(device)


def group_sums(terms64, gid, chunks):
    """fp64 sums of [M, C] terms per group, rounded to fp32 -> [C, chunks] contiguous."""
    out = torch.zeros(chunks, terms64.shape[1], dtype=torch.float64, device=terms64.device)
    out.index_add_(0, gid, terms64)
    return out.float().t().contiguous()
