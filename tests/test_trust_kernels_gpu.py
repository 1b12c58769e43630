"""trust_kernels.hip (LARS / LAMB over a flat arena) against the fp64 oracle and the derived ratio
bounds of tests/trust_oracle.py.

One hand-made arena: segments of 1, 3, 10, 16, 1000 elements, one chunk, one chunk + 4 and three
chunks + 20, each on a 16-element boundary, inside sentinel-padded buffers.  One segment has an
all-zero gradient, one all-zero weights, two are excluded (1-D rule: both flag bits clear).  A
second case is one segment of more chunks than the launch's grid cap, so the grid-stride loops take
their second trip.
"""
import pytest
import torch

import trust_oracle as orc
from distributed_pytorch_training_amd import ops
from distributed_pytorch_training_amd.ops import trust
from distributed_pytorch_training_amd.optim import FusedLAMB, FusedLARS
from distributed_pytorch_training_amd.parallel.flat import FlatArena

pytestmark = pytest.mark.gpu

C = trust.TRUST_CHUNK
PAD = 8
SENT32, SENT16 = 0x4B5A5A5A, 0x5B5A
NUMELS = [1, 3, 10, 16, 1000, C, C + 4, 3 * C + 20]
FLAGS = [3, 0, 0, 3, 3, 1, 3, 3]          # segments 1 and 2 excluded; segment 5 adapts without decay
ZERO_W, ZERO_G = 3, 4
GRID_CAP = 2048                           # kMaxBlocks (csrc/kernels/common.h)
BIG = (GRID_CAP + 1) * C + 20             # 2050 chunks: 8,392,724 elements

LARS_KW = dict(lr=0.5, momentum=0.9, weight_decay=5e-4, eta=0.02)
LAMB_KW = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.01)


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


def _layout(numels, order=None):
    """Offsets (by segment id) of the segments laid out in ``order``, each on a 16-element boundary."""
    order = list(range(len(numels))) if order is None else order
    offsets, cur = [0] * len(numels), 0
    for i in order:
        cur = (cur + 15) // 16 * 16
        offsets[i] = cur
        cur += numels[i]
    return offsets, (cur + 63) // 64 * 64


def _content(seg, n, kind):
    """What segment ``seg`` holds, whatever its place in the arena (kind 0: weights, 1: gradients)."""
    g = torch.Generator().manual_seed(1000 * kind + seg)
    v = torch.randn(n, generator=g) * (1.0 if kind == 0 else 0.1)
    if (kind == 0 and seg == ZERO_W) or (kind == 1 and seg == ZERO_G):
        v.zero_()
    return v


class Case:
    """Arenas for p, g and two state tensors over one layout, and the table in arena order."""

    def __init__(self, dev, numels=NUMELS, flags=FLAGS, order=None, shadow=None):
        self.order = list(range(len(numels))) if order is None else order
        offs, self.total = _layout(numels, order)
        self.offsets = [offs[i] for i in self.order]           # arena order
        self.numels = [numels[i] for i in self.order]
        self.flags = [flags[i] for i in self.order]
        self.ids = self.order
        self.dev = dev
        z = torch.zeros(self.total)
        self.p0, self.g0 = z.clone(), z.clone()
        for off, n, seg in zip(self.offsets, self.numels, self.ids):
            self.p0[off:off + n] = _content(seg, n, 0)
            self.g0[off:off + n] = _content(seg, n, 1)
        self.P, self.G, self.S1, self.S2 = (Arena(self.total, dev).set(v) for v in (self.p0, self.g0, z, z))
        self.SH = Arena(self.total, dev, shadow).set(torch.zeros(self.total)) if shadow is not None else None
        self.table = ops.trust_segments(self.offsets, self.numels, self.flags, self.total, dev)
        self.step = torch.zeros(1, device=dev)
        self.fi = torch.zeros(1, device=dev)
        self.pad = torch.ones(self.total, dtype=torch.bool)
        for off, n in zip(self.offsets, self.numels):
            self.pad[off:off + n] = False

    def layout(self):
        return self.offsets, self.numels, self.flags

    def lars(self, nesterov=False, scale=None, host_factor=1.0, zero_grad=True, fi=None, **over):
        ops.lars_step(self.P.t, self.G.t, self.S1.t, self.table, self.table.ratio, **dict(LARS_KW, **over),
                      nesterov=nesterov, scale=scale, host_factor=host_factor,
                      found_inf=self.fi if fi is None else fi, step=self.step, zero_grad=zero_grad,
                      shadow=self.SH.t if self.SH else None)

    def lamb(self, scale=None, host_factor=1.0, zero_grad=True, fi=None, **over):
        ops.lamb_step(self.P.t, self.G.t, self.S1.t, self.S2.t, self.table, self.table.ratio,
                      **dict(LAMB_KW, **over), scale=scale, host_factor=host_factor,
                      found_inf=self.fi if fi is None else fi, step=self.step, zero_grad=zero_grad,
                      shadow=self.SH.t if self.SH else None)

    def tail(self, fi=None):
        ops.optim_tail(None, None, self.fi if fi is None else fi, self.step)

    def ratios(self):
        return self.table.ratio.cpu().double().tolist()

    def arenas(self):
        return [a for a in (self.P, self.G, self.S1, self.S2, self.SH) if a is not None]

    def check_frame(self, state=2):
        """Sentinels intact; padding between the segments bitwise zero in p and the state."""
        assert all(a.intact() for a in self.arenas())
        for a in (self.P, self.S1, self.S2)[:1 + state]:
            assert not a.bits().cpu()[self.pad].any()


def _check_ratios(got, exact, bounds, ids, pinned, tag=""):
    """``pinned`` segments give exactly 1.0, the others lie within their derived bound."""
    for r, e, b, seg in zip(got, exact, bounds, ids):
        print(f"{tag}segment {seg}: ratio {r:.9g} exact {e:.9g} rel.err {abs(r - e) / e:.3g} bound {b:.3g}")
        if seg in pinned:
            assert r == 1.0 and e == 1.0, seg
        else:
            assert e != 1.0 and abs(r - e) <= b * e, (seg, r, e, b)


EXCLUDED = {i for i, fl in enumerate(FLAGS) if not fl & 1}


# ---- LARS -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "nesterov", "scaled"])
def test_lars_three_steps(cuda, variant):
    c = Case(cuda)
    nesterov = variant == "nesterov"
    scale, hf, mult = (torch.tensor([256.0], device=cuda), 0.25, 1024.0) if variant == "scaled" else (None, 1.0, 1.0)
    p64, b64 = c.p0.double(), torch.zeros(c.total, dtype=torch.float64)
    bounds = [orc.lars_ratio_bound(n, C) for n in c.numels]
    for it in range(3):
        g = c.g0 * (it + 1) * mult
        c.G.set(g)
        p_in = c.P.t.cpu().clone()
        c.lars(nesterov=nesterov, scale=scale, host_factor=hf)
        c.tail()
        got = c.ratios()
        kw = dict(LARS_KW, nesterov=nesterov, factor=hf / 256.0 if scale is not None else 1.0, first=it == 0)
        _, _, exact = orc.lars_oracle(p_in, g, b64, *c.layout(), **kw)          # from what the kernel read
        # the zero-weight segment moves off zero with its first update (ratio 1, d = g)
        _check_ratios(got, exact, bounds, c.ids, EXCLUDED | {ZERO_G} | ({ZERO_W} if it == 0 else set()), f"step {it} ")
        p64, b64, _ = orc.lars_oracle(p64, g, b64, *c.layout(), ratios=got, **kw)
        assert torch.count_nonzero(c.G.t) == 0
    assert c.step.item() == 3.0
    torch.testing.assert_close(c.P.t.cpu().double(), p64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(c.S1.t.cpu().double(), b64, rtol=1e-5, atol=1e-6)
    assert not torch.equal(c.P.t.cpu(), c.p0)
    c.check_frame(state=1)


# ---- LAMB -------------------------------------------------------------------------------------------
def test_lamb_three_steps(cuda):
    c = Case(cuda)
    z = torch.zeros(c.total, dtype=torch.float64)
    p64, m64, v64 = c.p0.double(), z.clone(), z.clone()
    for it in range(3):
        g = c.g0 * (it + 1)
        c.G.set(g)
        p_in = c.P.t.cpu().clone()
        c.lamb()
        c.tail()
        got = c.ratios()
        exact, amp = orc.lamb_ratio_from_stored(p_in, c.S1.t, c.S2.t, *c.layout(), beta1=LAMB_KW["beta1"],
                                                beta2=LAMB_KW["beta2"], eps=LAMB_KW["eps"],
                                                weight_decay=LAMB_KW["weight_decay"], t=it + 1)
        bounds = [orc.lamb_ratio_bound(n, C, a) for n, a in zip(c.numels, amp)]
        # a zero gradient does not pin LAMB's ratio (u = wd p): only the excluded segments and, until
        # its first update moves it off zero, the zero-weight segment give exactly 1
        _check_ratios(got, exact, bounds, c.ids, EXCLUDED | ({ZERO_W} if it == 0 else set()), f"step {it} ")
        p64, m64, v64, _ = orc.lamb_oracle(p64, g, m64, v64, *c.layout(), ratios=got, t=it + 1, **LAMB_KW)
        assert torch.count_nonzero(c.G.t) == 0
    assert c.step.item() == 3.0
    torch.testing.assert_close(c.P.t.cpu().double(), p64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(c.S1.t.cpu().double(), m64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(c.S2.t.cpu().double(), v64, rtol=1e-5, atol=1e-6)
    assert not torch.equal(c.P.t.cpu(), c.p0)
    c.check_frame()


# ---- more chunks than the grid cap ------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_second_grid_stride_trip(cuda, opt):
    c = Case(cuda, numels=[BIG], flags=[3])
    assert c.table.nchunks == GRID_CAP + 2 and c.table.chunks[-1] == ((GRID_CAP + 1) * C, 20, 0)
    # the tail of the segment, which only the second trip reaches, carries most of the norm
    tail = slice((GRID_CAP + 1) * C - 100, BIG)
    c.P.t[tail] *= 2000.0
    c.G.t[tail] *= 2000.0
    p_in, g_in = c.P.t.cpu().clone(), c.G.t.cpu().clone()
    z = torch.zeros(c.total, dtype=torch.float64)
    if opt == "lars":
        c.lars()
        got = c.ratios()
        _, _, exact = orc.lars_oracle(p_in, g_in, z, [0], [BIG], [3], **LARS_KW, nesterov=False, first=True)
        bound = orc.lars_ratio_bound(BIG, C)
        p64, s64, _ = orc.lars_oracle(p_in, g_in, z, [0], [BIG], [3], **LARS_KW, nesterov=False, first=True, ratios=got)
    else:
        c.lamb()
        got = c.ratios()
        exact, amp = orc.lamb_ratio_from_stored(p_in, c.S1.t, c.S2.t, [0], [BIG], [3], beta1=LAMB_KW["beta1"],
                                                beta2=LAMB_KW["beta2"], eps=LAMB_KW["eps"],
                                                weight_decay=LAMB_KW["weight_decay"], t=1)
        bound = orc.lamb_ratio_bound(BIG, C, amp[0])
        p64, s64, _, _ = orc.lamb_oracle(p_in, g_in, z, z, [0], [BIG], [3], ratios=got, t=1, **LAMB_KW)
    print(f"{opt}: ratio {got[0]:.9g} exact {exact[0]:.9g} rel.err {abs(got[0] - exact[0]) / exact[0]:.3g} bound {bound:.3g}")
    assert abs(got[0] - exact[0]) <= bound * exact[0]
    # a ratio that missed the tail would be far outside the bound: the tail holds > 90 % of ||p||^2
    assert float(p_in[tail].double().square().sum() / p_in.double().square().sum()) > 0.9
    torch.testing.assert_close(c.P.t.cpu().double(), p64, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(c.S1.t.cpu().double(), s64, rtol=1e-5, atol=1e-6)
    assert torch.count_nonzero(c.G.t) == 0
    c.check_frame()


# ---- found_inf, zero_grad, shadows -------------------------------------------------------------------
@pytest.mark.parametrize("zero_grad", [True, False])
@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_found_inf_leaves_everything_but_grad(cuda, opt, zero_grad):
    c = Case(cuda, shadow=torch.bfloat16)
    g = torch.Generator().manual_seed(3)
    for a in (c.S1, c.S2):
        a.set(torch.where(c.pad, torch.zeros(c.total), torch.rand(c.total, generator=g)))
    c.G.t[c.offsets[-1] + 5] = float("inf")
    c.step.fill_(2.0)
    c.fi.fill_(1.0)
    before = [a.bits() for a in c.arenas()]
    getattr(c, opt)(zero_grad=zero_grad)
    after = [a.bits() for a in c.arenas()]
    for i, name in ((0, "p"), (2, "buf / exp_avg"), (3, "exp_avg_sq"), (4, "shadow")):
        assert torch.equal(after[i], before[i]), name
    if zero_grad:
        assert torch.count_nonzero(after[1]) == 0
    else:
        assert torch.equal(after[1], before[1])
    c.tail()
    assert c.step.item() == 2.0 and c.fi.item() == 0.0
    c.check_frame(state=0)


@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_zero_grad_false_keeps_grad(cuda, opt):
    c, d = Case(cuda), Case(cuda)
    gbits = c.G.bits()
    getattr(c, opt)(zero_grad=False)
    getattr(d, opt)(zero_grad=True)
    assert torch.equal(c.G.bits(), gbits) and torch.count_nonzero(d.G.t) == 0
    for a, b in zip((c.P, c.S1, c.S2), (d.P, d.S1, d.S2)):
        assert torch.equal(a.bits(), b.bits())
    assert not torch.equal(c.P.t.cpu(), c.p0)
    c.check_frame()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_shadow_is_rounding_of_new_param(cuda, opt, dt):
    c = Case(cuda, shadow=dt)
    for it in range(2):
        c.G.set(c.g0 * (it + 1))
        before = c.P.bits()
        getattr(c, opt)()
        c.tail()
        assert not torch.equal(c.P.bits(), before)
        assert torch.equal(c.SH.t, c.P.t.to(dt)), f"step {it}"
    c.check_frame()


# ---- determinism and position independence ----------------------------------------------------------
@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_bitwise_repeatable_and_position_independent(cuda, opt):
    """Same segment contents, two runs in one layout and one in another order at other offsets:
    ratios and updated values agree to the bit, segment by segment."""
    runs = [Case(cuda), Case(cuda), Case(cuda, order=[7, 2, 5, 0, 6, 4, 1, 3])]
    assert runs[2].offsets != runs[0].offsets
    for c in runs:
        for it in range(2):
            c.G.set(c.g0 * (it + 1))
            getattr(c, opt)(nesterov=True) if opt == "lars" else c.lamb()
            c.tail()
    a = runs[0]
    for c in runs[1:]:
        rb = dict(zip(c.ids, c.table.ratio.view(torch.int32).tolist()))
        off_b = dict(zip(c.ids, c.offsets))
        for seg, off, n, r in zip(a.ids, a.offsets, a.numels, a.table.ratio.view(torch.int32).tolist()):
            assert rb[seg] == r, seg
            for x, y in zip((a.P, a.S1, a.S2), (c.P, c.S1, c.S2)):
                assert torch.equal(x.bits()[off:off + n], y.bits()[off_b[seg]:off_b[seg] + n]), seg
        c.check_frame()


# ---- hipGraph ----------------------------------------------------------------------------------------
def _params(dev):
    g = torch.Generator().manual_seed(11)
    shapes = [(96, 64), (33,), (7, 5, 3, 3), (2 * C + 12,), (40, 100)]
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]


def _grads(arena, k):
    """A gradient arena: random inside the parameters, zero in the padding."""
    flat = torch.zeros_like(arena.grad_flat)
    g = torch.Generator().manual_seed(50 + k)
    for v in arena.views(flat):
        v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    return flat


@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_graph_replay_matches_eager(cuda, opt):
    def make():
        arena = FlatArena(_params(cuda))
        if opt == "lars":
            return arena, FusedLARS(arena, lr=0.5, momentum=0.9, weight_decay=5e-4, trust_coefficient=0.02)
        return arena, FusedLAMB(arena, lr=0.01, eps=1e-6, weight_decay=0.01)

    ea, eo = make()
    for k in range(3):
        ea.grad_flat.copy_(_grads(ea, k))
        eo.step()
    ga, go = make()
    p0 = ga.param_flat.clone()
    go.step()                                   # eager warm-up: builds the table, allocates the state
    torch.cuda.synchronize()
    ga.param_flat.copy_(p0)                     # ... and is undone
    for s in go.arena_state():
        s.zero_()
    go._step.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        go.step()
    for k in range(3):
        ga.grad_flat.copy_(_grads(ga, k))
        graph.replay()
    torch.cuda.synchronize()
    assert go.steps_taken.item() == 3.0 and eo.steps_taken.item() == 3.0
    assert torch.equal(ga.param_flat, ea.param_flat) and not torch.equal(ga.param_flat, p0)
    for a, b in zip(go.arena_state(), eo.arena_state()):
        assert torch.equal(a, b)
    assert torch.equal(go.trust_ratios, eo.trust_ratios)
    assert torch.count_nonzero(ga.grad_flat) == 0


def test_table_must_exist_before_capture(cuda, monkeypatch):
    """A step that would have to build its table (or allocate state) inside a captured region
    refuses; the eager warm-up steps that precede a capture build both."""
    arena = FlatArena(_params(cuda))
    opt = FusedLARS(arena, lr=0.1)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before"):
        opt.step()
    monkeypatch.undo()
    opt.step()
    first = opt._table
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    arena.grad_flat.copy_(_grads(arena, 0))
    p = arena.param_flat.clone()
    opt.step()                                   # table and state exist: nothing to build
    assert opt._table is first and not torch.equal(arena.param_flat, p)
