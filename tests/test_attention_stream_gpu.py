"""Streaming attention kernels (csrc/kernels/attn_stream_kernels.hip, 257 .. 4096 tokens) against
the fp64 reference and the derived rounding bounds of tests/attention_oracle.py - the acceptance
rule of tests/test_attention_gpu.py, unchanged: out, dQ, dK, dV within FACTOR x their elementwise
bound, lse2 within 1e-3 + 1e-5 |lse2|, everything finite.  Run with -s for the worst ratios
(profiles/attn_stream.md)."""
import math

import pytest
import torch
import torch.nn.functional as F

import attention_oracle as ao
import attention_stream_oracle as aso
from distributed_pytorch_training_amd import ops
from distributed_pytorch_training_amd.ops import attention as fa

pytestmark = pytest.mark.gpu

FACTOR = 1.25     # tests/test_attention_gpu.py's: second-order terms, fp32 accumulation, v_exp_f32
KINDS = ("gauss", "peaked", "negative", "lastkey", "firstkey")   # firstkey: lastkey mirrored
# (queries per workgroup, keys per chunk, query rows per backward chunk); None before the feature
TILES = (tuple(ops.native().attn_stream_tiles())
         if ops.native_available() and hasattr(ops.native(), "attn_stream_tiles") else None)


def _sweep_lengths():
    """Both sides and the exact value of the first three multiples above 256 of each tile size,
    257 and the ViT-B/16 lengths at 272, 288 and 384 px."""
    lengths = {257, 290, 325, 577}
    for t in TILES or ():
        first = 256 // t + 1
        for mult in range(first, first + 3):
            lengths.update((mult * t - 1, mult * t, mult * t + 1))
    return sorted(lengths)


SWEEP_S = _sweep_lengths()
_WORST = {}
_CASES = {}


def _shape(S):
    return (1, 2) if S > 600 else (2, 3)


def _case(cuda, kind, S, scale, B=None, H=None):
    """Inputs on the GPU with their fp64 reference (out, lse2, dqkv) and bounds, computed once."""
    if B is None:
        B, H = _shape(S)
    key = (kind, B, S, H, scale)
    if key not in _CASES:
        qkv, dout = ao.inputs("lastkey" if kind == "firstkey" else kind, B, S, H, S * 7 + H)
        if kind == "firstkey":
            qkv, dout = aso.mirror(qkv, dout)
        qkv, dout = qkv.to(cuda), dout.to(cuda)
        ref = ao.reference(qkv, dout, H, scale)
        _CASES[key] = (qkv, dout, H, ref[:3], ao.bounds(qkv, dout, H, scale))
    return _CASES[key]


def _stream(qkv, dout, H, scale):
    C = ops.native()
    out, lse = C.attn_stream_fwd(qkv, H, scale)
    return out, lse, C.attn_stream_bwd(qkv, out, dout, lse, H, scale)


def _named(out, dqkv, H):
    dq, dk, dv = ao.split_dqkv(dqkv, H)
    return {"out": out, "dQ": dq, "dK": dk, "dV": dv}


def _ratios(case, out, dqkv):
    _, _, H, ref, bound = case
    want, got = _named(ref[0], ref[2], H), _named(out, dqkv, H)
    return {n: ao.worst_ratio(got[n], want[n], e) for n, e in zip(("out", "dQ", "dK", "dV"), bound)}


def _lse_excess(lse, want, S):
    """max of |lse2 - want| - (1e-3 + 1e-5 |want|) over the slots < S, and the worst |error|."""
    want = want.reshape(-1, S)
    err = (lse[:, :S].double() - want).abs()
    return (err - (1e-3 + 1e-5 * want.abs())).max().item(), err.max().item()


def _check(case, got, S, tag, worst=None, kind=None):
    out, lse, dqkv = got
    ratios = _ratios(case, out, dqkv)
    excess, ratios["lse2"] = _lse_excess(lse, case[3][1], S)
    if worst is not None:
        w = worst.setdefault(kind, dict.fromkeys(ratios, 0.0))
        for n, r in ratios.items():
            w[n] = max(w[n], r)
    print(f"\n{tag}: " + " ".join(f"{n} {r:.3g}" for n, r in ratios.items()), end="")
    for n in ("out", "dQ", "dK", "dV"):
        assert ratios[n] <= FACTOR, f"{tag}: {n} error is {ratios[n]:.3f} x its bound"
    assert excess <= 0, f"{tag}: lse2 off by {ratios['lse2']:.3e}"
    assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all(), tag


@pytest.fixture(scope="module")
def worst():
    yield _WORST
    if _WORST:
        print("\nstreaming attention kernels vs fp64 reference, worst error / bound (lse2: worst abs error)")
        print(f"{'kind':10s} {'out':>7s} {'dQ':>7s} {'dK':>7s} {'dV':>7s} {'lse2':>9s}")
        for kind, w in _WORST.items():
            print(f"{kind:10s} {w['out']:7.3f} {w['dQ']:7.3f} {w['dK']:7.3f} {w['dV']:7.3f} {w['lse2']:9.2e}")


def test_stream_tiles_binding():
    assert TILES is not None, "attn_stream_tiles binding is missing"
    qb, kc, qc = TILES
    assert qb % 32 == 0 and kc % 32 == 0 and qc % 32 == 0 and min(TILES) >= 32


@pytest.mark.parametrize("scale", [0.125, 0.3])
@pytest.mark.parametrize("S", SWEEP_S)
@pytest.mark.parametrize("kind", KINDS)
def test_stream_within_rounding_bounds(cuda, worst, kind, S, scale):
    """Every chunk count up to the third tile multiple above 256 and both sides of each edge, data
    that makes a mask or rescale mistake visible (lastkey: every earlier chunk is rescaled when the
    maximum arrives in the last one; firstkey: every later chunk is added under an old maximum)."""
    case = _case(cuda, kind, S, scale)
    if kind in ("lastkey", "firstkey"):
        key = S - 1 if kind == "lastkey" else 0
        assert aso.dominant_probability(case[0], case[2], scale, key) > 0.9
    _check(case, _stream(case[0], case[1], case[2], scale), S, f"{kind} S={S} scale={scale}", worst, kind)


@pytest.mark.parametrize("scale", [0.125, 0.3])
@pytest.mark.parametrize("S", [785, 1025])
@pytest.mark.parametrize("kind", ["gauss", "lastkey", "firstkey"])
def test_stream_within_rounding_bounds_long(cuda, worst, kind, S, scale):
    """ViT-B/16 at 448 and 512 px (7 and 9 chunks), one image and two heads."""
    case = _case(cuda, kind, S, scale, 1, 2)
    if kind != "gauss":
        assert aso.dominant_probability(case[0], 2, scale, S - 1 if kind == "lastkey" else 0) > 0.9
    _check(case, _stream(case[0], case[1], 2, scale), S, f"{kind} S={S} scale={scale}", worst, kind)


@pytest.mark.parametrize("S", [1, 5, 31, 32, 33, 129, 255, 256])
@pytest.mark.parametrize("kind", ["gauss", "lastkey"])
def test_stream_short_sequences_match_bounds_and_on_chip_lse(cuda, kind, S):
    """One partial chunk (where an uninitialised running maximum would show), two full ones at 256:
    the same bounds, and lse2 next to the on-chip kernel's."""
    scale = 0.125
    case = _case(cuda, kind, S, scale, 2, 3)
    got = _stream(case[0], case[1], 3, scale)
    _check(case, got, S, f"{kind} S={S}")
    _, lse_chip = ops.native().attn_fwd(case[0], 3, scale)
    assert got[1].shape == lse_chip.shape
    assert _lse_excess(got[1], lse_chip[:, :S].double(), S)[0] <= 0


def test_stream_counts_keys_across_chunk_edges(cuda):
    """All keys equal: p == 1/S exactly, so out = mean(V), lse2 = s * scale * log2(e) + log2(S)
    and dV = mean_q(dO) - one key too many or too few shows at every S across two chunk edges."""
    assert TILES is not None
    kc = TILES[1]
    B, H, scale = 1, 2, 0.125
    lengths = list(range(2 * kc - 2, 2 * kc + 35)) + [577]
    rows = []
    for S in lengths:
        qkv, dout = ao.inputs("uniform", B, S, H, S * 7 + H)
        qkv, dout = qkv.to(cuda), dout.to(cuda)
        out, lse, dqkv = _stream(qkv, dout, H, scale)
        q, k, v = ao.split_heads(qkv.double(), H)
        mean_v = ao.merge_heads(v.mean(2, keepdim=True).expand_as(v))
        e_out = 2 * ao.U * ao.merge_heads(v.abs().mean(2, keepdim=True).expand_as(v))
        want_lse = ((q * k[:, :, :1]).sum(-1) * scale * ao.LOG2E + math.log2(S)).reshape(-1, S)
        do = dout.double()
        want_dv = do.mean(1, keepdim=True).expand_as(do)
        e_dv = ao.U * do.abs().mean(1, keepdim=True).expand_as(do) + ao.U * want_dv.abs()
        lse_err = (lse[:, :S].double() - want_lse).abs()
        rows.append(torch.stack([
            ((out.double() - mean_v).abs() - ao.TINY - e_out).max(),
            (lse_err - (1e-3 + 1e-5 * want_lse.abs())).max(),
            ((ao.split_dqkv(dqkv, H)[2].double() - want_dv).abs() - ao.TINY - e_dv).max()]))
    excess = torch.stack(rows).cpu()           # one synchronisation for the whole loop
    for col, name in enumerate(("out vs mean(V)", "lse2", "dV")):
        bad = [(S, f"{excess[i, col].item():.3e}") for i, S in enumerate(lengths) if not excess[i, col] <= 0]
        assert not bad, f"{name} outside its bound at (S, excess): {bad[:8]}"


@pytest.mark.parametrize("S", [289, 577])
def test_stream_bwd_masks_padding_keys_before_exp2(cuda, S):
    """Every scaled score near -118 (lse2 < -128): an admitted padding key's P = exp2(0 - lse2)
    overflows and inf * 0 would put NaN into dQ; the mask ahead of the exponential keeps it out."""
    scale = 0.7
    case = _case(cuda, "negative", S, scale, 2, 3)
    assert case[3][1].max().item() < -128
    _check(case, _stream(case[0], case[1], 3, scale), S, f"negative S={S} scale={scale}")


def test_stream_is_run_to_run_bitwise_equal(cuda):
    """No atomics: the same inputs give the same bits, forward and backward."""
    S = 577
    case = _case(cuda, "gauss", S, 0.125, 2, 3)
    a, b = _stream(case[0], case[1], 3, 0.125), _stream(case[0], case[1], 3, 0.125)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][:, :S], b[1][:, :S]) and torch.equal(a[2], b[2])


def test_stream_layout_empty_batch_and_argument_checks(cuda):
    C = ops.native()
    B, S, H, scale = 2, 290, 3, 0.125
    d3 = 3 * H * 64
    case = _case(cuda, "gauss", S, scale, B, H)
    qkv, dout = case[0], case[1]
    wide = torch.zeros(B, S, d3 + 64, device=cuda, dtype=torch.bfloat16)
    wide[:, :, :d3] = qkv
    view = wide[:, :, :d3]
    assert not view.is_contiguous()
    with pytest.raises(RuntimeError):
        C.attn_stream_fwd(view, H, scale)
    out, lse = C.attn_stream_fwd(qkv, H, scale)
    with pytest.raises(RuntimeError):
        C.attn_stream_bwd(view, out, dout, lse, H, scale)
    old = fa.ENABLED, fa.STREAMING
    fa.ENABLED = fa.STREAMING = True
    try:
        outs = []
        for x in (wide.requires_grad_(True)[:, :, :d3], qkv.clone().requires_grad_(True)):
            y = fa.attention(x, H)
            y.backward(dout)
            outs.append(y.detach())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], out)
        assert torch.equal(wide.grad[:, :, :d3], C.attn_stream_bwd(qkv, out, dout, lse, H, scale))
        assert not wide.grad[:, :, d3:].any()
    finally:
        fa.ENABLED, fa.STREAMING = old
    # B = 0: empty tensors without a launch, and the next call is unaffected
    qkv0 = torch.zeros(0, S, d3, device=cuda, dtype=torch.bfloat16)
    out0, lse0 = C.attn_stream_fwd(qkv0, H, scale)
    assert out0.shape == (0, S, H * 64) and out0.dtype == torch.bfloat16
    assert lse0.shape == (0, 320) and lse0.dtype == torch.float32
    dqkv0 = C.attn_stream_bwd(qkv0, out0, torch.zeros_like(out0), lse0, H, scale)
    assert dqkv0.shape == (0, S, d3) and dqkv0.dtype == torch.bfloat16
    torch.cuda.synchronize()
    _check(case, _stream(qkv, dout, H, scale), S, "after the empty batch")

    def z(*shape, dtype=torch.bfloat16):
        return torch.zeros(*shape, device=cuda, dtype=dtype)

    for bad in (z(1, 4097, d3), z(1, 290, d3, dtype=torch.float16), z(1, 290, d3 + 8), z(1, 0, d3), z(290, d3)):
        with pytest.raises(RuntimeError):
            C.attn_stream_fwd(bad, H, scale)
    with pytest.raises(RuntimeError, match="S <= 4096"):
        C.attn_stream_bwd(z(1, 4097, d3), z(1, 4097, H * 64), z(1, 4097, H * 64),
                          z(H, 4128, dtype=torch.float32), H, scale)
    with pytest.raises(RuntimeError):
        C.attn_stream_bwd(z(1, 290, d3, dtype=torch.float16), z(1, 290, H * 64), z(1, 290, H * 64),
                          z(H, 320, dtype=torch.float32), H, scale)
    with pytest.raises(RuntimeError, match="bad lse"):
        C.attn_stream_bwd(z(1, 290, d3), z(1, 290, H * 64), z(1, 290, H * 64), z(H, 352, dtype=torch.float32), H,
                          scale)
    # the on-chip bindings keep rejecting what they rejected
    with pytest.raises(RuntimeError, match="S <= 256"):
        C.attn_fwd(z(1, 257, d3), H, scale)


def test_stream_routing(cuda):
    H = 2
    d3 = 3 * H * 64

    def z(*shape, dtype=torch.bfloat16, device=cuda):
        return torch.zeros(*shape, device=device, dtype=dtype)

    old = fa.ENABLED, fa.STREAMING
    fa.ENABLED = fa.STREAMING = True
    try:
        assert not fa.supported(z(1, 257, d3), H)
        assert fa.supported_streaming(z(1, 257, d3), H) and fa.supported_streaming(z(1, 4096, d3), H)
        assert not fa.supported_streaming(z(1, 256, d3), H)
        assert not fa.supported_streaming(z(1, 4097, d3), H)
        assert not fa.supported_streaming(z(1, 290, d3, dtype=torch.float16), H)
        assert not fa.supported_streaming(z(1, 290, d3, device="cpu"), H)
        assert not fa.supported_streaming(z(290, d3), H)
        assert not fa.supported_streaming(z(1, 290, d3 + 8), H)
        fa.STREAMING = False
        assert not fa.supported_streaming(z(1, 290, d3), H)
        assert fa.supported(z(1, 256, d3), H)          # the switch is the long path's alone
        fa.STREAMING, fa.ENABLED = True, False
        assert not fa.supported_streaming(z(1, 290, d3), H)
    finally:
        fa.ENABLED, fa.STREAMING = old


def test_vit_272px_runs_streaming_attention(cuda, monkeypatch):
    """ViT-B/16 at 272 px (290 tokens) under bf16 autocast: 12 streaming forward calls per step, and
    loss and gradients as close to an fp32 run as the SDPA fallback's (the rule of
    test_vit_fused_encoder_matches_unfused)."""
    import copy

    from distributed_pytorch_training_amd.models import build_model
    from distributed_pytorch_training_amd.models.vit import set_native

    C = ops.native()
    calls = []
    real = C.attn_stream_fwd

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(C, "attn_stream_fwd", counting)
    monkeypatch.setattr(fa, "ENABLED", True)
    torch.manual_seed(0)
    base = build_model("vit_b_16", 10, cuda, image_size=272)
    with torch.no_grad():      # torchvision zero-inits the head: give it values so grads flow
        base.heads.head.weight.normal_(std=0.02)
    x = torch.randn(2, 3, 272, 272, device=cuda)
    y = torch.randint(0, 10, (2,), device=cuda)

    def run(model, autocast, streaming):
        monkeypatch.setattr(fa, "STREAMING", streaming)
        del calls[:]
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            loss = F.cross_entropy(model(x), y)
        forward_calls = len(calls)
        loss.backward()
        grads = {n: p.grad.detach().float().clone() for n, p in model.named_parameters()}
        return loss.detach(), grads, forward_calls

    stream_m, sdpa_m, ref_m = (copy.deepcopy(base) for _ in range(3))
    set_native(stream_m)
    set_native(sdpa_m)
    ls, gs, n_stream = run(stream_m, True, True)
    lu, gu, n_sdpa = run(sdpa_m, True, False)
    lr, gr, _ = run(ref_m, False, False)
    assert n_stream == 12 and n_sdpa == 0
    assert abs(ls - lr) < 2e-2 and abs(lu - lr) < 2e-2
    for n in gr:
        scale = gr[n].abs().max().item() + 1e-6
        es = (gs[n] - gr[n]).abs().max().item() / scale
        eu = (gu[n] - gr[n]).abs().max().item() / scale
        assert es < max(3 * eu, 0.05), (n, es, eu)


def test_stream_replays_in_a_captured_graph(cuda, monkeypatch):
    """Forward and backward at 290 tokens captured in a graph: two replays, each bitwise equal to
    the eager result (current stream only, no host synchronisation, scratch from the allocator)."""
    monkeypatch.setattr(fa, "ENABLED", True)
    monkeypatch.setattr(fa, "STREAMING", True)
    B, S, H = 2, 290, 3
    case = _case(cuda, "gauss", S, 0.125, B, H)
    qkv = case[0].clone().requires_grad_(True)
    dout = case[1]
    out_e = fa.attention(qkv, H)
    (grad_e,) = torch.autograd.grad(out_e, qkv, dout)
    out_e, grad_e = out_e.detach().clone(), grad_e.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.autograd.grad(fa.attention(qkv, H), qkv, dout)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = fa.attention(qkv, H)
        (grad_g,) = torch.autograd.grad(out_g, qkv, dout)
    for _ in range(2):
        with torch.no_grad():
            out_g.zero_()
            grad_g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_g.detach(), out_e) and torch.equal(grad_g, grad_e)
