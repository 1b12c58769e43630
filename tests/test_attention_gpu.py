"""Fused MFMA self-attention (csrc/kernels/attn_kernels.hip) vs an fp32 PyTorch reference."""
import math

import pytest
import torch

import attention_oracle as ao
from distributed_pytorch_training_amd import ops
from distributed_pytorch_training_amd.ops import attention as fa

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,S,H", [(2, 197, 12), (3, 64, 2), (1, 33, 4), (2, 256, 3), (4, 5, 1)])
def test_attention_fwd_bwd_matches_fp32(cuda, B, S, H):
    g = torch.Generator(device=cuda).manual_seed(S + H)
    qkv = (torch.randn(B, S, 3 * H * 64, device=cuda, generator=g) * 1.5).to(torch.bfloat16)
    qkv.requires_grad_(True)
    out = fa.attention(qkv, H)
    ref_in = qkv.detach().float().requires_grad_(True)
    ref = fa.reference_attention(ref_in, H)
    torch.testing.assert_close(out.float(), ref, rtol=2e-2, atol=2e-2)
    # lse2 matches log2-sum-exp of the scaled scores
    _, lse = ops.native().attn_fwd(qkv.detach(), H, 1 / 8)
    q, k, _ = ref_in.detach().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4).unbind(0)
    want = torch.logsumexp(q @ k.transpose(-1, -2) / 8, dim=-1) / math.log(2)
    torch.testing.assert_close(lse.view(B * H, -1)[:, :S], want.reshape(B * H, S), rtol=1e-3, atol=2e-2)
    dout = torch.randn(B, S, H * 64, device=cuda, generator=g).to(torch.bfloat16)
    out.backward(dout)
    ref.backward(dout.float())
    gq, gr = qkv.grad.float(), ref_in.grad
    scale = gr.abs().max().item()
    torch.testing.assert_close(gq, gr, rtol=3e-2, atol=2e-2 * scale)
    assert ((gq - gr).norm() / gr.norm()).item() < 2e-2


def test_vit_uses_fused_attention(cuda):
    from distributed_pytorch_training_amd.models import build_model

    from distributed_pytorch_training_amd.models.vit import set_native

    m = build_model("vit_b_16", 10, cuda, image_size=32).train()
    assert set_native(m) > 0
    x = torch.randn(2, 3, 32, 32, device=cuda)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y1 = m(x)
    fa.ENABLED = False
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y2 = m(x)
    finally:
        fa.ENABLED = True
    torch.testing.assert_close(y1.float(), y2.float(), rtol=5e-2, atol=5e-2)


def test_attention_bwd_phase_split_is_bitwise_identical(cuda):
    """The backward as two phase kernels (dK/dV over Q and dO images, dQ over K and V images,
    the ViT-B/16 default) computes exactly what the one two-phase kernel does."""
    C = ops.native()
    g = torch.Generator(device=cuda).manual_seed(5)
    B, S, H = 3, 197, 4
    qkv = (torch.randn(B, S, 3 * H * 64, device=cuda, generator=g) * 1.5).to(torch.bfloat16)
    dout = torch.randn(B, S, H * 64, device=cuda, generator=g).to(torch.bfloat16)
    out, lse = C.attn_fwd(qkv, H, 0.125)
    try:
        C.attn_set_bwd_split(0)
        one = C.attn_bwd(qkv, out, dout, lse, H, 0.125)
        C.attn_set_bwd_split(1)
        split = C.attn_bwd(qkv, out, dout, lse, H, 0.125)
    finally:
        C.attn_set_bwd_split(1)
    assert torch.equal(one, split)


# ---- every tile count, mask edges, derived error bounds (tests/attention_oracle.py) ----
# The kernels are held to the worst-case rounding bounds of their stated arithmetic against an
# fp64 reference, per tensor and per element; run with -s for the worst ratios per data kind
# (profiles/attention_error_bounds.md).

FACTOR = 1.25     # over the first-order bound: second-order terms, fp32 accumulation, v_exp_f32
SWEEP_S = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 197, 224, 225, 255, 256)
_WORST = {}


def _gpu_inputs(cuda, kind, B, S, H, seed=None):
    qkv, dout = ao.inputs(kind, B, S, H, S * 7 + H if seed is None else seed)
    return qkv.to(cuda), dout.to(cuda)


def _fwd_bwd(qkv, dout, H, scale):
    C = ops.native()
    out, lse = C.attn_fwd(qkv, H, scale)
    return out, lse, C.attn_bwd(qkv, out, dout, lse, H, scale)


def _named(out, dqkv, H):
    dq, dk, dv = ao.split_dqkv(dqkv, H)
    return {"out": out, "dQ": dq, "dK": dk, "dV": dv}


def _bound_ratios(qkv, dout, H, scale, out, dqkv):
    """Worst |kernel - fp64 reference| / bound for out, dQ, dK, dV, plus the reference."""
    ref = ao.reference(qkv, dout, H, scale)
    want, got = _named(ref[0], ref[2], H), _named(out, dqkv, H)
    bound = dict(zip(("out", "dQ", "dK", "dV"), ao.bounds(qkv, dout, H, scale)))
    return {n: ao.worst_ratio(got[n], want[n], bound[n]) for n in bound}, ref


def _lse_excess(lse, want, S):
    """max of |lse2 - want| - (1e-3 + 1e-5 |want|) over the slots < S, and the worst |error|."""
    want = want.reshape(-1, S)
    err = (lse[:, :S].double() - want).abs()
    return (err - (1e-3 + 1e-5 * want.abs())).max().item(), err.max().item()


@pytest.fixture(scope="module")
def worst():
    yield _WORST
    if _WORST:
        print("\nattention kernels vs fp64 reference, worst error / bound (lse2: worst abs error)")
        print(f"{'kind':10s} {'out':>7s} {'dQ':>7s} {'dK':>7s} {'dV':>7s} {'lse2':>9s}")
        for kind, w in _WORST.items():
            print(f"{kind:10s} {w['out']:7.3f} {w['dQ']:7.3f} {w['dK']:7.3f} {w['dV']:7.3f} {w['lse2']:9.2e}")


@pytest.mark.parametrize("scale", [0.125, 0.3])
@pytest.mark.parametrize("S", SWEEP_S)
@pytest.mark.parametrize("kind", ["gauss", "peaked", "negative", "lastkey"])
def test_attention_within_rounding_bounds(cuda, worst, kind, S, scale):
    """Every tile count (S = 1..256 in steps around the 32-row tiles), both sides of each tile
    edge, data that makes a mask off-by-one visible, two scales: out, dQ, dK and dV each stay
    within FACTOR x their elementwise bound, and lse2 within 1e-3 + 1e-5 |lse2|."""
    B, H = 2, 3
    qkv, dout = _gpu_inputs(cuda, kind, B, S, H)
    out, lse, dqkv = _fwd_bwd(qkv, dout, H, scale)
    ratios, ref = _bound_ratios(qkv, dout, H, scale, out, dqkv)
    excess, ratios["lse2"] = _lse_excess(lse, ref[1], S)
    w = worst.setdefault(kind, dict.fromkeys(ratios, 0.0))
    for n, r in ratios.items():
        w[n] = max(w[n], r)
    tag = f"{kind} S={S} scale={scale}"
    print(f"\n{tag}: " + " ".join(f"{n} {r:.3g}" for n, r in ratios.items()), end="")
    for n in ("out", "dQ", "dK", "dV"):
        assert ratios[n] <= FACTOR, f"{tag}: {n} error is {ratios[n]:.3f} x its bound"
    assert excess <= 0, f"{tag}: lse2 off by {ratios['lse2']:.3e}"
    assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all(), tag
    if kind == "gauss":  # per-tensor relative L2 error: at most twice the rounding model's own
        mod = ao.model(qkv, dout, H, scale)
        got, emu, want = _named(out, dqkv, H), _named(mod[0], mod[2], H), _named(ref[0], ref[2], H)
        for n in ("dQ", "dK", "dV"):
            if not want[n].any():  # S = 1: dS == 0, so dQ = dK = 0 and a relative error is undefined
                assert S == 1 and n != "dV"
                continue
            rel = ((got[n].double() - want[n]).norm() / want[n].norm()).item()
            rel_model = ((emu[n] - want[n]).norm() / want[n].norm()).item()
            print(f" | {n} rel-L2 {rel:.3g} (model {rel_model:.3g})", end="")
            assert rel <= 2 * rel_model, f"{tag}: {n} rel-L2 {rel:.3e}, the model has {rel_model:.3e}"


def test_attention_counts_keys_at_every_length(cuda):
    """All keys equal: p == 1/S exactly, so out = mean(V), lse2 = s * scale * log2(e) + log2(S)
    and dV = mean_q(dO) for every key - one key too many or too few shows at every S in 1..256."""
    B, H, scale = 1, 2, 0.125
    rows = []
    for S in range(1, 257):
        qkv, dout = _gpu_inputs(cuda, "uniform", B, S, H)
        out, lse, dqkv = _fwd_bwd(qkv, dout, H, scale)
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
        bad = [(S + 1, f"{excess[S, col].item():.3e}") for S in range(256) if not excess[S, col] <= 0]
        assert not bad, f"{name} outside its bound at (S, excess): {bad[:8]}"


@pytest.mark.parametrize("S", [33, 97, 197, 225])
def test_attention_bwd_masks_padding_keys_before_exp2(cuda, S):
    """The backward's key mask is what keeps a padding key finite, nothing else: its K row is
    zero in LDS, so an admitted padding key adds P * 0 to dQ and only touches dK / dV rows that
    are never stored - unless P = exp2(0 - lse2) overflows.  With every scaled score near -118
    (lse2 < -128) it does, and inf * 0 would put NaN into every dQ (both the one-kernel backward
    and, at S = 197, the phase split)."""
    B, H, scale = 2, 3, 0.7
    qkv, dout = _gpu_inputs(cuda, "negative", B, S, H)
    out, lse, dqkv = _fwd_bwd(qkv, dout, H, scale)
    ratios, ref = _bound_ratios(qkv, dout, H, scale, out, dqkv)
    assert ref[1].max().item() < -128
    assert torch.isfinite(dqkv.float()).all()
    for n, r in ratios.items():
        assert r <= FACTOR, f"S={S}: {n} error is {r:.3f} x its bound"
    assert _lse_excess(lse, ref[1], S)[0] <= 0


@pytest.mark.parametrize("B,H", [(1, 1), (3, 4)])
@pytest.mark.parametrize("S", [193, 197, 224])
def test_attention_bwd_phase_split_bitwise_at_every_7_tile_edge(cuda, S, B, H):
    """launch_attn_bwd splits whenever ceil(S / 32) == 7: one valid row in the last tile (193),
    ViT-B/16 (197) and no padding at all (224)."""
    C = ops.native()
    qkv, dout = _gpu_inputs(cuda, "gauss", B, S, H)
    out, lse = C.attn_fwd(qkv, H, 0.125)
    try:
        C.attn_set_bwd_split(0)
        one = C.attn_bwd(qkv, out, dout, lse, H, 0.125)
        C.attn_set_bwd_split(1)
        split = C.attn_bwd(qkv, out, dout, lse, H, 0.125)
    finally:
        C.attn_set_bwd_split(1)
    assert torch.equal(one, split)


def _equal3(a, b, S):
    """out, lse2 (the slots < S: the rest is at::empty and never written) and dqkv, bitwise."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1][:, :S], b[1][:, :S]) and torch.equal(a[2], b[2])


def test_attention_workgroups_are_independent(cuda):
    """One workgroup per (image, head), H not a power of two: each image alone, another image's
    data and the order of the heads change nothing, bitwise."""
    B, H, S, scale = 3, 3, 97, 0.125
    qkv, dout = _gpu_inputs(cuda, "gauss", B, S, H)
    full = _fwd_bwd(qkv, dout, H, scale)
    for b in range(B):
        alone = _fwd_bwd(qkv[b:b + 1].contiguous(), dout[b:b + 1].contiguous(), H, scale)
        assert torch.equal(alone[0], full[0][b:b + 1]), f"image {b} out"
        assert torch.equal(alone[1][:, :S], full[1][b * H:(b + 1) * H, :S]), f"image {b} lse2"
        assert torch.equal(alone[2], full[2][b:b + 1]), f"image {b} dqkv"
    other_q, other_d = _gpu_inputs(cuda, "peaked", 1, S, H, seed=99)
    qkv2, dout2 = qkv.clone(), dout.clone()
    qkv2[1], dout2[1] = other_q[0], other_d[0]
    changed = _fwd_bwd(qkv2, dout2, H, scale)
    assert not torch.equal(changed[0][1], full[0][1])
    for b in (0, 2):
        assert torch.equal(changed[0][b], full[0][b]), f"image {b} out"
        assert torch.equal(changed[1][b * H:(b + 1) * H, :S], full[1][b * H:(b + 1) * H, :S]), f"image {b} lse2"
        assert torch.equal(changed[2][b], full[2][b]), f"image {b} dqkv"
    perm = torch.tensor([2, 0, 1], device=cuda)
    qkv_p = qkv.view(B, S, 3, H, 64)[:, :, :, perm].reshape(B, S, 3 * H * 64).contiguous()
    dout_p = dout.view(B, S, H, 64)[:, :, perm].reshape(B, S, H * 64).contiguous()
    out_p, lse_p, dqkv_p = _fwd_bwd(qkv_p, dout_p, H, scale)
    assert torch.equal(out_p.view(B, S, H, 64), full[0].view(B, S, H, 64)[:, :, perm])
    assert torch.equal(lse_p.view(B, H, -1)[:, :, :S], full[1].view(B, H, -1)[:, perm, :S])
    assert torch.equal(dqkv_p.view(B, S, 3, H, 64), full[2].view(B, S, 3, H, 64)[:, :, :, perm])


@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("S", [97, 197])
def test_attention_is_run_to_run_bitwise_equal(cuda, S, split):
    """No atomics anywhere: the same inputs give the same bits."""
    C = ops.native()
    qkv, dout = _gpu_inputs(cuda, "gauss", 2, S, 3)
    try:
        C.attn_set_bwd_split(split)
        first = _fwd_bwd(qkv, dout, 3, 0.125)
        second = _fwd_bwd(qkv, dout, 3, 0.125)
    finally:
        C.attn_set_bwd_split(1)
    assert _equal3(first, second, S)


@pytest.mark.parametrize("S", [5, 33, 197])
def test_attention_bwd_never_reads_lse_padding(cuda, S):
    """lse2 is [B*H, ceil(S/32)*32] from at::empty and the forward writes only the slots < S."""
    C = ops.native()
    B, H = 2, 3
    qkv, dout = _gpu_inputs(cuda, "gauss", B, S, H)
    out, lse = C.attn_fwd(qkv, H, 0.125)
    assert lse.shape == (B * H, (S + 31) // 32 * 32)
    poisoned = lse.clone()
    poisoned[:, S:] = float("nan")
    clean = C.attn_bwd(qkv, out, dout, lse, H, 0.125)
    got = C.attn_bwd(qkv, out, dout, poisoned, H, 0.125)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, clean)


def test_attention_autograd_wrapper_strides_and_grad_dtypes(cuda):
    """fa.attention on a non-contiguous qkv, with a stride-0 grad_output (sum().backward()) and
    with an fp32 grad_output: each within the same bounds as the direct calls.  The fp32
    grad_output is rounded to bf16 by the wrapper; the reference gets that rounded value (the
    bounds are those of the kernel, whose operands are bf16)."""
    B, S, H, scale = 2, 97, 3, 0.125
    qkv, dout = _gpu_inputs(cuda, "gauss", B, S, H)
    d3 = 3 * H * 64

    def run(backward):
        wide = torch.zeros(B, S, d3 + 64, device=cuda, dtype=torch.bfloat16)
        wide[:, :, :d3] = qkv
        wide.requires_grad_(True)
        x = wide[:, :, :d3]
        assert not x.is_contiguous() and fa.supported(x, H)
        out = fa.attention(x, H)
        seen = backward(out)
        assert not wide.grad[:, :, d3:].any()
        return out.detach(), wide.grad[:, :, :d3].contiguous(), seen

    def explicit(out):
        out.backward(dout)
        return dout

    def summed(out):
        out.sum().backward()
        return torch.ones_like(dout)

    def squared_fp32(out):
        out.float().pow(2).sum().backward()
        return (2 * out.detach().float()).to(torch.bfloat16)

    for backward in (explicit, summed, squared_fp32):
        out, grad, seen = run(backward)
        ratios, _ = _bound_ratios(qkv, seen, H, scale, out, grad)
        for n, r in ratios.items():
            assert r <= FACTOR, f"{backward.__name__}: {n} error is {r:.3f} x its bound"


def test_attention_routing_and_argument_checks(cuda):
    C = ops.native()
    H = 2
    d3 = 3 * H * 64

    def z(*shape, dtype=torch.bfloat16):
        return torch.zeros(*shape, device=cuda, dtype=dtype)

    assert fa.supported(z(1, 5, d3), H) and fa.supported(z(1, 256, d3), H)
    assert not fa.supported(z(1, 0, d3), H)
    assert not fa.supported(z(1, 257, d3), H)
    assert not fa.supported(z(1, 5, d3, dtype=torch.float16), H)
    assert not fa.supported(z(5, d3), H)
    assert not fa.supported(z(1, 5, d3 + 8), H)
    fa.ENABLED = False
    try:
        assert not fa.supported(z(1, 5, d3), H)
    finally:
        fa.ENABLED = True
    for bad in (z(1, 257, d3), z(1, 5, d3, dtype=torch.float16), z(1, 5, 2 * d3)[:, :, ::2], z(1, 5, d3 + 8),
                z(1, 0, d3), z(5, d3)):
        with pytest.raises(RuntimeError):
            C.attn_fwd(bad, H, 0.125)
    # the backward rejects what the forward rejects (S > 256 would run attn_bwd_kernel<8> past its
    # LDS images); the lse of each call has the size the binding expects, so only that check fires
    with pytest.raises(RuntimeError, match="S <= 256"):
        C.attn_bwd(z(1, 257, d3), z(1, 257, H * 64), z(1, 257, H * 64), z(H, 288, dtype=torch.float32), H, 0.125)
    with pytest.raises(RuntimeError, match="qkv must be"):
        C.attn_bwd(z(5, d3), z(1, 5, H * 64), z(1, 5, H * 64), z(H, 32, dtype=torch.float32), H, 0.125)
    with pytest.raises(RuntimeError):
        C.attn_bwd(z(1, 5, d3), z(1, 5, H * 64), z(1, 5, H * 64), z(H, 64, dtype=torch.float32), H, 0.125)


def test_attention_empty_batch(cuda):
    """B = 0 returns empty, correctly shaped tensors without a launch (a zero-sized grid is an
    invalid configuration), and the next call is unaffected."""
    C = ops.native()
    S, H = 33, 3
    qkv0 = torch.zeros(0, S, 3 * H * 64, device=cuda, dtype=torch.bfloat16)
    out0, lse0 = C.attn_fwd(qkv0, H, 0.125)
    assert out0.shape == (0, S, H * 64) and out0.dtype == torch.bfloat16
    assert lse0.shape == (0, 64) and lse0.dtype == torch.float32
    dqkv0 = C.attn_bwd(qkv0, out0, torch.zeros_like(out0), lse0, H, 0.125)
    assert dqkv0.shape == (0, S, 3 * H * 64) and dqkv0.dtype == torch.bfloat16
    torch.cuda.synchronize()
    qkv, dout = _gpu_inputs(cuda, "gauss", 2, S, H)
    out, lse, dqkv = _fwd_bwd(qkv, dout, H, 0.125)
    ratios, ref = _bound_ratios(qkv, dout, H, 0.125, out, dqkv)
    assert max(ratios.values()) <= FACTOR, ratios
    assert _lse_excess(lse, ref[1], S)[0] <= 0
