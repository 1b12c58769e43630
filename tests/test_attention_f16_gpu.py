"""The fp16 instantiations of the attention kernels (csrc/kernels/attn_f16_kernels.hip) against the
fp64 reference of tests/attention_oracle.py computed from the fp16 inputs.

bound16 = ao.bounds * (u16 + S 2^-24) / 2^-8 + eta (1 + c): the oracle's first-order bound is
linear in its unit round-off 2^-8, so the ratio moves it to fp16's u16 = 2^-11 and adds the
fp32-accumulation term; eta = 2^-25 is the rounding of a subnormal fp16 operand (P or dS below
2^-14), times the sum c of what that operand multiplies.  Run with -s for the ratios
(profiles/attention_f16_error_bounds.md)."""
import copy

import pytest
import torch

import attention_oracle as ao
from distributed_pytorch_training_amd import ops
from distributed_pytorch_training_amd.ops import attention as fa

pytestmark = pytest.mark.gpu

FACTOR = 1.25     # over the first-order bound: second-order terms, v_exp_f32
U16, ETA = 2.0 ** -11, 2.0 ** -25
NAMES = ("out", "dQ", "dK", "dV")


def _fwd_bwd(family, qkv, dout, H, scale):
    C = ops.native()
    fwd, bwd = (C.attn_fwd_f16, C.attn_bwd_f16) if family == "onchip" else (C.attn_stream_fwd_f16, C.attn_stream_bwd_f16)
    out, lse = fwd(qkv, H, scale)
    return out, lse, bwd(qkv, out, dout, lse, H, scale)


def _ratios(qkv, dout, H, scale, out, dqkv):
    """Worst |kernel - fp64 reference| / bound16 for out, dQ, dK, dV, and the reference's lse2."""
    S = qkv.shape[1]
    ref_out, lse2, ref_dqkv, _ = ao.reference(qkv, dout, H, scale)
    q, k, v = (ao.merge_heads(t.double().abs().sum(2, keepdim=True).expand_as(t)) for t in ao.split_heads(qkv, H))
    c = (v, scale * k, scale * q, dout.double().abs().sum(1, keepdim=True).expand_as(dout))
    rel = (U16 + S * 2.0 ** -24) / ao.U
    got, want = (out, *ao.split_dqkv(dqkv, H)), (ref_out, *ao.split_dqkv(ref_dqkv, H))
    bound = [e * rel + ETA * (1 + ci) for e, ci in zip(ao.bounds(qkv, dout, H, scale), c)]
    return {n: ao.worst_ratio(g, w, b) for n, g, w, b in zip(NAMES, got, want, bound)}, lse2


def _inputs(cuda, kind, B, S, H):
    return tuple(t.to(cuda).half() for t in ao.inputs(kind, B, S, H, S * 7 + H))


# on chip: one tile, one past a tile edge, the 7-tile two-launch split, the largest (PHASE 0);
# streaming: one key in the last chunk, an exact multiple of the 128 tile, ViT at 384 px
@pytest.mark.parametrize("kind", ["gauss", "peaked", "lastkey"])
@pytest.mark.parametrize("family,S", [("onchip", s) for s in (5, 33, 197, 256)] + [("stream", s) for s in (257, 384, 577)])
def test_f16_within_rounding_bounds(cuda, family, S, kind):
    B, H, scale = 2, 3, 0.125
    qkv, dout = _inputs(cuda, kind, B, S, H)
    out, lse, dqkv = _fwd_bwd(family, qkv, dout, H, scale)
    assert out.dtype == dqkv.dtype == torch.float16 and lse.dtype == torch.float32
    ratios, lse2 = _ratios(qkv, dout, H, scale, out, dqkv)
    want = lse2.reshape(-1, S)
    lse_err = (lse[:, :S].double() - want).abs()
    print(f"\n{family} {kind} S={S}: " + " ".join(f"{n} {r:.3f}" for n, r in ratios.items())
          + f" lse2 {lse_err.max().item():.2e}", end="")
    for n, r in ratios.items():
        assert r <= FACTOR, f"{family} {kind} S={S}: {n} error is {r:.3f} x its bound"
    assert (lse_err <= 1e-3 + 1e-5 * want.abs()).all()
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all()


@pytest.mark.parametrize("family,S", [("onchip", 33), ("stream", 257)])
def test_f16_overflow_reaches_the_gradient_as_inf(cuda, family, S):
    """Every dO element 30000 and p > 0.9 on key S-1 for every query: dV[S-1] > 0.9 * S * 30000 does
    not fit fp16 and must come back +inf (a saturating conversion gives 65504); out stays finite."""
    B, H = 1, 2
    qkv = _inputs(cuda, "lastkey", B, S, H)[0]
    dout = torch.full((B, S, H * 64), 30000.0, device=cuda, dtype=torch.float16)
    out, _, dqkv = _fwd_bwd(family, qkv, dout, H, 0.125)
    assert ao.reference(qkv, dout, H, 0.125)[3][..., S - 1].min().item() > 0.9
    assert torch.isfinite(out).all()
    assert (ao.split_dqkv(dqkv, H)[2][:, S - 1] == float("inf")).all()


def test_f16_routing(cuda, monkeypatch):
    H, d3 = 2, 3 * 2 * 64

    def z(s, dtype=torch.float16, device=cuda):
        return torch.zeros(1, s, d3, device=device, dtype=dtype)

    for pred, good, bad, switch in ((fa.supported_f16, (5, 256), (0, 257), "ENABLED"),
                                    (fa.supported_streaming_f16, (257, 4096), (256, 4097), "STREAMING")):
        assert all(pred(z(s), H) for s in good)
        assert not any(pred(z(s), H) for s in bad)
        assert not pred(z(good[0], dtype=torch.bfloat16), H) and not pred(z(good[0], device="cpu"), H)
        for name in {"ENABLED", switch}:
            with monkeypatch.context() as mp:
                mp.setattr(fa, name, False)
                assert not pred(z(good[0]), H)


@pytest.mark.parametrize("S", [97, 290])
def test_f16_autograd_wrapper_strides_and_grad_dtype(cuda, S):
    """fa.attention on a non-contiguous fp16 qkv with an fp32 grad_output, which the wrapper rounds
    to fp16 (the reference gets the rounded value): fp16 out and gradient, both within the bounds."""
    B, H, scale = 2, 3, 0.125
    qkv, _ = _inputs(cuda, "gauss", B, S, H)
    d3 = 3 * H * 64
    wide = torch.zeros(B, S, d3 + 64, device=cuda, dtype=torch.float16)
    wide[:, :, :d3] = qkv
    wide.requires_grad_(True)
    x = wide[:, :, :d3]
    assert not x.is_contiguous() and (fa.supported_f16(x, H) or fa.supported_streaming_f16(x, H))
    out = fa.attention(x, H)
    out.float().pow(2).sum().backward()
    assert out.dtype == wide.grad.dtype == torch.float16 and not wide.grad[:, :, d3:].any()
    seen = (2 * out.detach().float()).half()
    ratios, _ = _ratios(qkv, seen, H, scale, out.detach(), wide.grad[:, :, :d3].contiguous())
    assert max(ratios.values()) <= FACTOR, ratios


@pytest.mark.parametrize("family,S", [("onchip", 33), ("stream", 290)])
def test_f16_empty_batch(cuda, family, S):
    H = 3
    qkv0 = torch.zeros(0, S, 3 * H * 64, device=cuda, dtype=torch.float16)
    out0, lse0, dqkv0 = _fwd_bwd(family, qkv0, torch.zeros(0, S, H * 64, device=cuda, dtype=torch.float16), H, 0.125)
    assert out0.shape == (0, S, H * 64) and out0.dtype == torch.float16
    assert lse0.shape == (0, (S + 31) // 32 * 32) and lse0.dtype == torch.float32
    assert dqkv0.shape == (0, S, 3 * H * 64) and dqkv0.dtype == torch.float16


@pytest.mark.parametrize("tokens,binding", [(197, "attn_fwd_f16"), (290, "attn_stream_fwd_f16")])
def test_vit_block_uses_f16_attention(cuda, monkeypatch, tokens, binding):
    """A native ViT-B/16 self-attention block under fp16 autocast calls the fp16 binding and agrees
    with the stock (SDPA) block of the same weights within test_vit_uses_fused_attention's bf16
    tolerance scaled by u16 / 2^-8."""
    from distributed_pytorch_training_amd.models.vit import SelfAttention, set_native

    C = ops.native()
    calls, real = [], getattr(C, binding)
    monkeypatch.setattr(C, binding, lambda *a: calls.append(1) or real(*a))
    torch.manual_seed(tokens)
    stock = SelfAttention(768, 12).to(cuda).train()
    native_block = copy.deepcopy(stock)
    assert set_native(native_block) == 1
    x = torch.randn(2 if tokens == 197 else 1, tokens, 768, device=cuda)
    with torch.autocast("cuda", dtype=torch.float16):
        y, want = native_block(x), stock(x)
    assert len(calls) == 1 and y.dtype == torch.float16
    tol = 5e-2 * U16 / ao.U
    torch.testing.assert_close(y.float(), want.float(), rtol=tol, atol=tol)
