"""The attention error bounds of tests/attention_oracle.py hold for an fp64 emulation of the
kernel's rounding points (no GPU): the bounds the GPU tests hold the kernel to are reachable by
the arithmetic the kernel states, and the data families do what they are for.

Run with ``-s`` to print the worst error / bound ratios per kind (the CPU-model column of
profiles/attention_error_bounds.md)."""
import math

import pytest
import torch

import attention_oracle as ao

B, H = 2, 3
LENGTHS = (1, 5, 31, 32, 33, 65, 97, 129, 161, 193, 197, 224, 225, 256)
SCALES = (0.125, 0.3)
_WORST = {}


@pytest.fixture(scope="module")
def worst():
    yield _WORST
    if _WORST:
        print("\nattention model vs fp64 reference, worst error / bound (lse2: worst abs error)")
        print(f"{'kind':10s} {'out':>7s} {'dQ':>7s} {'dK':>7s} {'dV':>7s} {'lse2':>9s}")
        for kind, w in _WORST.items():
            print(f"{kind:10s} {w['out']:7.3f} {w['dQ']:7.3f} {w['dK']:7.3f} {w['dV']:7.3f} {w['lse2']:9.2e}")


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("S", LENGTHS)
@pytest.mark.parametrize("kind", ["gauss", "peaked", "negative", "lastkey"])
def test_model_stays_inside_the_bounds(worst, kind, S, scale):
    qkv, dout = ao.inputs(kind, B, S, H, S * 7 + H)
    out_r, lse_r, dqkv_r, _ = ao.reference(qkv, dout, H, scale)
    out_m, lse_m, dqkv_m = ao.model(qkv, dout, H, scale)
    e_out, e_dq, e_dk, e_dv = ao.bounds(qkv, dout, H, scale)
    got = dict(zip(("dQ", "dK", "dV"), ao.split_dqkv(dqkv_m, H)), out=out_m)
    want = dict(zip(("dQ", "dK", "dV"), ao.split_dqkv(dqkv_r, H)), out=out_r)
    bound = {"out": e_out, "dQ": e_dq, "dK": e_dk, "dV": e_dv}
    ratios = {n: ao.worst_ratio(got[n], want[n], bound[n]) for n in bound}
    ratios["lse2"] = (lse_m - lse_r).abs().max().item()
    w = worst.setdefault(kind, dict.fromkeys(ratios, 0.0))
    for n, r in ratios.items():
        w[n] = max(w[n], r)
    for n in bound:
        assert ratios[n] <= 1.0, f"{kind} S={S} scale={scale}: {n} error is {ratios[n]:.3f} x its bound"
    assert ratios["lse2"] <= 1e-4, f"{kind} S={S} scale={scale}: lse2 off by {ratios['lse2']:.3e}"


@pytest.mark.parametrize("S", [33, 97, 197, 225])
def test_model_stays_inside_the_bounds_where_exp2_of_minus_lse_overflows(S):
    """`negative` at scale 0.7: lse2 < -128, the data of the GPU test of the backward's key mask."""
    qkv, dout = ao.inputs("negative", B, S, H, S * 7 + H)
    out_r, lse_r, dqkv_r, _ = ao.reference(qkv, dout, H, 0.7)
    out_m, lse_m, dqkv_m = ao.model(qkv, dout, H, 0.7)
    assert lse_r.max().item() < -128
    assert ao.worst_ratio(out_m, out_r, ao.bounds(qkv, dout, H, 0.7)[0]) <= 1.0
    for got, want, bound in zip(ao.split_dqkv(dqkv_m, H), ao.split_dqkv(dqkv_r, H), ao.bounds(qkv, dout, H, 0.7)[1:]):
        assert ao.worst_ratio(got, want, bound) <= 1.0
    assert (lse_m - lse_r).abs().max().item() <= 1e-4


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("S", LENGTHS)
def test_negative_scores_are_all_far_below_zero(S, scale):
    qkv, _ = ao.inputs("negative", B, S, H, S * 7 + H)
    q, k, _ = ao.split_heads(qkv.double(), H)
    assert ((q @ k.transpose(-1, -2)) * scale).max().item() < -10


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("S", LENGTHS)
def test_lastkey_dominates_every_row(S, scale):
    qkv, dout = ao.inputs("lastkey", B, S, H, S * 7 + H)
    p = ao.reference(qkv, dout, H, scale)[3]
    assert p[..., S - 1].min().item() > 0.9


@pytest.mark.parametrize("S", LENGTHS)
def test_uniform_counts_keys(S):
    qkv, dout = ao.inputs("uniform", B, S, H, S * 7 + H)
    out, lse2, _, p = ao.reference(qkv, dout, H, 0.125)
    assert (p - 1.0 / S).abs().max().item() <= 1e-12
    q, k, v = ao.split_heads(qkv.double(), H)
    torch.testing.assert_close(out, ao.merge_heads(v.mean(2, keepdim=True).expand_as(v)), rtol=0, atol=1e-12)
    s = (q * k[:, :, :1]).sum(-1) * 0.125
    torch.testing.assert_close(lse2, s * ao.LOG2E + math.log2(S), rtol=0, atol=1e-10)


def test_inputs_are_reproducible_bf16():
    for kind in ao.KINDS:
        a, da = ao.inputs(kind, 2, 33, 3, 11)
        b, db = ao.inputs(kind, 2, 33, 3, 11)
        assert a.dtype == da.dtype == torch.bfloat16
        assert a.shape == (2, 33, 3 * 3 * 64) and da.shape == (2, 33, 3 * 64)
        assert torch.equal(a, b) and torch.equal(da, db)
    with pytest.raises(ValueError):
        ao.inputs("nope", 1, 1, 1, 0)
