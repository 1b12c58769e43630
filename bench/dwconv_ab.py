"""Depthwise 7x7 conv, native kernels (ops/dwconv.py) against the ``F.conv2d`` path that
``DPT_NATIVE_DWCONV=0`` takes, at ConvNeXt-T's four stage shapes (batch 128, bf16 operands, fp32
and bf16 activations): median us per call of the three passes, arms interleaved over rounds, and
the TB/s of the bytes each pass must move (forward x + y, backward-data dy + dx, backward-weight
x + dy) next to the device's copy rate.  The stock arm includes what autocast and autograd add
around MIOpen for an fp32 x: the cast of x (forward, backward-weight) and the widening of dx.

    python bench/dwconv_ab.py [--batch 128] [--rounds 5] > profiles/dwconv.md
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ((96, 56), (192, 28), (384, 14), (768, 7))
COPY_TBS = 6.29  # the device copy rate the other profiles use (profiles/step_pmc_r5.md)


def _window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / reps


def _ab(native_fn, stock_fn, rounds, reps):
    for fn in (native_fn, stock_fn):   # warm up: code objects, MIOpen's solver choice
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(rounds):
        ts[0].append(_window(native_fn, reps))
        ts[1].append(_window(stock_fn, reps))
    return statistics.median(ts[0]), statistics.median(ts[1])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args(argv)
    from distributed_pytorch_training_amd.ops import native
    from distributed_pytorch_training_amd.utils.env import setup_miopen_env
    setup_miopen_env()
    C = native()
    dev = torch.device("cuda:0")
    dt, K, cl = torch.bfloat16, 7, torch.channels_last
    print(f"# Depthwise 7x7: native kernels vs F.conv2d (MIOpen), batch {a.batch}, bf16 operands\n")
    print(f"Median of {a.rounds} interleaved windows of {a.reps} calls; TB/s = bytes the pass must move / native "
          f"time; copy rate {COPY_TBS} TB/s.\n")
    print("| C | H | x | pass | native us | stock us | stock / native | native TB/s | % of copy rate |")
    print("|---|---|---|---|---|---|---|---|---|")
    for c, h in STAGES:
        for act in (torch.float32, dt):
            x = torch.randn(a.batch, c, h, h, device=dev).to(act).contiguous(memory_format=cl)
            dy = torch.randn(a.batch, c, h, h, device=dev).to(dt).contiguous(memory_format=cl)
            w = (torch.randn(c, 1, K, K, device=dev) / K).to(dt)
            b = torch.randn(c, device=dev).to(dt)
            f32 = act == torch.float32

            x16_keep = x.to(dt)   # backward-data does not read x: no cast charged to it

            def bwd(mask):
                x16 = x.to(dt) if mask[1] else x16_keep
                g = torch.ops.aten.convolution_backward(dy, x16, w, [c], [1, 1], [3, 3], [1, 1], False, [0, 0], c, mask)
                return g[0].float() if (f32 and mask[0]) else g

            n_el = x.numel()
            xb = 4 if f32 else 2
            passes = (
                ("forward", lambda: C.dwconv_fwd(x, w, b),
                 lambda: torch.nn.functional.conv2d(x.to(dt), w, b, 1, 3, 1, c), n_el * (xb + 2)),
                ("backward-data", lambda: C.dwconv_dgrad(dy, w, f32), lambda: bwd([True, False, False]), n_el * (2 + xb)),
                ("backward-weight", lambda: C.dwconv_wgrad(dy, x, K, 1), lambda: bwd([False, True, True]),
                 n_el * (xb + 2)),
            )
            for name, nf, sf, nbytes in passes:
                tn, ts = _ab(nf, sf, a.rounds, a.reps)
                tbs = nbytes / tn / 1e6
                print(f"| {c} | {h} | {'fp32' if f32 else 'bf16'} | {name} | {tn:.1f} | {ts:.1f} | {ts / tn:.2f} | "
                      f"{tbs:.2f} | {100 * tbs / COPY_TBS:.0f} |", flush=True)


if __name__ == "__main__":
    main()
