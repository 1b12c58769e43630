"""Patchify convs with bias (ops/patchconv.py, csrc/kernels/patchconv_kernels.hip), native against
what ``DPT_NATIVE_PATCHCONV=0`` runs (``F.conv2d`` on MIOpen with autocast's cast of an fp32 stem
input), on one MI355X:

1. the three passes at the four patchify shapes of ConvNeXt-T and ConvNeXt-B (batch 128, bf16; the
   stem reads the fp32 image and has no backward-data): median us per call, arms interleaved over
   rounds;
2. the ConvNeXt-T training step (bf16 autocast, channels_last, batch 128, one Trainer, eager
   launches), ``ops.patchconv.ENABLED`` on / off interleaved over rounds.

    python bench/patchconv_ab.py [--batch 128] [--rounds 5] [--no-step] > profiles/patchconv.md
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (k, C, Cout, H) of the stem and the three downsamples
MODELS = {"ConvNeXt-T": ((4, 3, 96, 224), (2, 96, 192, 56), (2, 192, 384, 28), (2, 384, 768, 14)),
          "ConvNeXt-B": ((4, 3, 128, 224), (2, 128, 256, 56), (2, 256, 512, 28), (2, 512, 1024, 14))}


def _window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / reps


def _ab(fns, rounds, reps):
    for fn in fns:   # warm up: code objects, MIOpen's solver choice
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(ts, fns):
            t.append(_window(fn, reps))
    return [statistics.median(t) for t in ts]


def kernels_table(C, a, dev):
    dt, cl = torch.bfloat16, torch.channels_last
    print(f"Median of {a.rounds} interleaved windows of {a.reps} calls.\n")
    print("| model | k | C | Cout | H | pass | native us | stock us | stock / native |")
    print("|---|---|---|---|---|---|---|---|---|")
    for model, shapes in MODELS.items():
        for k, c, cout, h in shapes:
            x = torch.randn(a.batch, c, h, h, device=dev).to(torch.float32 if k == 4 else dt).contiguous(memory_format=cl)
            w = (torch.randn(cout, c, k, k, device=dev) / (k * k * c) ** 0.5).to(dt).contiguous(memory_format=cl)
            b = torch.randn(cout, device=dev).to(dt)
            dy = torch.randn(a.batch, cout, h // k, h // k, device=dev).to(dt).contiguous(memory_format=cl)

            def bwd(mask):
                return torch.ops.aten.convolution_backward(dy, x.to(dt), w, [cout], [k, k], [0, 0], [1, 1], False,
                                                           [0, 0], 1, mask)

            passes = [("forward", lambda: C.patchconv_fwd(x, w, b), lambda: F.conv2d(x.to(dt), w, b, k)),
                      ("backward-weight + bias", lambda: C.patchconv_wgrad(dy, x, k, 1),
                       lambda: bwd([False, True, True]))]
            if k == 2:
                passes.insert(1, ("backward-data", lambda: C.patchconv_dgrad(dy, w, h, h),
                                  lambda: bwd([True, False, False])))
            for name, nf, sf in passes:
                tn, ts = _ab((nf, sf), a.rounds, a.reps)
                print(f"| {model} | {k} | {c} | {cout} | {h} | {name} | {tn:.1f} | {ts:.1f} | {ts / tn:.2f} |",
                      flush=True)


def step_ab(a, dev):
    from distributed_pytorch_training_amd.config import parse_args
    from distributed_pytorch_training_amd.data import SyntheticLoader
    from distributed_pytorch_training_amd.engine.trainer import Trainer
    from distributed_pytorch_training_amd.models import build_model
    from distributed_pytorch_training_amd.ops import patchconv
    from distributed_pytorch_training_amd.utils.env import setup_tunableop

    setup_tunableop()
    args = parse_args(["--model", "convnext_tiny", "--dataset", "synthetic", "--batch-size", str(a.batch), "--amp",
                       "--amp-dtype", "bf16", "--channels-last", "--no-cuda-graph"])
    torch.manual_seed(0)
    tr = Trainer(build_model("convnext_tiny", 1000, dev, channels_last=True), args, 0, 1, dev, log=lambda s: None)
    batches = list(iter(SyntheticLoader(a.batch * 4, a.batch, 224, 1000, dev, channels_last=True, pool=4, seed=0)))

    def run(n):
        for i in range(n):
            tr.train_step(*batches[i % len(batches)])

    times = {True: [], False: []}
    for on in (True, False):
        patchconv.ENABLED = on
        run(a.warmup)
    torch.cuda.synchronize()
    for rnd in range(a.rounds):
        for on in ((True, False) if rnd % 2 == 0 else (False, True)):
            patchconv.ENABLED = on
            run(2)
            torch.cuda.synchronize()
            t0 = time.time()
            run(a.steps)
            torch.cuda.synchronize()
            times[on].append(1e3 * (time.time() - t0) / a.steps)
    patchconv.ENABLED = True
    print(f"\nConvNeXt-T step, batch {a.batch}, 224 px, bf16 autocast, channels_last, eager launches; median of "
          f"{a.rounds} interleaved windows of {a.steps} steps:\n")
    print("| DPT_NATIVE_PATCHCONV | ms / step | img/s | spread (ms) | all windows (ms) |\n|---|---|---|---|---|")
    for on in (True, False):
        m = statistics.median(times[on])
        print(f"| {int(on)} | {m:.2f} | {a.batch * 1e3 / m:.0f} | {max(times[on]) - min(times[on]):.2f} | "
              f"{' '.join(f'{t:.2f}' for t in times[on])} |")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args(argv)
    from distributed_pytorch_training_amd.ops import native
    from distributed_pytorch_training_amd.utils.env import setup_miopen_env
    setup_miopen_env()
    if not torch.cuda.is_available():
        raise SystemExit("bench/patchconv_ab.py measures on a GPU; none is visible")
    C = native()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    print(f"# Patchify convs with bias: native kernels vs F.conv2d (DPT_NATIVE_PATCHCONV=0), batch {a.batch}, bf16\n")
    kernels_table(C, a, dev)
    if not a.no_step:
        step_ab(a, dev)


if __name__ == "__main__":
    main()
