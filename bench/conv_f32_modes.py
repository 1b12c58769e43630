"""fp32 convolution paths side by side: MIOpen fp32, the exact fp32 MFMA kernels and their
split-bf16 mode (csrc/kernels/conv_f32_kernels.hip), per conv shape (forward, input gradient,
weight gradient) and as the whole native fp32 training step.

    python bench/conv_f32_modes.py --model resnet50 --image 224 --batch 256 > bench_out/modes_r50.md
    python bench/conv_f32_modes.py --model resnet18 --image 32 --batch 128 > bench_out/modes_r18.md
    python bench/conv_f32_modes.py --steps 60 > bench_out/modes_step.md   # whole step, three ways

Per shape: every path is warmed up, then timed with device events over ``--iters`` calls in each
of ``--rounds`` rounds that alternate the three paths; the table shows the fastest round.  The
``x`` column is how often the shape occurs in the model; the totals weight by it.  Whole step:
``train_ddp.py --dataset synthetic --model resnet50 --batch-size 256 --max-steps N`` in a fresh
process per path, identical except for ``--fp32-conv``; the median throughput window after the
warm-up is reported.  ``train_ddp.py`` sets ``cudnn.benchmark`` as the reference does, so on a box
without a tuned MIOpen database the ``miopen`` run first spends minutes in MIOpen's find
(utils/env.py): it runs last and ``--step-timeout`` is sized for it.  Needs a GPU: there is no
CPU fall-back.
"""
from __future__ import annotations

import argparse
import os
import re
import statistics
import subprocess
import sys
from collections import OrderedDict

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model_convs(name: str, image: int, classes: int):
    """{(C, H, W, Co, k, stride, pad): count} of the model's convolutions at this image size."""
    from distributed_pytorch_training_amd.models import build_model

    m = build_model(name, classes, torch.device("cpu"), image_size=image).eval()
    shapes = OrderedDict()
    hooks = []

    def hook(mod, inp, out):
        c, h, w = inp[0].shape[1:]
        key = (c, h, w, mod.out_channels, mod.kernel_size[0], mod.stride[0], mod.padding[0])
        shapes[key] = shapes.get(key, 0) + 1

    for mod in m.modules():
        if isinstance(mod, torch.nn.Conv2d):
            hooks.append(mod.register_forward_hook(hook))
    with torch.no_grad():
        m(torch.zeros(1, 3, image, image))
    return shapes


def time_rounds(fns, iters: int, rounds: int):
    """Fastest round (ms per call) of each callable; the rounds alternate the callables."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    best = [float("inf")] * len(fns)
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                fn()
            end.record()
            torch.cuda.synchronize()
            best[i] = min(best[i], start.elapsed_time(end) / iters)
    return best


def per_shape(a) -> None:
    from distributed_pytorch_training_amd import ops
    from distributed_pytorch_training_amd.utils.env import setup_miopen_env

    setup_miopen_env()
    torch.backends.cudnn.benchmark = False
    C_ = ops.native()
    dev, cl = torch.device("cuda"), torch.channels_last
    print(f"# fp32 conv paths, {a.model} / {a.image} px / batch {a.batch}, channels_last, "
          f"{torch.cuda.get_device_name(0)}\n")
    print("ms per call (fastest of %d rounds of %d calls); TF/s of the split-bf16 kernels on the conv's "
          "2*M*N*K FLOPs\n" % (a.rounds, a.iters))
    print("| conv | x | pass | MIOpen | exact | split-bf16 | exact / split | MIOpen / split | split TF/s |")
    print("|---|---|---|---|---|---|---|---|---|")
    tot = {p: [0.0, 0.0, 0.0] for p in ("fwd", "dgrad", "wgrad")}
    for (c, h, w, co, k, st, pad), count in model_convs(a.model, a.image, a.classes).items():
        g = torch.Generator(device=dev).manual_seed(c + h + co + k)
        x = torch.randn(a.batch, c, h, w, device=dev, generator=g).contiguous(memory_format=cl)
        wt = (torch.randn(co, c, k, k, device=dev, generator=g) / (c * k * k) ** 0.5).contiguous(memory_format=cl)
        y = F.conv2d(x, wt, stride=st, padding=pad)
        gy = torch.randn(y.shape, device=dev, generator=g).contiguous(memory_format=cl)
        # the native kernels take 16-byte channel groups: the 3-channel stem is zero-padded to 4
        # (ops/conv_f32.py conv2d; the padding copies are part of a step, not of these timings)
        extra = (4 - c % 4) % 4
        xn = F.pad(x, (0, 0, 0, 0, 0, extra)).contiguous(memory_format=cl) if extra else x
        wn = F.pad(wt, (0, 0, 0, 0, 0, extra)).contiguous(memory_format=cl) if extra else wt
        flops = 2.0 * y.numel() * c * k * k
        name = f"{c}x{h}x{w}->{co} k{k} s{st}"
        sp, pp = (st, st), (pad, pad)

        def bwd(mask):
            return lambda: torch.ops.aten.convolution_backward(gy, x, wt, None, sp, pp, (1, 1), False, (0, 0), 1, mask)

        passes = [("fwd", [lambda: F.conv2d(x, wt, stride=st, padding=pad),
                           lambda: C_.conv_f32_fwd(xn, wn, st, pad),
                           lambda: C_.conv_f32_fwd(xn, wn, st, pad, split=True)])]
        if c > 3:   # the stem's input needs no gradient
            passes.append(("dgrad", [bwd((True, False, False)),
                                     lambda: C_.conv_f32_dgrad(gy, wn, st, pad, h, w),
                                     lambda: C_.conv_f32_dgrad(gy, wn, st, pad, h, w, split=True)]))
        passes.append(("wgrad", [bwd((False, True, False)),
                                 lambda: C_.conv_f32_wgrad(gy, xn, list(wn.shape), st, pad),
                                 lambda: C_.conv_f32_wgrad(gy, xn, list(wn.shape), st, pad, split=True)]))
        for pname, fns in passes:
            t = time_rounds(fns, a.iters, a.rounds)
            for i in range(3):
                tot[pname][i] += t[i] * count
            print(f"| {name} | {count} | {pname} | {t[0]:.3f} | {t[1]:.3f} | {t[2]:.3f} | {t[1] / t[2]:.2f} | "
                  f"{t[0] / t[2]:.2f} | {flops / t[2] / 1e9:.0f} |", flush=True)
        del x, wt, y, gy, xn, wn
    print("\n| pass, all convs of one step | MIOpen ms | exact ms | split-bf16 ms |")
    print("|---|---|---|---|")
    for pname, t in tot.items():
        print(f"| {pname} | {t[0]:.2f} | {t[1]:.2f} | {t[2]:.2f} |")
    s = [sum(t[i] for t in tot.values()) for i in range(3)]
    print(f"| sum | {s[0]:.2f} | {s[1]:.2f} | {s[2]:.2f} |")


def whole_step(a) -> None:
    print(f"# whole native fp32 step, {a.model} / {a.image} px / batch {a.batch}, 1 GPU\n")
    print("| --fp32-conv | samples/s (median window) | ms/step | windows |")
    print("|---|---|---|---|")
    for path in a.paths.split(","):
        cmd = [sys.executable, os.path.join(ROOT, "train_ddp.py"), "--dataset", "synthetic", "--model", a.model,
               "--batch-size", str(a.batch), "--image-size", str(a.image), "--num-classes", str(a.classes),
               "--epochs", "1", "--no-val", "--workers", "0", "--max-steps", str(a.steps),
               "--warmup-steps", str(a.warmup), "--print-freq", str(a.window),
               "--output-dir", os.path.join(a.out, "step_" + path), "--fp32-conv", path]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        thr = [float(v) for v in re.findall(r"Throughput: ([0-9.]+) samples/s", r.stdout)]
        if r.returncode != 0 or not thr:
            print(f"| {path} | failed (exit {r.returncode}) | - | - |", flush=True)
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            raise SystemExit(1)     # nothing more is started on the GPU after a failed run
        med = statistics.median(thr)
        print(f"| {path} | {med:.0f} | {1e3 * a.batch / med:.2f} | {' '.join(f'{v:.0f}' for v in thr)} |", flush=True)
    print("\ncommand: `" + " ".join(cmd[1:-1]).replace(ROOT + os.sep, "") + " {miopen,exact,split-bf16}`")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=0, help="> 0: time the whole step instead (train_ddp.py steps)")
    ap.add_argument("--paths", default="exact,split-bf16,miopen", help="--fp32-conv choices of the whole-step runs, in order")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds per train_ddp.py run")
    ap.add_argument("--out", default=os.path.join(ROOT, "bench_out", "conv_f32_modes"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("conv_f32_modes: needs a GPU")
    whole_step(a) if a.steps > 0 else per_shape(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
