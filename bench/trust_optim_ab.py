"""Isolated optimizer-step time of the fused LARS / LAMB steps over the ResNet-50 and ViT-B/16
arenas, against the per-tensor stock classes (optim/stock.py) and with FusedSGD / FusedAdam as the
floor.

hipEvents around ``--inner`` back-to-back steps, the variants interleaved round after round (so a
slow minute on a shared host hits every variant alike), median and spread over ``--repeats``
rounds, after ``--warmup`` untimed steps of every variant.  The fused steps zero the gradients
they consume, so every timed step after the first sees zero gradients: the bytes moved are the
same, and no kernel branches on the data.  Bytes per parameter are the passes' reads and writes
(csrc/kernels/trust_kernels.hip); TB/s is that model over the measured time, not a counter.

    python bench/trust_optim_ab.py [--models resnet50,vit_b_16] [--out profiles/trust_optim.md]
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES = {"FusedSGD": 24, "FusedAdam": 32, "FusedLARS": 8 + 24, "FusedLAMB": 28 + 16}


def _variants(model, dev):
    from distributed_pytorch_training_amd.optim import (LAMB, LARS, FusedAdam, FusedLAMB, FusedLARS,
                                                        FusedSGD)
    from distributed_pytorch_training_amd.parallel.flat import FlatArena

    def fused(cls, **kw):
        params = [p for p in copy.deepcopy(model).parameters() if p.requires_grad]
        arena = FlatArena(params)
        g = torch.Generator(device=dev).manual_seed(1)
        for v in arena.views(arena.grad_flat):
            v.copy_(torch.randn(v.shape, device=dev, generator=g) * 0.01)
        opt = cls(arena, **kw)
        return (lambda: opt.step()), arena.numel

    def stock(cls, **kw):
        params = [p for p in copy.deepcopy(model).parameters() if p.requires_grad]
        g = torch.Generator(device=dev).manual_seed(1)
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 0.01
        opt = cls(params, **kw)
        return (lambda: opt.step()), sum(p.numel() for p in params)

    lr = 1e-6      # hundreds of steps on fixed gradients: keep the weights where they are
    return {
        "FusedSGD": fused(FusedSGD, lr=lr, momentum=0.9, weight_decay=5e-4),
        "FusedAdam": fused(FusedAdam, lr=lr, weight_decay=1e-2, adamw=True),
        "FusedLARS": fused(FusedLARS, lr=lr, momentum=0.9, weight_decay=5e-4),
        "FusedLAMB": fused(FusedLAMB, lr=lr, weight_decay=1e-2),
        "stock LARS (per tensor)": stock(LARS, lr=lr, momentum=0.9, weight_decay=5e-4),
        "stock LAMB (per tensor)": stock(LAMB, lr=lr, weight_decay=1e-2),
    }


def measure(model_name: str, dev, warmup: int, inner: int, repeats: int):
    from distributed_pytorch_training_amd.models import build_model
    torch.manual_seed(0)
    image = 224
    model = build_model(model_name, 1000, dev, image_size=image)
    variants = _variants(model, dev)
    ntensors = sum(1 for p in model.parameters() if p.requires_grad)
    del model
    for fn, _ in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for name, (fn, _) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1000.0 / inner)
    rows = []
    for name, (fn, numel) in variants.items():
        ts = sorted(times[name])
        med = statistics.median(ts)
        row = {"model": model_name, "tensors": ntensors, "variant": name, "elements": numel,
               "us_median": round(med, 1), "us_min": round(ts[0], 1), "us_max": round(ts[-1], 1)}
        if name in BYTES:
            row["bytes_per_param"] = BYTES[name]
            row["model_tb_per_s"] = round(BYTES[name] * numel / med / 1e6, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def to_markdown(rows, warmup, inner, repeats) -> str:
    out = ["# Fused LARS / LAMB: isolated optimizer step", "",
           f"`python bench/trust_optim_ab.py` on one MI355X: hipEvents around {inner} back-to-back steps, "
           f"variants interleaved, median (min - max) over {repeats} rounds after {warmup} warm-up steps. "
           "Eager launches, no hipGraph; the host's launch cost is inside every figure. B/param and TB/s "
           "are the passes' modelled reads and writes over the measured time, not a counter.", "",
           "| model | variant | us / step (min - max) | B/param | modelled TB/s | vs FusedSGD |",
           "|---|---|---|---|---|---|"]
    for model in dict.fromkeys(r["model"] for r in rows):
        mine = [r for r in rows if r["model"] == model]
        floor = next(r["us_median"] for r in mine if r["variant"] == "FusedSGD")
        for r in mine:
            out.append(f"| {model} ({r['tensors']} tensors, {r['elements'] / 1e6:.1f} M) | {r['variant']} | "
                       f"{r['us_median']} ({r['us_min']} - {r['us_max']}) | {r.get('bytes_per_param', '-')} | "
                       f"{r.get('model_tb_per_s', '-')} | {r['us_median'] / floor:.2f}x |")
    return "\n".join(out) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="resnet50,vit_b_16")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--out", default=None, help="write the markdown table here")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("trust_optim_ab.py times GPU kernels: no GPU found")
    dev = torch.device("cuda:0")
    rows = []
    for m in a.models.split(","):
        rows += measure(m, dev, a.warmup, a.inner, a.repeats)
    md = to_markdown(rows, a.warmup, a.inner, a.repeats)
    print(md)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(md)


if __name__ == "__main__":
    main()
