"""ConvNeXt block kernels (ops/convnext.py, csrc/kernels/cnx_kernels.hip), native against what
``DPT_NATIVE_CNBLOCK=0`` runs, on one MI355X:

1. the kernels alone at ConvNeXt-T's four stage shapes (batch 128, bf16): channel LayerNorm
   forward (16-bit rows, and fp32 rows as in front of a downsample) and backward, block tail
   forward and backward, against the ATen ops of the module-by-module path (``F.layer_norm`` with
   autocast's casts around it, ``x + layer_scale * (z + b2)`` and their autograd backward):
   median us per call, arms interleaved over rounds, and the TB/s of the bytes each pass must
   move next to the device copy rate;
2. the ConvNeXt-T training step (bf16 autocast, channels_last, batch 128, one Trainer, eager
   launches), ``ops.convnext.ENABLED`` on / off interleaved over rounds.

    python bench/cnblock_ab.py [--batch 128] [--rounds 5] [--no-step] > profiles/convnext_block.md
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

STAGES = ((96, 56), (192, 28), (384, 14), (768, 7))
COPY_TBS = 6.29  # the device copy rate the other profiles use (profiles/step_pmc_r5.md)
EPS = 1e-6


def _window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / reps


def _ab(fns, rounds, reps):
    for fn in fns:   # warm up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(ts, fns):
            t.append(_window(fn, reps))
    return [statistics.median(t) for t in ts]


def _ln_passes(C, T, c, dt, dev):
    """(name, native fn, stock fn, bytes) of the LayerNorm passes over [T, c] rows."""
    gamma, beta = torch.randn(c, device=dev), torch.randn(c, device=dev)
    gh = torch.randn(T, c, device=dev).to(dt)
    out = []
    for f32 in (False, True):
        y = torch.randn(T, c, device=dev).to(torch.float32 if f32 else dt)
        yb = 4 if f32 else 2
        _, mean, rstd = C.cnx_ln_fwd(y, gamma, beta, EPS, 1)
        yr = y.detach().clone().requires_grad_(True)
        gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        h_stock = F.layer_norm(yr.float(), (c,), gr, br, EPS).to(dt)   # autocast: fp32 LayerNorm, then the cast

        def stock_fwd(y=y):
            return F.layer_norm(y.float(), (c,), gamma, beta, EPS).to(dt)

        def stock_bwd(h=h_stock, ins=(yr, gr, br)):
            return torch.autograd.grad(h, ins, gh, retain_graph=True)

        tag = "fp32" if f32 else "bf16"
        out.append((f"LayerNorm forward ({tag} rows)", lambda y=y: C.cnx_ln_fwd(y, gamma, beta, EPS, 1), stock_fwd,
                    T * c * (yb + 2)))
        out.append((f"LayerNorm backward ({tag} rows)", lambda y=y, m=mean, r=rstd: C.cnx_ln_bwd(gh, y, m, r, gamma),
                    stock_bwd, T * c * (2 + yb + yb)))
    return out


def _tail_passes(C, T, c, dt, dev):
    x, dout = torch.randn(T, c, device=dev), torch.randn(T, c, device=dev)
    z = torch.randn(T, c, device=dev).to(dt)
    b2 = torch.randn(c, device=dev).to(dt)
    ls = torch.rand(c, device=dev) * 0.9 + 0.1
    zb = (z + b2).requires_grad_(True)       # stock: fc2 wrote z + b2 (the bias gradient is one more column sum)
    lr = ls.clone().requires_grad_(True)
    o_stock = x + lr * zb

    def stock_bwd():
        dzb, dls = torch.autograd.grad(o_stock, (zb, lr), dout, retain_graph=True)
        return dzb, dls, dzb.sum(0)

    return [("block tail forward", lambda: C.cnx_scale_residual_fwd(x, z, b2, ls), lambda: x + ls * zb.detach(),
             T * c * (4 + 2 + 4)),
            ("block tail backward", lambda: C.cnx_scale_residual_bwd(dout, z, b2, ls), stock_bwd, T * c * (4 + 2 + 2))]


def kernels_table(C, a, dev):
    dt = torch.bfloat16
    print(f"Median of {a.rounds} interleaved windows of {a.reps} calls; TB/s = bytes the pass must move / native time; "
          f"copy rate {COPY_TBS} TB/s.\n")
    print("| C | H | pass | native us | stock us | stock / native | native TB/s | % of copy rate |")
    print("|---|---|---|---|---|---|---|---|")
    for c, h in STAGES:
        T = a.batch * h * h
        for name, nf, sf, nbytes in _ln_passes(C, T, c, dt, dev) + _tail_passes(C, T, c, dt, dev):
            tn, ts = _ab((nf, sf), a.rounds, a.reps)
            tbs = nbytes / tn / 1e6
            print(f"| {c} | {h} | {name} | {tn:.1f} | {ts:.1f} | {ts / tn:.2f} | {tbs:.2f} | "
                  f"{100 * tbs / COPY_TBS:.0f} |", flush=True)


def step_ab(a, dev, model="convnext_tiny", title="ConvNeXt-T"):
    from distributed_pytorch_training_amd.config import parse_args
    from distributed_pytorch_training_amd.data import SyntheticLoader
    from distributed_pytorch_training_amd.engine.trainer import Trainer
    from distributed_pytorch_training_amd.models import build_model
    from distributed_pytorch_training_amd.ops import convnext as cnx
    from distributed_pytorch_training_amd.utils.env import setup_tunableop

    setup_tunableop()
    args = parse_args(["--model", model, "--dataset", "synthetic", "--batch-size", str(a.batch), "--amp",
                       "--amp-dtype", "bf16", "--channels-last", "--no-cuda-graph"])
    torch.manual_seed(0)
    tr = Trainer(build_model(model, 1000, dev, channels_last=True), args, 0, 1, dev, log=lambda s: None)
    batches = list(iter(SyntheticLoader(a.batch * 4, a.batch, 224, 1000, dev, channels_last=True, pool=4, seed=0)))

    def run(n):
        for i in range(n):
            tr.train_step(*batches[i % len(batches)])

    times = {True: [], False: []}
    for on in (True, False):
        cnx.ENABLED = on
        run(a.warmup)
    torch.cuda.synchronize()
    for rnd in range(a.rounds):
        for on in ((True, False) if rnd % 2 == 0 else (False, True)):
            cnx.ENABLED = on
            run(2)
            torch.cuda.synchronize()
            t0 = time.time()
            run(a.steps)
            torch.cuda.synchronize()
            times[on].append(1e3 * (time.time() - t0) / a.steps)
    cnx.ENABLED = True
    print(f"\n{title} step, batch {a.batch}, 224 px, bf16 autocast, channels_last, eager launches; median of "
          f"{a.rounds} interleaved windows of {a.steps} steps:\n")
    print("| DPT_NATIVE_CNBLOCK | ms / step | img/s | all windows (ms) |\n|---|---|---|---|")
    for on in (True, False):
        m = statistics.median(times[on])
        print(f"| {int(on)} | {m:.2f} | {a.batch * 1e3 / m:.0f} | {' '.join(f'{t:.2f}' for t in times[on])} |")


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
        raise SystemExit("bench/cnblock_ab.py measures on a GPU; none is visible")
    C = native()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    print(f"# ConvNeXt block kernels: native vs the ATen ops of DPT_NATIVE_CNBLOCK=0, batch {a.batch}, bf16\n")
    kernels_table(C, a, dev)
    if not a.no_step:
        step_ab(a, dev)


if __name__ == "__main__":
    main()
