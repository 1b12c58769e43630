"""GELU + Global Response Normalization (ops/convnext.py gelu_grn16, csrc/kernels/grn_kernels.hip)
against the PyTorch composition under autocast, on one MI355X:

1. forward and backward at ConvNeXt V2-T's four stage shapes (batch 128, bf16: H*W = 3136 / 784 /
   196 / 49 rows per sample, D = 384 / 768 / 1536 / 3072).  The stock arm is what the module-by-module
   block runs between fc1 and fc2 under autocast: GELU on fc1's 16-bit output (bias already added by
   the GEMM), the GRN module (its norm and everything after it in fp32), the cast to fc2's operand
   type, and in the backward autograd's kernels plus the bias gradient's column sum.  Median, min and
   max us per call over interleaved windows, and the TB/s of the bytes the native sweeps move (forward:
   u twice, g once = 6 B / element; backward: dg and u twice, du once = 10 B / element);
2. the ConvNeXt V2-T training step (bf16 autocast, channels_last, batch 128, eager launches) with the
   native block route (``ops.convnext.ENABLED``) on / off, interleaved over rounds.

    python bench/grn_ab.py [--batch 128] [--rounds 7] [--no-step] > profiles/convnext_v2_grn.md

Per-kernel times come from a kernel trace of the native arm alone, in a run of its own:

    rocprofv3 --kernel-trace -d <dir> -o run -- python bench/grn_ab.py --native-only
    python bench/grn_ab.py --trace <dir>/.../run_results.db      # or run_kernel_trace.csv
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench.cnblock_ab import COPY_TBS, _window, step_ab  # noqa: E402

STAGES = ((384, 56), (768, 28), (1536, 14), (3072, 7))   # (D = 4 dim, H = W)
# bytes per element each sweep must move (16-bit u, dg, g, du)
SWEEP_BYTES = {"grn_fwd_stats": 2, "grn_fwd_apply": 4, "grn_bwd_stats": 4, "grn_bwd_apply": 6}


def _ab(fns, rounds, reps):
    for fn in fns:   # warm up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for rnd in range(rounds):
        for i in (range(len(fns)) if rnd % 2 == 0 else reversed(range(len(fns)))):
            ts[i].append(_window(fns[i], reps))
    return ts


def _passes(C, N, R, D, dt, dev):
    """[(name, native fn, stock fn, bytes)] for forward and backward over u [N, R, D]."""
    from distributed_pytorch_training_amd.models.convnext import GRN

    h = int(R ** 0.5)
    u = (torch.randn(N, R, D, device=dev) * 1.5).to(dt)
    dg = torch.randn(N, R, D, device=dev).to(dt)
    b1 = (torch.randn(D, device=dev) * 0.5).to(dt)
    gamma, beta = torch.randn(D, device=dev), torch.randn(D, device=dev)
    _, G, inv, s = C.cnx_grn_fwd(u, b1, gamma, beta, R, 1e-6)
    grn = GRN(D).to(dev)
    with torch.no_grad():
        grn.gamma.copy_(gamma.view(1, 1, 1, D))
        grn.beta.copy_(beta.view(1, 1, 1, D))
    ub = (u + b1).view(N, h, h, D).requires_grad_(True)    # stock: fc1's GEMM wrote u + b1
    dg4 = dg.view(N, h, h, D)

    def stock_fwd(x=ub):
        with torch.autocast("cuda", dtype=dt):
            return grn(F.gelu(x)).to(dt)

    g_stock = stock_fwd()

    def stock_bwd():
        dub, dga, dbe = torch.autograd.grad(g_stock, (ub, grn.gamma, grn.beta), dg4, retain_graph=True)
        return dub, dub.sum((0, 1, 2)), dga, dbe

    def stock_fwd_nograd():
        with torch.no_grad():
            return stock_fwd(ub.detach())

    n = N * R * D
    return [("forward", lambda: C.cnx_grn_fwd(u, b1, gamma, beta, R, 1e-6), stock_fwd_nograd, 6 * n),
            ("backward", lambda: C.cnx_grn_bwd(dg, u, b1, gamma, G, inv, s, R), stock_bwd, 10 * n)]


def kernels_table(C, a, dev):
    dt = torch.bfloat16
    print(f"Median (min-max) of {a.rounds} interleaved windows of {a.reps} calls; TB/s = bytes the native sweeps move "
          f"/ native time; copy rate {COPY_TBS} TB/s.\n")
    print("| D | H*W | pass | native us | stock us | stock / native | native TB/s | % of copy rate |")
    print("|---|---|---|---|---|---|---|---|")
    for D, h in STAGES:
        for name, nf, sf, nbytes in _passes(C, a.batch, h * h, D, dt, dev):
            tn, ts = _ab((nf, sf), a.rounds, a.reps)
            mn, ms = statistics.median(tn), statistics.median(ts)
            tbs = nbytes / mn / 1e6
            print(f"| {D} | {h * h} | {name} | {mn:.1f} ({min(tn):.1f}-{max(tn):.1f}) | {ms:.1f} ({min(ts):.1f}-"
                  f"{max(ts):.1f}) | {ms / mn:.2f} | {tbs:.2f} | {100 * tbs / COPY_TBS:.0f} |", flush=True)
        torch.cuda.empty_cache()


def native_only(C, a, dev):
    for D, h in STAGES:
        for _, nf, _, _ in _passes(C, a.batch, h * h, D, torch.bfloat16, dev):
            for _ in range(a.reps):
                nf()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def trace_table(a):
    """Per-kernel medians from a rocprofv3 kernel trace of --native-only, which runs the stages in
    order with the same number of calls each: the dispatches of a kernel split evenly over them."""
    from bench.rocprof_rows import load_rows

    rows = load_rows(a.trace)
    print(f"\nPer-kernel medians over a kernel trace of the native arm (batch {a.batch}, bf16); TB/s = bytes the sweep "
          f"must move / kernel time; copy rate {COPY_TBS} TB/s.\n")
    print("| D | H*W | kernel | calls | median us | TB/s | % of copy rate |\n|---|---|---|---|---|---|---|")
    for name in ("grn_fwd_stats", "grn_fwd_finalize", "grn_fwd_apply", "grn_bwd_stats", "grn_bwd_finalize",
                 "grn_bwd_apply"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        per = len(us) // len(STAGES)
        for i, (D, h) in enumerate(STAGES):
            m = statistics.median(us[i * per:(i + 1) * per])
            rate = ""
            if name in SWEEP_BYTES:
                tbs = SWEEP_BYTES[name] * a.batch * h * h * D / m / 1e6
                rate = f"{tbs:.2f} | {100 * tbs / COPY_TBS:.0f}"
            print(f"| {D} | {h * h} | {name} | {per} | {m:.1f} | {rate or ' | '} |")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--native-only", action="store_true", help="run the native arm alone (for a kernel trace)")
    ap.add_argument("--trace", default=None, help="print the per-kernel table from this rocprofv3 kernel trace")
    a = ap.parse_args(argv)
    from distributed_pytorch_training_amd.ops import native
    from distributed_pytorch_training_amd.utils.env import setup_miopen_env
    if a.trace:
        return trace_table(a)
    setup_miopen_env()
    if not torch.cuda.is_available():
        raise SystemExit("bench/grn_ab.py measures on a GPU; none is visible")
    C = native()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if a.native_only:
        return native_only(C, a, dev)
    print(f"# GELU + GRN: native gelu_grn16 vs the PyTorch composition under autocast, batch {a.batch}, bf16\n")
    kernels_table(C, a, dev)
    if not a.no_step:
        step_ab(a, dev, "convnextv2_tiny", "ConvNeXt V2-T")


if __name__ == "__main__":
    main()
