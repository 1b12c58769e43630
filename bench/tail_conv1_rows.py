"""Per-launch rows of the six block-tail applies and the six 1x1 conv1 forwards they feed (layer1.0 -
layer2.2 tails of ResNet-50), or of the six fused launches that replace them (ops/bn.py
TAIL_CONV1_FUSE), from the rocprofv3 runs of ``bench/step_pmc.py``'s docstring, plus the step's
totals (kernel time; HBM-side bytes = 2 x FETCH_SIZE + WRITE_SIZE as in step_pmc.py).

    python bench/tail_conv1_rows.py --trace D/kt [--passes D/pB D/pC] > rows.md
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from step_pmc import load_pass, load_trace, short  # noqa: E402

TAIL = ("bn_fwd_apply_kernel<BF16,t,t,f>", "bn_fwd_apply_kernel<BF16,t,t,t>")
FUSED = "tail_conv1_fwd_kernel"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", required=True)
    ap.add_argument("--passes", nargs="*", default=[])
    a = ap.parse_args(argv)
    trace = load_trace(a.trace)
    ctr = [dict() for _ in trace]
    for d in a.passes:
        p = load_pass(d)
        if len(p) != len(trace):
            raise SystemExit(f"{d}: {len(p)} dispatches in the last step vs {len(trace)} in the trace")
        for k, (n, c) in enumerate(p):
            if short(n) != short(trace[k][0]):
                raise SystemExit(f"{d}: dispatch {k} differs from the trace")
            ctr[k].update(c)
    names = [short(n) for n, _ in trace]
    picks = []
    fused = [k for k, n in enumerate(names) if n.startswith(FUSED)]
    if fused:
        picks = [(k, "fused") for k in fused]
    else:
        tails = [k for k, n in enumerate(names) if n.startswith(TAIL)][:6]
        for k in tails:
            picks.append((k, "tail apply"))
            nxt = next(j for j in range(k + 1, len(names)) if names[j].startswith("conv_fwd_kernel"))
            picks.append((nxt, "conv1 forward"))

    def gb(c):
        return (2 * c.get("FETCH_SIZE", 0.0) + c.get("WRITE_SIZE", 0.0)) * 1024 / 1e9

    print("| # | what | kernel | us | read GB (2 x FETCH_SIZE) | write GB |")
    print("|---|---|---|---|---|---|")
    tot_us = tot_gb = 0.0
    for k, what in picks:
        c = ctr[k]
        us = trace[k][1]
        tot_us += us
        tot_gb += gb(c)
        print(f"| {k} | {what} | `{names[k][:60]}` | {us:.1f} | {2 * c.get('FETCH_SIZE', 0.0) * 1024 / 1e9:.3f} | "
              f"{c.get('WRITE_SIZE', 0.0) * 1024 / 1e9:.3f} |")
    print(f"\n{len(picks)} launches: {tot_us:.1f} us, {tot_gb:.3f} GB")
    print(f"step: {len(trace)} dispatches, kernel time {sum(u for _, u in trace) / 1e3:.3f} ms, "
          f"HBM-side bytes {sum(gb(c) for c in ctr):.2f} GB "
          f"(read {sum(2 * c.get('FETCH_SIZE', 0.0) for c in ctr) * 1024 / 1e9:.2f}, "
          f"write {sum(c.get('WRITE_SIZE', 0.0) for c in ctr) * 1024 / 1e9:.2f})")


if __name__ == "__main__":
    main()
