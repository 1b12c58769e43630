"""Per-launch rows of the seven block-tail backward applies and the seven conv3 backward-data launches
behind them (layer1.0 - layer2.3 of ResNet-50), or of the fused launches that replace them and the
backward-weight reduces that then run on their own (ops/conv.py TAIL_CONV3_BWD_FUSE), from the
rocprofv3 runs of ``bench/step_pmc.py``'s docstring, plus the step's totals (kernel time; HBM-side
bytes = 2 x FETCH_SIZE + WRITE_SIZE as in step_pmc.py).

    python bench/tail_conv3_bwd_rows.py --trace D/kt [--passes D/pB D/pC] > rows.md

A tail's apply is followed by conv3's backward-weight and then its backward-data: the first
``conv_fwd_kernel`` with the plain BNB epilogue after the apply.  The last seven such pairs of the step
are the one-tile shapes (the backward runs layer4 first).
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from step_pmc import load_pass, load_trace, short  # noqa: E402

APPLY = ("bn_bwd_apply_kernel<BF16,f,t,f>", "bn_bwd_apply2_kernel<BF16>")
# conv_fwd_kernel<128, BN, 1, LDSEPI, !BKN, !STATS, BNB, !BNR, ...>
DGRAD = ("conv_fwd_kernel<128,64,1,t,f,f,t,f,", "conv_fwd_kernel<128,128,1,t,f,f,t,f,")
FUSED = "tail_conv3_bwd_kernel"
REDUCE = "conv_wgrad_reduce_kernel"


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
        for k in fused:
            picks.append((k, "fused"))
            # conv3's backward-weight follows; its reduce is no longer carried by a backward-data launch
            nxt = next((j for j in range(k + 1, min(k + 4, len(names))) if names[j].startswith(REDUCE)), None)
            if nxt is not None:
                picks.append((nxt, "backward-weight reduce"))
    else:
        pairs = []
        for k, n in enumerate(names):
            if not n.startswith(APPLY):
                continue
            nxt = next((j for j in range(k + 1, min(k + 4, len(names))) if names[j].startswith(DGRAD)), None)
            if nxt is not None:
                pairs.append((k, nxt))
        for k, nxt in pairs[-7:]:
            picks.append((k, "tail backward apply"))
            picks.append((nxt, "conv3 backward-data"))

    def gb(c):
        return (2 * c.get("FETCH_SIZE", 0.0) + c.get("WRITE_SIZE", 0.0)) * 1024 / 1e9

    print("| # | what | kernel | us | read GB (2 x FETCH_SIZE) | write GB |")
    print("|---|---|---|---|---|---|")
    tot_us = tot_gb = tot_rd = 0.0
    for k, what in picks:
        c = ctr[k]
        us = trace[k][1]
        tot_us += us
        tot_gb += gb(c)
        tot_rd += 2 * c.get("FETCH_SIZE", 0.0) * 1024 / 1e9
        print(f"| {k} | {what} | `{names[k][:60]}` | {us:.1f} | {2 * c.get('FETCH_SIZE', 0.0) * 1024 / 1e9:.3f} | "
              f"{c.get('WRITE_SIZE', 0.0) * 1024 / 1e9:.3f} |")
    print(f"\n{len(picks)} launches: {tot_us:.1f} us, {tot_gb:.3f} GB (read {tot_rd:.3f})")
    print(f"step: {len(trace)} dispatches, kernel time {sum(u for _, u in trace) / 1e3:.3f} ms, "
          f"HBM-side bytes {sum(gb(c) for c in ctr):.2f} GB "
          f"(read {sum(2 * c.get('FETCH_SIZE', 0.0) for c in ctr) * 1024 / 1e9:.2f}, "
          f"write {sum(c.get('WRITE_SIZE', 0.0) for c in ctr) * 1024 / 1e9:.2f})")


if __name__ == "__main__":
    main()
