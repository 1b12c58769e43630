"""Self-attention forward + backward above 256 tokens: the streaming kernels (fa.attention ->
attn_stream_fwd / attn_stream_bwd) vs the fallback they replace (split_heads + scaled_dot_product_
attention + merge_heads), at ViT-B/16 shapes of 288, 384 and 512 px.

    python bench/attn_stream_ab.py [--rounds 20] [--iters 10] [--out profiles/attn_stream_ab.json]

Each shape is timed in a child process of its own under ``timeout``; the arms alternate round by
round after a warm-up of both, a round is ``iters`` forward+backward calls between two device
events, and the table reports the median round (min - max) per call.  A shape whose child fails
ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = 12
SHAPES = ((64, 577), (32, 1025), (128, 325))   # (batch, tokens): 384, 512 and 288 px


def one(B, S, rounds, iters):
    import torch
    import torch.nn.functional as F

    from distributed_pytorch_training_amd import ops
    from distributed_pytorch_training_amd.ops import attention as fa
    from distributed_pytorch_training_amd.ops.vit import merge_heads, split_heads

    ops.native()
    fa.ENABLED = fa.STREAMING = True
    torch.manual_seed(0)
    qkv = torch.randn(B, S, 3 * H * 64, device="cuda").to(torch.bfloat16).requires_grad_(True)
    dout = torch.randn(B, S, H * 64, device="cuda").to(torch.bfloat16)
    assert fa.supported_streaming(qkv, H)

    def streaming():
        return fa.attention(qkv, H)

    def fallback():
        q, k, v = split_heads(qkv, H)
        return merge_heads(F.scaled_dot_product_attention(q, k, v))

    def step(fn):
        qkv.grad = None
        out = fn()
        out.backward(dout)
        return out

    arms = {"streaming": streaming, "fallback": fallback}
    outs = {}
    for name, fn in arms.items():          # warm-up: code objects, SDPA's kernel choice
        for _ in range(5):
            outs[name] = step(fn).detach().float()
        outs[name + "_grad"] = qkv.grad.float().clone()
    torch.cuda.synchronize()
    # the two arms compute the same op: bf16-rounding apart
    rel = ((outs["streaming"] - outs["fallback"]).norm() / outs["fallback"].norm()).item()
    rel_g = ((outs["streaming_grad"] - outs["fallback_grad"]).norm() / outs["fallback_grad"].norm()).item()
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                step(fn)
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / iters * 1e3)
    res = {"B": B, "S": S, "H": H, "rounds": rounds, "iters": iters, "out_rel_l2": rel, "grad_rel_l2": rel_g}
    for name, t in times.items():
        res[name + "_us"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    res["speedup"] = res["fallback_us"]["median"] / res["streaming_us"]["median"]
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per shape")
    ap.add_argument("--out", default="")
    ap.add_argument("--one", type=int, nargs=2, metavar=("B", "S"), help="time one shape in this process")
    a = ap.parse_args()
    if a.rounds < 20:
        ap.error("medians over at least 20 rounds")
    if a.one:
        one(a.one[0], a.one[1], a.rounds, a.iters)
        return 0
    results = []
    for B, S in SHAPES:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", str(B), str(S),
               "--rounds", str(a.rounds), "--iters", str(a.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout + r.stderr)
            print(f"shape ({B}, {S}) ended with status {r.returncode}: stopping")
            return 1
        results.append(json.loads(line[-1][7:]))
    print("| B | S | streaming us (min - max) | fallback us (min - max) | fallback / streaming | out rel-L2 | grad rel-L2 |")
    print("|---|---|---|---|---|---|---|")
    for r in results:
        s, f = r["streaming_us"], r["fallback_us"]
        print(f"| {r['B']} | {r['S']} | {s['median']:.0f} ({s['min']:.0f} - {s['max']:.0f}) | "
              f"{f['median']:.0f} ({f['min']:.0f} - {f['max']:.0f}) | {r['speedup']:.2f} | "
              f"{r['out_rel_l2']:.1e} | {r['grad_rel_l2']:.1e} |")
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
