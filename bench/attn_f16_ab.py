"""Self-attention forward + backward in fp16: the native kernels (fa.attention -> the *_f16 bindings)
vs what fp16 ran before them (split_heads + scaled_dot_product_attention + merge_heads), with the
native bf16 path alongside, at ViT-B/16's 224 px and 384 px token counts.

    python bench/attn_f16_ab.py [--rounds 20] [--iters 10] [--batch 128]

The three arms alternate round by round after a warm-up of each; a round is ``iters``
forward+backward calls between two device events; the table reports the median round (min - max)
per call in microseconds.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H = 12


def main():
    from distributed_pytorch_training_amd import ops
    from distributed_pytorch_training_amd.ops import attention as fa
    from distributed_pytorch_training_amd.ops.vit import merge_heads, split_heads

    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    ops.native()
    fa.ENABLED = fa.STREAMING = True
    print("| B | S | native fp16 us (min - max) | SDPA fp16 us (min - max) | native bf16 us (min - max) | SDPA / native fp16 |")
    print("|---|---|---|---|---|---|")
    for S in (197, 577):
        torch.manual_seed(0)
        x = torch.randn(a.batch, S, 3 * H * 64, device="cuda")
        d = torch.randn(a.batch, S, H * 64, device="cuda")
        qkv = {dt: x.to(dt).requires_grad_(True) for dt in (torch.float16, torch.bfloat16)}
        dout = {dt: d.to(dt) for dt in qkv}
        assert fa.supported_f16(qkv[torch.float16], H) or fa.supported_streaming_f16(qkv[torch.float16], H)

        def sdpa(t):
            q, k, v = split_heads(t, H)
            return merge_heads(F.scaled_dot_product_attention(q, k, v))

        arms = {"native fp16": (lambda t: fa.attention(t, H), torch.float16), "SDPA fp16": (sdpa, torch.float16),
                "native bf16": (lambda t: fa.attention(t, H), torch.bfloat16)}

        def step(name):
            fn, dt = arms[name]
            qkv[dt].grad = None
            fn(qkv[dt]).backward(dout[dt])

        for name in arms:          # warm-up: code objects, SDPA's kernel choice
            for _ in range(5):
                step(name)
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for _ in range(a.rounds):
            for name in arms:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.iters):
                    step(name)
                e.record()
                torch.cuda.synchronize()
                times[name].append(s.elapsed_time(e) / a.iters * 1e3)
        med = {n: statistics.median(t) for n, t in times.items()}
        cells = " | ".join(f"{med[n]:.0f} ({min(times[n]):.0f} - {max(times[n]):.0f})" for n in arms)
        print(f"| {a.batch} | {S} | {cells} | {med['SDPA fp16'] / med['native fp16']:.2f} |", flush=True)


if __name__ == "__main__":
    main()
