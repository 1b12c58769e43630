"""Which kernel every convolution pass of one eager training step takes, as a list and its hash.

The conv / BatchNorm ops (ops/conv.py, ops/bn.py, ops/pool.py) hand work to each other through the
records of ops/handover.py; which native call runs, and with whose statistics, is decided by that
Python routing.  This tool records it: one eager step (bf16, channels_last, native engine, no
hipGraph) with ``ops.conv.profile_calls(True)``, then the ordered list of (pass, shape key, variant)
from ``take_profile()`` and its SHA-256.  Two commits route alike when the hashes agree for every
model and switch setting; the switches are read at import, so each setting is a process of its own:

    DPT_TAIL_CONV1_FUSE=0 python bench/handover_routing.py --model resnet50 --out r50.json

The default shape, batch 20 at 128 px, is the smallest batch at that size at which ResNet-50's
layer1 tails still take both tail fusions (``conv1x1_tail_refusal`` / ``conv1x1_tail_bwd_refusal``
refuse M = 19 * 32 * 32 rows: the split-K policy splits a grid of fewer than 160 tiles); layer2.0's
downsample conv takes the compact stride-2 path at any size.  ``--expect`` lists variants the step
must contain (exit status 3 otherwise).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from distributed_pytorch_training_amd import ops  # noqa: E402
from distributed_pytorch_training_amd.config import parse_args  # noqa: E402
from distributed_pytorch_training_amd.data import SyntheticLoader  # noqa: E402
from distributed_pytorch_training_amd.engine.trainer import Trainer  # noqa: E402
from distributed_pytorch_training_amd.models import build_model  # noqa: E402
from distributed_pytorch_training_amd.ops import conv as native_conv  # noqa: E402
from distributed_pytorch_training_amd.utils.env import setup_miopen_env, setup_tunableop  # noqa: E402

SWITCHES = ("DPT_TAIL_CONV1_FUSE", "DPT_TAIL_CONV3_BWD_FUSE", "DPT_S2_COMPACT_DRES", "DPT_BNR_FUSE",
            "DPT_BN_BWD_FUSE")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--batch-size", type=int, default=20)
    ap.add_argument("--image-size", type=int, default=128)
    ap.add_argument("--expect", default="", help="comma-separated variants the step must contain")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)

    setup_miopen_env()
    ops.native()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    setup_tunableop()
    args = parse_args(["--model", a.model, "--dataset", "synthetic", "--batch-size", str(a.batch_size),
                       "--image-size", str(a.image_size), "--amp", "--amp-dtype", "bf16", "--channels-last",
                       "--no-cuda-graph"])
    torch.manual_seed(0)
    model = build_model(a.model, 1000, dev, image_size=a.image_size, channels_last=True)
    tr = Trainer(model, args, 0, 1, dev, log=lambda s: None)
    loader = SyntheticLoader(a.batch_size, a.batch_size, a.image_size, 1000, dev, channels_last=True, pool=1,
                             seed=0)
    x, y = next(iter(loader))
    native_conv.profile_calls(True)
    tr.train_step(x, y)
    torch.cuda.synchronize()
    calls = [[kind, list(key[:7]) + [list(key[7])], variant] for kind, key, variant, _, _ in
             native_conv.take_profile()]
    native_conv.profile_calls(False)

    variants = {}
    for _, _, v in calls:
        variants[v] = variants.get(v, 0) + 1
    rec = {"model": a.model, "batch": a.batch_size, "image": a.image_size,
           "switches_off": [s for s in SWITCHES if os.environ.get(s) == "0"],
           "calls": len(calls), "sha256": hashlib.sha256(json.dumps(calls).encode()).hexdigest(),
           "variants": dict(sorted(variants.items()))}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(rec, list=calls), f)
    missing = [v for v in a.expect.split(",") if v and not any(v in got for got in variants)]
    if missing:
        print(f"handover_routing: the step took no {missing}", file=sys.stderr)
        return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())
