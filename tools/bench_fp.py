#!/usr/bin/env python3
"""Timing of the feature-propagation operators (csrc/pointnet2_interp.hip).

    python tools/bench_fp.py [--repeats 7] [--iters 20]

three_nn, three_interpolate and three_interpolate_grad (scratch allocation included: the call a user makes) at B = 16, C = 256
for (n, m) = (1024, 256), a segmentation-like up-sampling step, and (4096, 4096); beside them torch.cdist + topk(3,
largest=False) on the same clouds (what a user without the kernel would write; its distances are not the reference's
bits).  Device events around `iters` calls after warm-up, the median of `repeats` such windows."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n   # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from geoa3_amd.pointnet2 import ext
    dev = torch.device("cuda")
    B, C = 16, 256
    for n, m in ((1024, 256), (4096, 4096)):
        g = torch.Generator().manual_seed(n + m)
        unknown = torch.randn(B, n, 3, generator=g).to(dev)
        known = torch.randn(B, m, 3, generator=g).to(dev)
        feats = torch.randn(B, C, m, generator=g).to(dev)
        grad = torch.randn(B, C, n, generator=g).to(dev)
        dist2, idx = ext.three_nn(unknown, known)
        rec = 1.0 / (dist2.sqrt() + 1e-8)
        weight = (rec / rec.sum(2, keepdim=True)).contiguous()
        fns = {
            "three_nn": lambda: ext.three_nn(unknown, known),
            "cdist_topk3": lambda: torch.cdist(unknown, known).topk(3, dim=2, largest=False),
            "three_interpolate": lambda: ext.three_interpolate(feats, idx, weight),
            "three_interpolate_grad": lambda: ext.three_interpolate_grad(grad, idx, weight, m),
        }
        for name, fn in fns.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            t = [window(fn, a.iters) for _ in range(a.repeats)]
            print(json.dumps({"what": name, "B": B, "n": n, "m": m, "C": C, "us_median": round(statistics.median(t), 1),
                              "us_min": round(min(t), 1), "us_max": round(max(t), 1)}), flush=True)


if __name__ == "__main__":
    main()
