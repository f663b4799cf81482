#!/usr/bin/env python3
"""Timing of the uniformity term (geoa3_uniform_loss, csrc/geom_uniform.hip) and of the attack iteration with
--uniform_loss_weight 0 and 1.

    python tools/bench_uniform.py [--repeats 7] [--iters 20] [--steps 20]

op: U and dU/dx at B = 250 for N = 1024 and 4096, device events around `iters` calls after warm-up, the median of
`repeats` such windows.  iteration: configs[1] (PointNet, 1024 points, k = 16) and configs[4] (4096 points, k = 32) runners
with weight 0 and weight 1 built in one process, timed in alternation (windows of `steps` iterations, median of
`repeats`)."""
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
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    import bench
    from geoa3_amd import ops
    from geoa3_amd.attack import AttackRunner
    from geoa3_amd.data import synthetic_state_dict
    from geoa3_amd.pointnet import PointNet
    from oracle import geoa3_oracle as O
    dev = torch.device("cuda")
    rows = []
    for N in (1024, 4096):
        ori, _ = O.make_synthetic_clouds(250, N, seed=0)
        x = (ori + 0.01 * torch.randn(ori.shape, generator=torch.Generator().manual_seed(1))).to(dev).contiguous()
        ws = ops.uniform_workspace(250, N, dev)
        out = (torch.empty((), device=dev), torch.empty(250, 3, N, device=dev))
        fn = lambda: ops.uniform_loss(x, workspace=ws, out=out)
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t = [window(fn, a.iters) for _ in range(a.repeats)]
        rows.append({"what": "op", "B": 250, "N": N, "us_median": round(statistics.median(t), 1),
                     "us_min": round(min(t), 1), "us_max": round(max(t), 1)})
        print(json.dumps(rows[-1]), flush=True)
    net = PointNet(40)
    net.load_state_dict(synthetic_state_dict(40, seed=0, device=dev))
    net = net.to(dev).eval()
    for name, N, knn in (("configs[1]", 1024, 16), ("configs[4]", 4096, 32)):
        ori, nrm = O.make_synthetic_clouds(250, N, seed=0)
        ori, nrm = ori.to(dev), nrm.to(dev)
        with torch.no_grad():
            gt = net(ori).argmax(1).int()
        runners = {}
        for w in (0.0, 1.0):
            cfg = bench.cfg_full_geoa3(10 ** 6, N, knn)
            cfg.uniform_loss_weight = w
            r = AttackRunner(net, 250, N, cfg, dev)
            r.setup(ori, nrm, gt, gt)
            r.begin_search_step((torch.randn(250, 3, N, generator=torch.Generator().manual_seed(7)) * 1e-3).to(dev))
            runners[w] = r
        step = {w: 0 for w in runners}

        def run(w):
            r = runners[w]
            r.step(step[w], 0)
            step[w] += 1

        for w in runners:
            for _ in range(5):
                run(w)
        torch.cuda.synchronize()
        times = {w: [] for w in runners}
        for _ in range(a.repeats):
            for w in runners:
                times[w].append(window(lambda: run(w), a.steps))
        m0, m1 = statistics.median(times[0.0]), statistics.median(times[1.0])
        rows.append({"what": "iteration", "config": name, "N": N, "w0_us": round(m0, 1), "w1_us": round(m1, 1),
                     "ratio": round(m1 / m0, 4)})
        print(json.dumps(rows[-1]), flush=True)
        for r in runners.values():
            r.end_search_step()


if __name__ == "__main__":
    main()
