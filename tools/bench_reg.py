#!/usr/bin/env python3
"""Timing of the neighbour-based regularisers (csrc/geom_reg.hip) and of the attack iteration with
--is_use_knn_smoothing_loss, --displacement_loss_weight, --repulsion_loss_weight and --corr_normal_loss_weight off and on.

    python tools/bench_reg.py [--repeats 7] [--iters 20] [--steps 20] [--skip-kernels]

kernels: forward and backward of kNN_smoothing_loss / repulsion_loss / displacement_loss at B = 250 for (N, k) = (1024, 5),
(1024, 16), (4096, 16), the K-NN table handed over (its search is not in the figure; `knn_self` is it alone, without a
prior), device events around `iters` calls after warm-up, the median of `repeats` such windows.  iteration: configs[1]
(PointNet, 1024 points, curvature k = 16) runners with every term off, with the kNN-smoothing term on (weight 5, k 5,
coef 1.10: the shared-table path; `on_us`), with the displacement / repulsion / normal term on alone (`disp_us`, `rep_us`,
`cnor_us`; the reference functions' own k, weight 1) and with those three on (`all3_us`), built in one process, timed in
alternation (windows of `steps` iterations, median of `repeats`)."""
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
    ap.add_argument("--skip-kernels", action="store_true", help="the iteration figures only")
    a = ap.parse_args()
    import bench
    from geoa3_amd import ops
    from geoa3_amd.attack import AttackRunner
    from geoa3_amd.data import synthetic_state_dict
    from geoa3_amd.pointnet import PointNet
    from oracle import geoa3_oracle as O
    dev = torch.device("cuda")
    B = 250
    for N, k in (() if a.skip_kernels else ((1024, 5), (1024, 16), (4096, 16))):
        ori, _ = O.make_synthetic_clouds(B, N, seed=0)
        x = (ori + 0.01 * torch.randn(ori.shape, generator=torch.Generator().manual_seed(1))).to(dev).contiguous()
        ori = ori.to(dev).contiguous()
        ws = ops.reg_workspace(B, N, k, dev)
        tx, to = ops.knn_self_planar(x, k + 1), ops.knn_self_planar(ori, k + 1)
        vb, vn, g = torch.empty(B, device=dev), torch.empty(B, N, device=dev), torch.empty(B, 3, N, device=dev)
        vc, gg = torch.zeros(B, device=dev), torch.zeros(B, 3, N, device=dev)
        fns = {
            "knn_self": lambda: ops.knn_self_planar(x, k + 1, out=tx),
            "smoothing_fwd": lambda: ops.knn_smoothing_loss(x, k, 1.1, knn=tx, workspace=ws, out=vb),
            "smoothing_bwd": lambda: ops.knn_smoothing_loss_grad(x, k, 1.1, knn=tx, workspace=ws, out=g),
            "repulsion_fwd": lambda: ops.repulsion_loss(x, k, 0.03, knn=tx, workspace=ws, out=vn),
            "repulsion_bwd": lambda: ops.repulsion_loss_grad(x, k, 0.03, knn=tx, workspace=ws, out=g),
            "displacement_fwd": lambda: ops.displacement_loss(x, ori, k, knn=to, workspace=ws, out=vn),
            "displacement_bwd": lambda: ops.displacement_loss_grad(x, ori, k, knn=to, workspace=ws, out=g),
            "fold_points": lambda: ops.reg_fold_points(vn, g, 0.5, B, N, term=vb, constrain=vc, constrain_add=True, g=gg,
                                                       g_add=True),
        }
        for name, fn in fns.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            t = [window(fn, a.iters) for _ in range(a.repeats)]
            print(json.dumps({"what": name, "B": B, "N": N, "k": k, "us_median": round(statistics.median(t), 1),
                              "us_min": round(min(t), 1), "us_max": round(max(t), 1)}), flush=True)
    net = PointNet(40)
    net.load_state_dict(synthetic_state_dict(40, seed=0, device=dev))
    net = net.to(dev).eval()
    N, knn = 1024, 16
    ori, nrm = O.make_synthetic_clouds(B, N, seed=0)
    ori, nrm = ori.to(dev), nrm.to(dev)
    with torch.no_grad():
        gt = net(ori).argmax(1).int()
    # the loop with one term on at a time: the kNN-smoothing term (weight 5, k 5, coef 1.10: the shared-table path), then
    # the displacement (k 16: the clean table of the curvature term), repulsion (k 4) and normal (k 2) terms, which take
    # the curvature term's table of the iteration, and the three together
    variants = {
        "off": {},
        "on": dict(is_use_knn_smoothing_loss=True),
        "disp": dict(displacement_loss_weight=1.0),
        "rep": dict(repulsion_loss_weight=1.0),
        "cnor": dict(corr_normal_loss_weight=1.0),
        "all3": dict(displacement_loss_weight=1.0, repulsion_loss_weight=1.0, corr_normal_loss_weight=1.0),
    }
    runners = {}
    for name, kw in variants.items():
        cfg = bench.cfg_full_geoa3(10 ** 6, N, knn)
        cfg.is_use_knn_smoothing_loss = False
        cfg.knn_smoothing_loss_weight, cfg.knn_smoothing_k, cfg.knn_threshold_coef = 5.0, 5, 1.10
        for key, val in kw.items():
            setattr(cfg, key, val)
        r = AttackRunner(net, B, N, cfg, dev)
        r.setup(ori, nrm, gt, gt)
        r.begin_search_step((torch.randn(B, 3, N, generator=torch.Generator().manual_seed(7)) * 1e-3).to(dev))
        runners[name] = r
    step = {on: 0 for on in runners}

    def run(on):
        runners[on].step(step[on], 0)
        step[on] += 1

    for on in runners:
        for _ in range(5):
            run(on)
    torch.cuda.synchronize()
    times = {on: [] for on in runners}
    for _ in range(a.repeats):
        for on in runners:
            times[on].append(window(lambda: run(on), a.steps))
    med = {on: statistics.median(times[on]) for on in runners}
    res = {"what": "iteration", "config": "configs[1]", "N": N, "off_us": round(med["off"], 1), "on_us": round(med["on"], 1),
           "off_min_max_us": [round(min(times["off"]), 1), round(max(times["off"]), 1)],
           "ratio": round(med["on"] / med["off"], 4)}
    for on in ("disp", "rep", "cnor", "all3"):
        res[on + "_us"] = round(med[on], 1)
        res[on + "_min_max_us"] = [round(min(times[on]), 1), round(max(times[on]), 1)]
    print(json.dumps(res), flush=True)
    for r in runners.values():
        r.end_search_step()


if __name__ == "__main__":
    main()
