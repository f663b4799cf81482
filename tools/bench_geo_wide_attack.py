#!/usr/bin/env python3
"""ms per iteration of a PointNet attack on dense clouds (default: b = 32, 8192 points, the full objective), with the
objective's share of it: the loop with and without the geometric terms' kernels timed alone.
python tools/bench_geo_wide_attack.py [--b 32] [--n 8192] [--k 16] [--steps 20]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=32)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import bench
    from geoa3_amd import ops
    from geoa3_amd.attack import AttackRunner
    from geoa3_amd.data import synthetic_clouds, synthetic_state_dict
    from geoa3_amd.pointnet import PointNet
    dev = torch.device("cuda")
    net = PointNet(40)
    net.load_state_dict(synthetic_state_dict(40, seed=0))
    net = net.to(dev).eval()
    ori, nrm = synthetic_clouds(a.b, a.n, seed=7)
    ori, nrm = ori.to(dev), nrm.to(dev)
    with torch.no_grad():
        gt = net(ori).argmax(1)
    cfg = bench.cfg_full_geoa3(a.steps + a.warmup + 4, a.n, a.k)
    r = AttackRunner(net, a.b, a.n, cfg, dev)
    r.setup(ori, nrm, gt, gt)
    r.begin_search_step((torch.randn(a.b, 3, a.n, generator=torch.Generator().manual_seed(11)) * 1e-3).to(dev))
    for s in range(a.warmup):
        r.step(s, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(a.warmup, a.warmup + a.steps):
        r.step(s, 0)
    torch.cuda.synchronize()
    ms_iter = (time.perf_counter() - t0) * 1e3 / a.steps
    # the objective's launch alone, on the loop's last iterate
    x = r.t["x"][:, :, :a.n].contiguous() if r.t["x"].shape[2] != a.n else r.t["x"]
    d_ao, i_ao, d_oa, i_oa = ops.nn1_pair(x, ori)
    _, knn_ori = ops.knn_planar(ori, ori, a.k + 1)
    kap = ops.kappa(ori, nrm, knn_ori)
    _, knn_adv = ops.knn_planar(x, x, a.k + 1, knn_ori)
    scratch, out = ops.geo_scratch(a.b, a.n, dev, a.k), {}
    fn = lambda: ops.geo_loss_grad(x, ori, normal_ori=nrm, kappa_ori=kap, d_ao=d_ao, i_ao=i_ao, d_oa=d_oa, i_oa=i_oa,
                                   knn_adv=knn_adv, k=a.k, w_dis=1.0, w_hd=0.1, w_curv=1.0, out=out, scratch=scratch)
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    geo_ms = e0.elapsed_time(e1) / a.steps
    print(json.dumps({"b": a.b, "n": a.n, "k": a.k, "ms_per_iteration": round(ms_iter, 3), "objective_ms": round(geo_ms, 4),
                      "objective_share": round(geo_ms / ms_iter, 4)}))


if __name__ == "__main__":
    main()
