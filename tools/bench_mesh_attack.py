#!/usr/bin/env python3
"""Timing of the mesh attack's kernels (csrc/mesh_attack.hip) and of one loop iteration of --attack GeoA3_mesh beside the
point-cloud iteration at the same B, S and victim.

    python tools/bench_mesh_attack.py [--repeats 7] [--iters 20] [--steps 20] [--level 3] [--skip-kernels]

kernels: B = 250 icospheres of `--level` subdivisions (level 3: 642 vertices, 1280 faces, 1920 edges), stretched per
instance, S = 1024 surface points: mesh_points, mesh_corner_index, the destination-list build (once per draw in the loop),
mesh_points_grad, mesh_reg, mesh_reg_grad (both terms on), mesh_edge_lengths, and -- for scale -- the whole geometric
objective of the point-cloud loop on the same clouds (1-NN tables, K-NN table, fused CD + HD + curvature kernel:
`geo_objective`).  Device events around `iters` calls after warm-up, the median of `repeats` such windows.
iteration: the PointNet victim, configs[1]'s flags (curvature k = 16); `points_us` the point-cloud runner on the clean
sample, `mesh_off_us` the mesh runner with both mesh weights 0, `mesh_on_us` with --laplacian_loss_weight 0.5
--edge_loss_weight 20, built in one process and timed in alternation (windows of `steps` iterations, median of `repeats`)."""
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
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--skip-kernels", action="store_true", help="the iteration figures only")
    a = ap.parse_args()
    import bench
    from geoa3_amd import mesh as M
    from geoa3_amd.attack import AttackRunner
    from geoa3_amd.data import synthetic_state_dict
    from geoa3_amd.mesh_attack import MeshAttackRunner, synthetic_meshes
    from geoa3_amd.pointnet import PointNet
    dev = torch.device("cuda")
    B, S, knn = a.batch, 1024, 16
    packed = M.pack_meshes(synthetic_meshes(B, seed=0, level=a.level), dev)
    verts, nv = M.to_planar(packed)
    vp = verts.shape[2]
    topo = M.MeshTopology.from_packed(packed)
    u = torch.rand(B, S, 3, device=dev, generator=torch.Generator(dev).manual_seed(1))
    pts, nrm, fidx, _ = M.sample_surface(packed, S, u=u)
    x = (verts + 0.01 * torch.randn(verts.shape, device=dev, generator=torch.Generator(dev).manual_seed(2))).contiguous()
    own = topo.edge_lengths(verts)
    lists = M.mesh_point_lists(nv, packed.faces, packed.face_off, fidx, vp)
    g_pts = torch.randn(B, 3, S, device=dev, generator=torch.Generator(dev).manual_seed(3))
    g_out = torch.empty(B, 3, vp, device=dev)
    _, _, unit = M.mesh_reg_forward(x, nv, topo.row_off, topo.col, topo.ne, own, 0.0)

    net = PointNet(40)
    net.load_state_dict(synthetic_state_dict(40, seed=0, device=dev))
    net = net.to(dev).eval()
    with torch.no_grad():
        gt = net(pts).argmax(1).int()
    cfg_p = bench.cfg_full_geoa3(10 ** 6, S, knn)
    points = AttackRunner(net, B, S, cfg_p, dev)
    points.setup(pts, nrm, gt, gt)
    points.begin_search_step((torch.randn(B, 3, S, generator=torch.Generator().manual_seed(7)) * 1e-3).to(dev))

    if not a.skip_kernels:
        s = torch.cuda.current_stream().cuda_stream
        xe = points.t["x"]

        def geo_objective():
            points._constrain, points._geo_on = None, False     # as AttackRunner._geometry starts its terms
            points._distance_curvature(xe, s)

        fns = {
            "mesh_points": lambda: M.mesh_points_forward(x, nv, packed.faces, packed.face_off, fidx, u),
            "mesh_corner_index": lambda: M.mesh_corner_index(nv, packed.faces, packed.face_off, fidx, vp),
            "mesh_point_lists": lambda: M.mesh_point_lists(nv, packed.faces, packed.face_off, fidx, vp),
            "mesh_points_grad": lambda: M.mesh_points_backward(g_pts, u, lists, vp, out=g_out),
            "mesh_reg": lambda: M.mesh_reg_forward(x, nv, topo.row_off, topo.col, topo.ne, own, 0.0),
            "mesh_reg_grad": lambda: M.mesh_reg_backward(x, nv, topo.row_off, topo.col, topo.ne, own, 0.0, unit, None, None,
                                                         0.5, 20.0, out=g_out),
            "mesh_edge_lengths": lambda: topo.edge_lengths(x),
            "geo_objective": geo_objective,
        }
        for name, fn in fns.items():
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            t = [window(fn, a.iters) for _ in range(a.repeats)]
            print(json.dumps({"what": name, "B": B, "S": S, "V": vp, "nnz": topo.nnz, "us_median": round(statistics.median(t), 1),
                              "us_min": round(min(t), 1), "us_max": round(max(t), 1)}), flush=True)

    runners = {"points": points}
    for name, (w_lap, w_edge) in (("mesh_off", (0.0, 0.0)), ("mesh_on", (0.5, 20.0))):
        cfg = bench.cfg_full_geoa3(10 ** 6, S, knn)
        cfg.laplacian_loss_weight, cfg.edge_loss_weight = w_lap, w_edge
        r = MeshAttackRunner(net, B, vp, cfg, dev)
        r.setup_mesh(packed, gt, gt, u=u)
        r.begin_search_step((torch.randn(B, 3, vp, generator=torch.Generator().manual_seed(7)) * 1e-3).to(dev))
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
    res = {"what": "iteration", "B": B, "S": S, "V": vp, "victim": "PointNet"}
    for on in runners:
        res[on + "_us"] = round(med[on], 1)
        res[on + "_min_max_us"] = [round(min(times[on]), 1), round(max(times[on]), 1)]
    res["mesh_on_over_points"] = round(med["mesh_on"] / med["points"], 4)
    print(json.dumps(res), flush=True)
    for r in runners.values():
        r.end_search_step()


if __name__ == "__main__":
    main()
