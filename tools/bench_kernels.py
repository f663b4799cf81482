#!/usr/bin/env python3
"""Micro-benchmarks of the individual HIP kernels at the BASELINE config (B=250, N=1024, k=16).
python tools/bench_kernels.py [--B 250] [--N 1024] [--k 16] [--iters 20]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def timeit(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us


def geo_case(ops, B, N, k, iters, **route):
    """The fused objective on B clouds of N points, k neighbours: us per launch and ns per (centre, neighbour) pair.
    Clouds of 1025..4096 points take geo_big_kernel, 5840..8192 the two-pass kernels (route: wide_ranges = S forces them)."""
    g = torch.Generator().manual_seed(N + k)
    u = torch.randn(B, 3, N, generator=g)
    ori = (u / u.norm(dim=1, keepdim=True)).cuda().contiguous()
    nrm = ori.clone()
    adv = (ori + 0.01 * torch.randn(B, 3, N, generator=g).cuda()).contiguous()
    _, knn_ori = ops.knn_planar(ori, ori, k + 1)
    kap = ops.kappa(ori, nrm, knn_ori)
    d_ao, i_ao, d_oa, i_oa = ops.nn1_pair(adv, ori)
    _, knn_adv = ops.knn_planar(adv, adv, k + 1, knn_ori)
    out = {}
    if "wide_ranges" not in route:
        route["scratch"] = ops.geo_scratch(B, N, adv.device, k)
    us = timeit(lambda: ops.geo_loss_grad(adv, ori, normal_ori=nrm, kappa_ori=kap, d_ao=d_ao, i_ao=i_ao, d_oa=d_oa, i_oa=i_oa,
                                          knn_adv=knn_adv, k=k, w_dis=1.0, w_hd=0.1, w_curv=1.0, out=out, **route), iters)
    return us, us * 1e3 / (B * N * k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geo-only", action="store_true", help="only the objective on large clouds (the last lines)")
    ap.add_argument("--B", type=int, default=250)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from geoa3_amd import ops
    B, N, k = a.B, a.N, a.k
    if not a.geo_only:
        kernels(ops, a, B, N, k)
    # the objective beyond 1024 points: geo_big_kernel at 4096, the two-pass kernels at 8192 (the first and the last line
    # hold the same number of pairs) and, for the cost of their S scans, forced onto the 4096-point case
    res = {}
    for name, (gB, gN, gk, route) in {"geo_wide_b64_n8192_k32": (64, 8192, 32, {}), "geo_wide_b250_n8192_k16": (250, 8192, 16, {}),
                                      "geo_wide_s1_b128_n4096_k32": (128, 4096, 32, dict(wide_ranges=1)),
                                      "geo_wide_s4_b128_n4096_k32": (128, 4096, 32, dict(wide_ranges=4)),
                                      "geo_big_b128_n4096_k32": (128, 4096, 32, {})}.items():
        us, ns = geo_case(ops, gB, gN, gk, a.iters, **route)
        res[name + "_us"], res[name + "_ns_per_pair"] = us, ns
    print(json.dumps({kk: round(v, 4) for kk, v in res.items()}))


def kernels(ops, a, B, N, k):
    g = torch.Generator().manual_seed(0)
    u = torch.randn(B, 3, N, generator=g)
    ori = (u / u.norm(dim=1, keepdim=True)).cuda().contiguous()
    nrm = ori.clone()
    adv = (ori + 0.01 * torch.randn(B, 3, N, generator=g).cuda()).contiguous()
    res = {}
    res["nn1_pair_us"] = timeit(lambda: ops.nn1_pair(adv, ori), a.iters)
    res["nn1_grid_us"] = timeit(lambda: ops.nn1_pair(adv, ori, method="grid"), a.iters)
    far = (ori + 0.3 * torch.randn(B, 3, N, generator=g).cuda()).contiguous()
    res["nn1_pair_far_us"] = timeit(lambda: ops.nn1_pair(far, ori), a.iters)
    res["nn1_grid_far_us"] = timeit(lambda: ops.nn1_pair(far, ori, method="grid"), a.iters)
    flops = 8.0 * B * N * N
    res["nn1_pair_alg_GBps"] = 40.0 * B * N / res["nn1_pair_us"] / 1e3
    res["nn1_pair_valu_frac"] = flops / (res["nn1_pair_us"] * 1e-6) / 157.3e12
    _, knn_ori = ops.knn_planar(ori, ori, k + 1)
    res["knn_noprior_us"] = timeit(lambda: ops.knn_planar(adv, adv, k + 1), a.iters)
    res["knn_prior_us"] = timeit(lambda: ops.knn_planar(adv, adv, k + 1, knn_ori), a.iters)
    scratch = ops.knn_self_scratch(B, N, adv.device)
    res["knn_slab_us"] = timeit(lambda: ops.knn_self_planar(adv, k + 1, knn_ori, scratch, method=1), a.iters)
    res["knn_grid_us"] = timeit(lambda: ops.knn_self_planar(adv, k + 1, knn_ori, scratch, method=2), a.iters)
    _, knn_far = ops.knn_planar(far, far, k + 1)
    res["knn_prior_far_us"] = timeit(lambda: ops.knn_planar(far, far, k + 1, knn_far), a.iters)
    res["knn_slab_far_us"] = timeit(lambda: ops.knn_self_planar(far, k + 1, knn_far, scratch, method=1), a.iters)
    res["knn_grid_far_us"] = timeit(lambda: ops.knn_self_planar(far, k + 1, knn_far, scratch, method=2), a.iters)
    # the attack's regime: a stale table (last iteration's, here the clean cloud's) as the radius
    res["knn_grid_stale_us"] = timeit(lambda: ops.knn_self_planar(far, k + 1, knn_ori, scratch, method=2), a.iters)
    res["knn_slab_stale_us"] = timeit(lambda: ops.knn_self_planar(far, k + 1, knn_ori, scratch, method=1), a.iters)
    # the position-list slab kernel for long lists / large clouds (knn_slabp_kernel<56, true>): method 4 at K = 33, N = 4096
    u4 = torch.randn(B, 3, 4096, generator=g)
    ori4 = (u4 / u4.norm(dim=1, keepdim=True)).cuda().contiguous()
    adv4 = (ori4 + 0.01 * torch.randn(B, 3, 4096, generator=g).cuda()).contiguous()
    _, knn4 = ops.knn_planar(ori4, ori4, 33)
    scratch4 = ops.knn_self_scratch(B, 4096, adv4.device)
    res["knn_slabp56_n4096_k33_us"] = timeit(lambda: ops.knn_self_planar(adv4, 33, knn4, scratch4, method=4), a.iters)
    kap = ops.kappa(ori, nrm, knn_ori)
    res["kappa_us"] = timeit(lambda: ops.kappa(ori, nrm, knn_ori), a.iters)
    d_ao, i_ao, d_oa, i_oa = ops.nn1_pair(adv, ori)
    _, knn_adv = ops.knn_planar(adv, adv, k + 1, knn_ori)
    out = {}
    for det in (True, False):
        res["geo_loss_grad_%s_us" % ("det" if det else "atomic")] = timeit(lambda: ops.geo_loss_grad(
            adv, ori, normal_ori=nrm, kappa_ori=kap, d_ao=d_ao, i_ao=i_ao, d_oa=d_oa, i_oa=i_oa, knn_adv=knn_adv, k=k,
            w_dis=1.0, w_hd=0.1, w_curv=1.0, out=out, deterministic=det), a.iters)
    print(json.dumps({"B": B, "N": N, "k": k, **{kk: round(v, 3) for kk, v in res.items()}}))


if __name__ == "__main__":
    main()
