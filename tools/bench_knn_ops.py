#!/usr/bin/env python3
"""Timing of knn_gather and of the backward passes of knn_gather / knn_points (csrc/geom_knn_ops.hip) beside the torch
composition they replace.

    python tools/bench_knn_ops.py [--repeats 7] [--iters 100] [--out profiles/knn_ops_bench.txt]

B = 250, n1 = n2 = 1024, K = 1 and K = 17 (the 1-NN tables and the k = 16 curvature table of the reference's objective: the
backward passes build their lists in LDS), and B = 64, n1 = n2 = 2048, K = 17 (the backward passes alone: an instance's
tables no longer fit LDS, the lists go through scratch).
Device events around `iters` calls after warm-up, the median (min .. max) of `repeats` such windows, the two forms timed in
alternation.  Per K:
  gather          out = knn_gather(x [B,n,3], idx)                       | torch.gather over the expanded index
  gather_bwd      d x from g [B,n,K,3]      (geoa3::knn_gather_grad)     | torch.zeros_like(x).scatter_add(...)
  points_bwd      d p1, d p2 from g [B,n,K] (geoa3::knn_points_grad)     | gather, two [B,n,K,3] products, sum, scatter_add
  kappa_adv       (K = 17 only: k = 16, with its own K = 1 search inside) forward + backward of the reference's
                  _get_kappa_adv (Lib/loss_utils.py:64-82) written on
                  ops.knn_points / ops.knn_gather                        | the same with torch.gather as knn_gather
The torch forms sum with float atomics (their bits change from run to run); the library's sum in a fixed order."""
import argparse
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


def torch_gather(x, idx):
    b, m, u = x.shape
    _, l, k = idx.shape
    return torch.gather(x, 1, idx.reshape(b, l * k, 1).expand(b, l * k, u)).view(b, l, k, u)


def torch_gather_bwd(g, idx, m):
    b, l, k, u = g.shape
    return g.new_zeros(b, m, u).scatter_add(1, idx.reshape(b, l * k, 1).expand(b, l * k, u), g.reshape(b, l * k, u))


def torch_points_bwd(p1, p2, idx, gd):
    b, n1, K = idx.shape
    nb = torch_gather(p2, idx)
    diff = 2.0 * gd.unsqueeze(-1) * (p1.unsqueeze(2) - nb)
    g1 = diff.sum(2)
    g2 = torch.zeros_like(p2).scatter_add(1, idx.reshape(b, n1 * K, 1).expand(b, n1 * K, 3), -diff.reshape(b, n1 * K, 3))
    return g1, g2


def kappa_adv(adv, ori, nrm, k, knn_points, knn_gather):
    pts = adv.permute(0, 2, 1)
    near = knn_points(pts, ori.permute(0, 2, 1), K=1)
    normal = knn_gather(nrm.permute(0, 2, 1), near.idx).permute(0, 3, 1, 2).squeeze(3).contiguous()
    own = knn_points(pts, pts, K=k + 1)
    nn_pts = knn_gather(pts, own.idx).permute(0, 3, 1, 2)[:, :, :, 1:].contiguous()
    v = nn_pts - adv.unsqueeze(3)
    v = v / v.norm(2, 1, keepdim=True).clamp(min=1e-12)
    return torch.abs((v * normal.unsqueeze(3)).sum(1)).mean(2), normal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from geoa3_amd import library, ops  # noqa: F401
    from oracle import geoa3_oracle as O
    assert torch.cuda.is_available(), "bench_knn_ops.py measures on the GPU"
    dev = torch.device("cuda")
    lines = []

    def compare(K, what, new, old):
        for fn in (new, old):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {0: [], 1: []}
        for _ in range(a.repeats):
            t[0].append(window(new, a.iters))
            t[1].append(window(old, a.iters))
        fmt = lambda v: "%9.1f (%9.1f .. %9.1f)" % (statistics.median(v), min(v), max(v))
        lines.append("%-4d %-11s %-30s %-30s %.3f" % (K, what, fmt(t[0]), fmt(t[1]),
                                                     statistics.median(t[0]) / statistics.median(t[1])))
        print(lines[-1], flush=True)

    # B = 250, n = 1024: the lists are built in LDS; B = 64, n = 2048, K = 17: 34816 entries per instance, 297 KB of tables --
    # the form with the lists in scratch (backward passes only)
    for B, n, K in ((250, 1024, 1), (250, 1024, 17), (64, 2048, 17)):
        ori, nrm = O.make_synthetic_clouds(B, n, seed=0)
        adv = (ori + 0.01 * torch.randn(ori.shape, generator=torch.Generator().manual_seed(1))).to(dev).contiguous()
        ori, nrm = ori.to(dev), nrm.to(dev)
        p1, p2 = adv.permute(0, 2, 1).contiguous(), ori.permute(0, 2, 1).contiguous()
        if K == 1 or n != 1024:
            lines += ["knn_gather / knn_points operators, B=%d n1=n2=%d, us per call: median (min .. max) of %d windows of %d calls"
                      % (B, n, a.repeats, a.iters),
                      "%-4s %-11s %-30s %-30s %s" % ("K", "what", "library", "torch composition", "library/torch")]
            print("\n".join(lines[-2:]), flush=True)
        idx = (ops.knn_points(p1, p2, K=K) if K == 1 else ops.knn_points(p1, p1, K=K)).idx
        src = p2 if K == 1 else p1
        g4 = torch.randn(B, n, K, 3, device=dev)
        gd = torch.rand(B, n, K, device=dev) + 0.5
        assert torch.equal(torch.ops.geoa3.knn_gather(src, idx), torch_gather(src, idx))
        torch.testing.assert_close(torch.ops.geoa3.knn_gather_grad(g4, idx, n), torch_gather_bwd(g4, idx, n), rtol=1e-4, atol=1e-5)
        for x, y in zip(torch.ops.geoa3.knn_points_grad(p1, src, idx, gd), torch_points_bwd(p1, src, idx, gd)):
            torch.testing.assert_close(x, y, rtol=1e-4, atol=1e-5)
        if n == 1024:
            compare(K, "gather", lambda: torch.ops.geoa3.knn_gather(src, idx), lambda: torch_gather(src, idx))
        compare(K, "gather_bwd", lambda: torch.ops.geoa3.knn_gather_grad(g4, idx, n), lambda: torch_gather_bwd(g4, idx, n))
        compare(K, "points_bwd", lambda: torch.ops.geoa3.knn_points_grad(p1, src, idx, gd),
                lambda: torch_points_bwd(p1, src, idx, gd))
        if K > 1 and n == 1024:
            def step(gather):
                x = adv.detach().requires_grad_()
                kap, _ = kappa_adv(x, ori, nrm, K - 1, ops.knn_points, gather)
                torch.autograd.grad(kap.sum(), x)
            compare(K, "kappa_adv", lambda: step(ops.knn_gather), lambda: step(torch_gather))
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
