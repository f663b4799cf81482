#!/usr/bin/env python3
"""Timing of the DGCNN victim's kernels (csrc/geom_knn_nd.hip, csrc/edgeconv.hip) and of the whole module.

    python tools/bench_dgcnn.py [--batch 250] [--npoint 1024] [--k 20] [--repeats 7] [--iters 10]

geoa3_knn_nd at D = 64 and 128 (the self search of a layer's input), edge_max forward and edge_max_grad (scratch allocation
included: the call a user makes) at C' = 64 and 256, every EdgeConv layer forward + backward to its input both fused (two
matmuls + geoa3::edge_max) and written with torch operators on the same folded-out weights (gather, cat, conv2d, batch_norm,
leaky_relu, max: what a user without the kernels would write, its [B,2C,N,k] tensors and atomic scatter included), and the
module's forward plus input gradient.  Device events around `iters` calls after warm-up, the median of `repeats` windows."""
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


def torch_edgeconv(x, idx, conv):
    """the public model's layer with the table given: x [B,C,N], idx int64 [B,N,k], conv = Sequential(Conv2d, BN, LeakyReLU)"""
    B, C, N = x.shape
    k = idx.shape[2]
    xt = x.transpose(1, 2)
    xj = torch.gather(xt, 1, idx.reshape(B, N * k, 1).expand(B, N * k, C)).view(B, N, k, C)
    xi = xt.unsqueeze(2).expand(B, N, k, C)
    return conv(torch.cat((xj - xi, xi), 3).permute(0, 3, 1, 2)).max(3)[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--npoint", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    from geoa3_amd import library, ops  # noqa: F401
    from geoa3_amd.dgcnn import DGCNN, EDGE_LAYERS, edgeconv
    dev = torch.device("cuda")
    B, N, k = a.batch, a.npoint, a.k
    torch.manual_seed(0)
    net = DGCNN(k=k).to(dev).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    w = net.folded(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 3, N, generator=g).to(dev)
    fns = {}
    # every layer's input and table, from one forward
    tables, inputs = [], []
    h = x.transpose(1, 2).contiguous()
    for l in range(1, 5):
        inputs.append(h)
        idx = ops.knn_points(h, h, K=k).idx
        tables.append(idx)
        h = edgeconv(h, w["wa%d" % l], w["wd%d" % l], w["t%d" % l], idx).transpose(1, 2).contiguous()
    for l in (2, 4):
        hq = inputs[l - 1]
        fns["knn_nd D=%d K=%d" % (hq.shape[2], k)] = lambda hq=hq: ops.knn_nd(hq, hq, k)
    for l in (1, 4):
        hl, idx = inputs[l - 1], tables[l - 1]
        U, V = torch.matmul(hl, w["wa%d" % l]), torch.matmul(hl, w["wd%d" % l])
        y, arg = ops.edge_max(U, V, w["t%d" % l], idx)
        go = torch.randn(y.shape, generator=g).to(dev)
        fns["edge_max C'=%d" % U.shape[2]] = lambda U=U, V=V, l=l, idx=idx: ops.edge_max(U, V, w["t%d" % l], idx)
        fns["edge_max_grad C'=%d" % U.shape[2]] = lambda go=go, y=y, arg=arg, idx=idx: ops.edge_max_grad(go, y, arg, idx)
    for l, (cin, cout) in enumerate(EDGE_LAYERS, 1):
        hl, idx = inputs[l - 1], tables[l - 1]
        go = torch.randn(B, cout, N, generator=g).to(dev)

        def fused(hl=hl, idx=idx, l=l, go=go):
            hh = hl.clone().requires_grad_()
            return torch.autograd.grad(edgeconv(hh, w["wa%d" % l], w["wd%d" % l], w["t%d" % l], idx), hh, go)

        def plain(hl=hl, idx=idx, l=l, go=go):
            xx = hl.transpose(1, 2).contiguous().requires_grad_()
            return torch.autograd.grad(torch_edgeconv(xx, idx, getattr(net, "conv%d" % l)), xx, go)

        fns["layer %d fused fwd+bwd (%d->%d)" % (l, cin // 2, cout)] = fused
        fns["layer %d torch fwd+bwd (%d->%d)" % (l, cin // 2, cout)] = plain

    def whole():
        xx = x.clone().requires_grad_()
        return torch.autograd.grad(net(xx).sum(), xx)

    fns["DGCNN forward + input gradient"] = whole
    for name, fn in fns.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        t = [window(fn, a.iters) for _ in range(a.repeats)]
        print(json.dumps({"what": name, "B": B, "N": N, "k": k, "us_median": round(statistics.median(t), 1),
                          "us_min": round(min(t), 1), "us_max": round(max(t), 1)}), flush=True)


if __name__ == "__main__":
    main()
