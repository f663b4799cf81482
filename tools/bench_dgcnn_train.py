#!/usr/bin/env python3
"""Timing and peak memory of DGCNN training at B = 32, N = 1024, k = 20: the fused train-mode EdgeConv layer
(geoa3_amd/dgcnn_train.py, csrc/edgeconv_train.hip) against the plain torch composition (edge_train = "torch") at the same
commit.

    python tools/bench_dgcnn_train.py [--windows 5] [--iters 10] [--batch 32] [--npoint 1024] [--k 20] [--out FILE]

  layer 1..4   one EdgeConv layer on a fixed neighbour table, forward + backward to its input and weights, and the forward
               alone, both ways; peak allocated bytes of one forward + backward above what is resident, both ways
  kernels      the two raw entries (geoa3_edge_train_forward / _grad) of every layer, alone
  step         one whole training step (forward with its four searches, smoothed-label loss, backward, Adam) both ways, and
               its peak memory
Device events around `iters` calls after a warm-up, `windows` windows, the two ways alternated window by window; minimum
and range per entry."""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import main_train  # noqa: E402
from geoa3_amd import _lib, ops  # noqa: E402
from geoa3_amd.dgcnn import DGCNN, EDGE_LAYERS  # noqa: E402
from geoa3_amd.dgcnn_train import edgeconv_train, split_edge_weight  # noqa: E402
from bench_train import report, windows  # noqa: E402


def peak_of(fn):
    """peak allocated bytes of one call above what is resident before it (after one warm call)"""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, base


def layer_setup(l, B, N, k, dev):
    cin, cout = EDGE_LAYERS[l - 1]
    g = torch.Generator(device=dev).manual_seed(l)
    h = torch.randn(B, N, cin // 2, device=dev, generator=g).requires_grad_()
    idx = ops.knn_points(h.detach(), h.detach(), K=k).idx
    up = torch.randn(B, cout, N, device=dev, generator=g)
    torch.manual_seed(l)
    conv, bn = nn.Conv2d(cin, cout, 1, bias=False).to(dev), nn.BatchNorm2d(cout).to(dev).train()
    return h, idx, up, conv, bn


def layer_entries(l, B, N, k, dev):
    h, idx, up, conv, bn = layer_setup(l, B, N, k, dev)

    def both(mode):
        def run():
            for t in (h, conv.weight, bn.weight, bn.bias):
                t.grad = None
            (edgeconv_train(h, conv, bn, idx, mode) * up).sum().backward()
        return run

    def fwd(mode):
        def run():
            with torch.no_grad():
                edgeconv_train(h, conv, bn, idx, mode)
        return run
    return {"fused fwd+bwd": both("fused"), "torch fwd+bwd": both("torch"), "fused fwd": fwd("fused"), "torch fwd": fwd("torch")}


def kernel_entries(l, B, N, k, dev):
    h, idx, up, conv, bn = layer_setup(l, B, N, k, dev)
    with torch.no_grad():
        wa, wd = split_edge_weight(conv)
        U0, V0 = torch.matmul(h, wa.t()).contiguous(), torch.matmul(h, wd.t()).contiguous()
    ga, be = bn.weight.detach(), bn.bias.detach()
    ws = ops.edge_train_workspace(B, N, U0.shape[2], k, dev)
    y, arg, S1, _, _, stats = ops.edge_train(U0, V0, idx, ga, be, bn.eps, ws)
    return {"edge_train_forward": lambda: ops.edge_train(U0, V0, idx, ga, be, bn.eps, ws),
            "edge_train_grad": lambda: ops.edge_train_grad(up, y, U0, V0, arg, S1, idx, ga, stats, ws)}


def step_entries(B, N, k, dev):
    pts = torch.randn(B, 3, N, device=dev)
    target = torch.arange(B, device=dev) % 40
    crit = main_train.SmoothedLabelLoss(40)
    entries, peaks = {}, {}
    for mode in ("fused", "torch"):
        torch.manual_seed(0)
        net = DGCNN(k=k).to(dev).train()
        net.edge_train = mode
        opt = torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-4)

        def run(net=net, opt=opt):
            opt.zero_grad()
            crit(net(pts), target).backward()
            opt.step()
        entries[mode + " step"] = run
        peaks[mode] = peak_of(run)
    return entries, peaks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--npoint", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.load()
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    B, N, k = a.batch, a.npoint, a.k
    say("bench_dgcnn_train: B %d N %d k %d, %s, %d windows x %d calls" % (B, N, k, torch.cuda.get_device_name(0), a.windows, a.iters))
    for l in range(1, 5):
        ent = layer_entries(l, B, N, k, dev)
        report("layer %d (C'=%d)" % (l, EDGE_LAYERS[l - 1][1]), windows(ent, a.windows, a.iters), say)
        for mode in ("fused", "torch"):
            delta, base = peak_of(ent[mode + " fwd+bwd"])
            say("layer %d memory %-6s peak of one fwd+bwd %8.1f MB above the resident %8.1f MB" % (l, mode, delta / 2 ** 20, base / 2 ** 20))
        del ent
        report("layer %d kernels" % l, windows(kernel_entries(l, B, N, k, dev), a.windows, a.iters), say)
        torch.cuda.empty_cache()
    entries, peaks = step_entries(B, N, k, dev)
    report("training", windows(entries, a.windows, a.iters), say)
    for mode, (delta, base) in peaks.items():
        say("memory %-6s peak of one step %8.1f MB above the resident %8.1f MB" % (mode, delta / 2 ** 20, base / 2 ** 20))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
