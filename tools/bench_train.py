#!/usr/bin/env python3
"""Timing of PointNet training at B = 32, N = 1024: the fused train-mode wide layer (geoa3_amd/pointnet_train.py) against
the plain torch composition (wide_train = "torch") at the same commit.

    python tools/bench_train.py [--windows 5] [--iters 20] [--batch 32] [--npoint 1024] [--out FILE]

  layer T=1 / T=3   one 1024-wide layer, forward + backward (conv -> BatchNorm(train) -> relu -> max, gradient of a random
                    upstream), both ways, and the forward alone both ways
  pieces T=1 / T=3  the fused backward's two kernels and its dense torch terms, each alone
  step              one whole training step (forward, loss of main_train.py, backward, Adam) both ways
  memory            peak allocated bytes of one step, both ways
Device events around `iters` calls after a warm-up, `windows` windows, the two ways alternated window by window; minimum
and range per entry."""
import argparse
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import main_train  # noqa: E402
from geoa3_amd import _lib  # noqa: E402
from geoa3_amd.pointnet import PointNet  # noqa: E402
from geoa3_amd.pointnet_train import wide_layer_train  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def windows(entries, nwin, iters):
    """entries: name -> callable; alternated window by window -> name -> list of ms per call"""
    for fn in entries.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {k: [] for k in entries}
    for _ in range(nwin):
        for k, fn in entries.items():
            res[k].append(timed(fn, iters))
    return res


def report(title, res, say):
    for k, v in res.items():
        say("%-40s min %8.3f ms   range %8.3f .. %8.3f   %s" % (title + " " + k, min(v), min(v), max(v),
                                                                " ".join("%.3f" % t for t in v)))


def layer_entries(taps, B, N, dev):
    g = torch.Generator(device=dev).manual_seed(taps)
    x = torch.randn(B, 128, N, device=dev, generator=g).relu().requires_grad_()
    up = torch.randn(B, 1024, device=dev, generator=g)
    mods = {}
    for mode in ("fused", "torch"):
        torch.manual_seed(0)
        conv, bn = nn.Conv1d(128, 1024, taps, 1, taps // 2).to(dev), nn.BatchNorm1d(1024, eps=1e-3).to(dev).train()
        mods[mode] = (conv, bn)

    def both(mode):
        conv, bn = mods[mode]

        def run():
            for t in (x, conv.weight, conv.bias, bn.weight, bn.bias):
                t.grad = None
            (wide_layer_train(x, conv, bn, True, mode) * up).sum().backward()
        return run

    def fwd(mode):
        conv, bn = mods[mode]

        def run():
            with torch.no_grad():
                wide_layer_train(x, conv, bn, True, mode)
        return run
    return {"fused fwd+bwd": both("fused"), "torch fwd+bwd": both("torch"), "fused fwd": fwd("fused"), "torch fwd": fwd("torch")}


def piece_entries(taps, B, N, dev):
    """the pieces of the fused layer's backward, each alone: the two kernels and the dense torch terms"""
    from geoa3_amd import pointnet_train as T
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    K = taps * 128
    g = torch.Generator(device=dev).manual_seed(10 + taps)
    x = torch.randn(B, 128, N, device=dev, generator=g).relu()
    w = torch.randn(1024, K, device=dev, generator=g) * 0.05
    coef = torch.randn(B, 1024, device=dev, generator=g)
    arg = torch.randint(0, N, (B, 1024), device=dev, generator=g, dtype=torch.int32)
    k2 = torch.randn(1024, device=dev, generator=g)
    dW, dX = torch.empty(1024, K, device=dev), torch.empty_like(x)
    U = T.unfold_taps(x, taps)
    Uf = U.permute(1, 0, 2).reshape(K, B * N)
    G = Uf @ Uf.t()
    P = w.t() @ (k2[:, None] * w)
    return {
        "gather kernel": lambda: lib.geoa3_wide_train_gather(x.data_ptr(), coef.data_ptr(), arg.data_ptr(), B, N, taps, dW.data_ptr(), st),
        "scatter kernel": lambda: lib.geoa3_wide_train_scatter(w.data_ptr(), coef.data_ptr(), arg.data_ptr(), B, N, taps, dX.data_ptr(), st),
        "torch S1": lambda: T.tap_sums(x, taps),
        "torch unfold + G = U U^T": lambda: (lambda Uf: Uf @ Uf.t())(T.unfold_taps(x, taps).permute(1, 0, 2).reshape(K, B * N)),
        "torch W G": lambda: w @ G,
        "torch P = W^T diag(k2) W": lambda: w.t() @ (k2[:, None] * w),
        "torch fold(P U + v)": lambda: T.fold_taps(torch.matmul(P, U) + k2[:K, None], taps),
    }


def step_entries(B, N, dev):
    pts = torch.randn(B, 3, N, device=dev)
    target = torch.arange(B, device=dev) % 40
    crit = main_train.SmoothedLabelLoss(40)
    entries, peaks = {}, {}
    for mode in ("fused", "torch"):
        torch.manual_seed(0)
        net = PointNet(40).to(dev).train()
        net.wide_train = mode
        opt = torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-4)

        def run(net=net, opt=opt):
            opt.zero_grad()
            out, tr = net(pts)
            (crit(out, target) + main_train.transform_penalty(tr) * 0.001).backward()
            opt.step()
        entries[mode + " step"] = run
        run()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run()
        torch.cuda.synchronize()
        peaks[mode] = (torch.cuda.max_memory_allocated() - base, torch.cuda.max_memory_allocated())
    return entries, peaks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--npoint", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.load()
    dev = torch.device("cuda")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("bench_train: B %d N %d, %s, %d windows x %d calls" % (a.batch, a.npoint, torch.cuda.get_device_name(0), a.windows, a.iters))
    for taps in (1, 3):
        report("layer T=%d" % taps, windows(layer_entries(taps, a.batch, a.npoint, dev), a.windows, a.iters), say)
    for taps in (1, 3):
        report("pieces T=%d" % taps, windows(piece_entries(taps, a.batch, a.npoint, dev), a.windows, a.iters), say)
    entries, peaks = step_entries(a.batch, a.npoint, dev)
    report("training", windows(entries, a.windows, a.iters), say)
    for mode, (delta, peak) in peaks.items():
        say("memory %-6s peak of one step %8.1f MB above the resident %8.1f MB" % (mode, delta / 2 ** 20, (peak - delta) / 2 ** 20))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
