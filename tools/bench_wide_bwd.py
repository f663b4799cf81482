#!/usr/bin/env python3
"""Timing of the three sparse arg-max backward launches of a configs[1] iteration (csrc/pointnet_wide_bwdconv.hip), alone,
for one or more builds of the library in ONE process.

    python tools/bench_wide_bwd.py [--libs A.so B.so ...] [--windows 5] [--iters 200] [--out profiles/wide_bwd_conv_ab.txt]

B = 250, N = 1024.  The lists are the loop's own: a forward + backward of the synthetic network on the synthetic clouds leaves
the arg-max tables and the forward-built hit lists of conv3 of both T-Nets and of conv5 in the workspace (read out by name:
geoa3_debug_pointnet_workspace_layout); they are copied and the three kernels are launched on the copies through
geoa3_debug_wide_bwd_conv, with the forward's lists (PRE, what the loop runs):
  t64     wide_bwd_conv_kernel<1, true>        T-Net 64's conv3 (one tap) + its 128 -> 64 layer
  first   wide_bwd_conv_first_kernel<true>     T-Net 3's conv3 + 128 -> 64 + the first layer's backward into dx
  conv5   wide_bwd_conv_kernel<3, true>        the trunk's conv5 (three taps) + its 128 -> 64 layer
Upstream gradients, weights and gate bits are random (seeded): they change no address and no trip count.
Device events around `iters` calls after warm-up; `windows` such windows per kernel and build, the builds alternated window
by window.  Reported per kernel and build: every window, minimum and range (us per call); and the same for the sum of the
three.  The outputs of the builds are compared bit for bit."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from geoa3_amd import _lib  # noqa: E402
from geoa3_amd.data import synthetic_clouds, synthetic_state_dict  # noqa: E402
from geoa3_amd.pointnet import PointNet, pack_wide_split  # noqa: E402

B, N = 250, 1024


def P(t):
    return None if t is None else t.data_ptr()


def loop_state(dev):
    """(arg, hits, hoff) of the three layers after one forward + backward, and the clouds"""
    lib = _lib.load()
    net = PointNet(40)
    net.load_state_dict(synthetic_state_dict(40, seed=0, device=dev))
    net = net.to(dev).eval()
    ori, _ = synthetic_clouds(B, N, seed=100)
    x = ori.to(dev).clone().requires_grad_()
    (net(x) * torch.randn(B, 40, device=dev, generator=torch.Generator(dev).manual_seed(1))).sum().backward()
    torch.cuda.synchronize()
    ws = net._ws_cache["ws"]
    names, offs = (C.c_char_p * 64)(), (C.c_int64 * 64)()
    n = lib.geoa3_debug_pointnet_workspace_layout(B, N, 40, names, offs, 64)
    at = {names[i].decode(): offs[i] for i in range(n)}

    def read(name, *shape):
        count = 1
        for s in shape:
            count *= s
        return ws[at[name]:at[name] + 4 * count].view(torch.int32).view(*shape).clone()

    out = {}
    for key, arg_n, hl, ho, taps in (("t64", "iq3", "hlq", "hoq", 1), ("first", "i3", "hl3", "ho3", 1), ("conv5", "i5", "hl5", "ho5", 3)):
        out[key] = dict(taps=taps, arg=read(arg_n, B, 1024), hits=read(hl, B, 1024 * taps), hoff=read(ho, B, N + 1))
    return out, x.detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="*", default=[_lib.LIB_PATH])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_wide_bwd.py measures on the GPU"
    dev = torch.device("cuda")
    state, x3 = loop_state(dev)
    gen = torch.Generator(dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)
    bits = lambda *s: torch.randint(-2 ** 62, 2 ** 62, s, device=dev, generator=gen, dtype=torch.int64)
    W2t = rn(64, 128) * 0.1
    w2th, uns = pack_wide_split(W2t.cpu())
    w2th = w2th.to(dev)
    w1, b1 = rn(64, 3), rn(64) * 0.5
    tiles = (N + 63) // 64
    m128, m64 = bits(B, tiles, 128), bits(B, tiles, 64)
    g = rn(B, 1024)
    stream = torch.cuda.current_stream().cuda_stream
    fns = []
    for path in a.libs:
        lib = C.CDLL(os.path.abspath(path))
        fn = lib.geoa3_debug_wide_bwd_conv
        fn.restype, fn.argtypes = _lib.SIGNATURES["geoa3_debug_wide_bwd_conv"]
        fns.append(fn)
    kernels = {}
    for key, st in state.items():
        W = rn(1024, 128 * st["taps"]) * 0.05
        first = key == "first"
        out0 = rn(B, 3, N) if first else None

        def call(fn, out, st=st, W=W, first=first):
            extra = (None, None, P(x3), P(w1), P(b1), P(out)) if first else (P(m64), P(out), None, None, None, None)
            rc = fn(P(g), P(st["arg"]), P(W), P(m128), P(W2t), P(w2th), uns, *extra, P(st["hits"]), P(st["hoff"]), B, N,
                    st["taps"], stream)
            assert rc == 0, (key, rc)

        kernels[key] = (call, out0)
    lines = ["sparse arg-max backward kernels alone, B=%d N=%d, forward-built lists of the loop's state; us per call, %d windows of %d "
             "calls, builds alternated" % (B, N, a.windows, a.iters)]
    lines += ["build %d: %s" % (i, p) for i, p in enumerate(a.libs)]
    t = {(k, i): [] for k in kernels for i in range(len(fns))}
    for key, (call, out0) in kernels.items():
        outs = []
        for fn in fns:     # the builds' outputs, bit for bit (the first-layer form adds into its output: same prefill)
            out = out0.clone() if out0 is not None else torch.full((B, 64, N), float("nan"), device=dev)
            call(fn, out)
            outs.append(out)
        torch.cuda.synchronize()
        same = all(torch.equal(outs[0], o) for o in outs[1:])
        lines.append("%-6s outputs of the builds equal bit for bit: %s" % (key, same))
        assert same, key
        out = outs[0]
        for fn in fns:
            for _ in range(20):
                call(fn, out)
        torch.cuda.synchronize()
        for _ in range(a.windows):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    call(fn, out)
                e1.record()
                torch.cuda.synchronize()
                t[(key, i)].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    fmt = lambda v: "min %7.2f  range %7.2f .. %7.2f   windows %s" % (min(v), min(v), max(v), " ".join("%.2f" % x for x in v))
    for key in kernels:
        for i in range(len(fns)):
            lines.append("%-6s build %d  %s" % (key, i, fmt(t[(key, i)])))
    for i in range(len(fns)):
        tot = [sum(t[(k, i)][w] for k in kernels) for w in range(a.windows)]
        lines.append("%-6s build %d  %s" % ("sum", i, fmt(tot)))
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
