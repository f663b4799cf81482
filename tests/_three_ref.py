"""numpy restatement of the three feature-propagation functions of `pointnet2_ops._ext` (interpolate_gpu.cu:9-154)  --
TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Written from the semantics, not from the kernels:

    three_nn                 every unknown point scans known k = 0 .. m-1 in order and keeps the three smallest float32
                             squared distances with the strict `<` cascade (ties ascending in index; NaN / +inf never
                             selected; unfilled slots (+inf, 0))
    three_interpolate        (p[i1] * w1 + p[i2] * w2) + p[i3] * w3 in float32, or fmaf(p3, w3, fmaf(p2, w2, p1 * w1))
    three_interpolate_grad64 the scatter sum in float64, with the contributor count and sum |g * w| per element (the terms
                             of the float32 summation bound)
    three_interpolate_grad32 the scatter sum as the library promises it: sequential in float32 from +0.0, in ascending
                             entry number e = 3 j + slot, each product rounded

numpy arrays in, numpy arrays out; the `*_t` forms take and return torch CPU tensors (what the golden generator registers
as the missing attributes of the `pointnet2_ops._ext` stand-in).
"""
from __future__ import annotations

import numpy as np

from oracle.pointnet2_oracle import _fmaf32, _sq3_arrays


def three_nn(unknown, known, contract: bool = False):
    """unknown [B,n,3], known [B,m,3] float32 -> dist2 [B,n,3] float32, idx [B,n,3] int32"""
    unknown = np.ascontiguousarray(unknown, dtype=np.float32)
    known = np.ascontiguousarray(known, dtype=np.float32)
    B, n, _ = unknown.shape
    m = known.shape[1]
    best = np.full((3, B, n), np.inf, dtype=np.float32)
    besti = np.zeros((3, B, n), dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(m):
            p = known[:, k:k + 1, :]                                   # [B,1,3]
            d = _sq3_arrays(unknown[..., 0] - p[..., 0], unknown[..., 1] - p[..., 1], unknown[..., 2] - p[..., 2], contract)
            c1 = d < best[0]
            c2 = ~c1 & (d < best[1])
            c3 = ~c1 & ~c2 & (d < best[2])
            s12 = c1 | c2
            best[2] = np.where(s12, best[1], np.where(c3, d, best[2]))
            besti[2] = np.where(s12, besti[1], np.where(c3, k, besti[2]))
            best[1] = np.where(c1, best[0], np.where(c2, d, best[1]))
            besti[1] = np.where(c1, besti[0], np.where(c2, k, besti[1]))
            best[0] = np.where(c1, d, best[0])
            besti[0] = np.where(c1, k, besti[0])
    return np.ascontiguousarray(best.transpose(1, 2, 0)), np.ascontiguousarray(besti.transpose(1, 2, 0))


def three_interpolate(points, idx, weight, contract: bool = False):
    """points [B,C,m] float32, idx [B,n,3] int, weight [B,n,3] float32 -> [B,C,n] float32"""
    f = np.float32
    points = np.asarray(points, dtype=f)
    weight = np.asarray(weight, dtype=f)
    idx = np.asarray(idx).astype(np.int64)
    B, C, m = points.shape
    p = [np.take_along_axis(points, np.broadcast_to(idx[:, None, :, s], (B, C, idx.shape[1])), axis=2) for s in range(3)]
    w = [weight[:, None, :, s] for s in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        if contract:
            return _fmaf32(p[2], w[2], _fmaf32(p[1], w[1], (p[0] * w[0]).astype(f)))
        s = ((p[0] * w[0]).astype(f) + (p[1] * w[1]).astype(f)).astype(f)
        return (s + (p[2] * w[2]).astype(f)).astype(f)


def three_interpolate_grad64(grad_out, idx, weight, m: int):
    """grad_out [B,C,n], idx / weight [B,n,3] -> (grad_points [B,C,m] float64, count [B,1,m] int64, sum |g * w| [B,C,m]
    float64)"""
    g = np.asarray(grad_out, dtype=np.float64)
    w = np.asarray(weight, dtype=np.float64)
    idx = np.asarray(idx).astype(np.int64)
    B, C, n = g.shape
    out = np.zeros((B, C, m), dtype=np.float64)
    mag = np.zeros((B, C, m), dtype=np.float64)
    cnt = np.zeros((B, 1, m), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for s in range(3):
                t = g[b] * w[b, None, :, s]                            # [C,n]
                for c in range(C):
                    np.add.at(out[b, c], idx[b, :, s], t[c])
                    np.add.at(mag[b, c], idx[b, :, s], np.abs(t[c]))
                np.add.at(cnt[b, 0], idx[b, :, s], 1)
    return out, cnt, mag


def three_interpolate_grad32(grad_out, idx, weight, m: int, descending: bool = False):
    """grad_out [B,C,n], idx / weight [B,n,3] -> grad_points [B,C,m] float32: the sum the library promises, bit for bit.
    A float32 loop over the entries e = 3 j + slot in ascending order, from +0.0:
    out[b,:,i] = fl(out[b,:,i] + fl(g[b,:,j] * w[b,e])); an entry whose index is outside [0, m) is dropped.
    `descending` walks the same entries backwards (tests only: what a wrong order does to the bits)."""
    f = np.float32
    g = np.asarray(grad_out, dtype=f)
    B, C, n = g.shape
    w = np.asarray(weight, dtype=f).reshape(B, 3 * n)
    idx = np.asarray(idx).astype(np.int64).reshape(B, 3 * n)
    out = np.zeros((B, C, m), dtype=f)
    entries = range(3 * n - 1, -1, -1) if descending else range(3 * n)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            for e in entries:
                i = idx[b, e]
                if 0 <= i < m:
                    out[b, :, i] = out[b, :, i] + g[b, :, e // 3] * w[b, e]     # float32 arrays: each operation rounds once
    return out


# ---- torch CPU forms with the signatures of interpolate.cpp (for the golden generator)
def three_nn_t(unknown, known):
    import torch
    d, i = three_nn(unknown.detach().numpy(), known.detach().numpy())
    return torch.from_numpy(d), torch.from_numpy(i)


def three_interpolate_t(points, idx, weight):
    import torch
    return torch.from_numpy(three_interpolate(points.detach().numpy(), idx.detach().numpy(), weight.detach().numpy()))


def three_interpolate_grad_t(grad_out, idx, weight, m):
    import torch
    out, _, _ = three_interpolate_grad64(grad_out.detach().numpy(), idx.detach().numpy(), weight.detach().numpy(), int(m))
    return torch.from_numpy(out.astype(np.float32))
