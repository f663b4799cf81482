"""Plain torch restatements (CPU; the tests use float64) of what each kernel of the PointNet backward computes, one
function per kernel, and the inputs of the cases tests/test_gpu_pointnet_bwd.py runs.  No project code.
tests/test_pointnet_bwd_ref.py pins every restatement to torch autograd of the forward it differentiates.

Every restatement returns (value, mag): mag[entry] = the sum of the absolute values of the products behind that entry
(nested sums: the absolute values all the way down), the quantity a rounding bound scales with.  The keyword arguments
named skip_* / omit_* / zero_* restate a DEFECTIVE kernel (one term, column or partial sum lost); the sensitivity tests use
them to show that the bound of a case would notice.

Shapes: clouds [B,3,N], activations [B,C,N], gates bool of the activation's shape, arg [B,1024] (long), W [1024, taps*128]
with k = tap*128 + ci.
"""
from __future__ import annotations

import math

import torch

U24 = 2.0 ** -24


def tolerance(ref, mag, n, c=4.0, extra=0.0):
    """|got - ref| <= c sqrt(n) 2^-24 mag + 2^-22 |ref| (+ extra * mag): n = terms in the longest sum behind an entry."""
    return (c * math.sqrt(n) * U24 + extra) * mag + 2.0 ** -22 * ref.abs()


def worst_ratio(got, ref, tol):
    """max err / tol; an entry with tol == 0 (ref and every product behind it zero) must be exactly zero."""
    err = (got.double() - ref.double()).abs()
    if not torch.isfinite(err).all():
        return float("inf")
    zero = tol <= 0
    if bool((err[zero] > 0).any()):
        return float("inf")
    return float((err[~zero] / tol[~zero]).max()) if bool((~zero).any()) else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# gate bits and hit lists
# ---------------------------------------------------------------------------------------------------------------------
def pack_gate_bits(gate, tail_ones=True):
    """bool [B,C,N] -> int64 words [B, ceil(N/64), C]: bit j of word (w, row) = gate[b, row, 64 w + j]; the bits of the last
    word beyond N are set when tail_ones (they must not leak into any result)."""
    B, C, N = gate.shape
    T = (N + 63) // 64
    pad = torch.full((B, C, T * 64), bool(tail_ones), dtype=torch.bool)
    pad[:, :, :N] = gate
    sh = torch.arange(64, dtype=torch.int64)
    words = (pad.view(B, C, T, 64).to(torch.int64) << sh).sum(-1)      # distinct bits: the sum is the OR (bit 63 wraps)
    return words.permute(0, 2, 1).contiguous()


def build_hits(arg, live, N, taps):
    """The hit lists of include/geoa3_hip_debug.h from arg [B,1024] and live [B,1024] (pooled output > 0):
    -> hits [B, 1024*taps] int32 (unused slots -1), hoff [B, N+1] int32."""
    B, Co = arg.shape
    hits = torch.full((B, Co * taps), -1, dtype=torch.int32)
    hoff = torch.zeros(B, N + 1, dtype=torch.int32)
    co = torch.arange(Co).repeat_interleave(taps)
    tap = torch.arange(taps).repeat(Co)
    for b in range(B):
        m = arg[b].long()[co] + tap - taps // 2
        ok = live[b][co] & (m >= 0) & (m < N)
        key = ((m * (Co // 64) + co // 64) * taps + tap) * Co + co
        order = torch.argsort(key[ok])
        ent = ((co * taps + tap) | (m << 16))[ok][order]
        hits[b, :ent.numel()] = ent.to(torch.int32)
        cnt = torch.bincount(m[ok], minlength=N)
        hoff[b, 1:] = torch.cumsum(cnt, 0).to(torch.int32)
    return hits, hoff


def share_starts(hits, hoff, b, tile, N):
    """(co, tap, m) of the first entry of each of the eight waves' shares of a 64-column tile's list (the kernels cut the
    tile's list into eight equal shares of ceil(total / 8) entries)."""
    h0, h1 = int(hoff[b, tile * 64]), int(hoff[b, min(tile * 64 + 64, N)])
    tot = h1 - h0
    per = (tot + 7) // 8
    out = []
    for w in range(8):
        lo = min(tot, w * per)
        if lo < min(tot, lo + per):
            out.append(int(hits[b, h0 + lo]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the sparse arg-max backward of a 1024-wide layer, alone and with the 128 -> 64 layer behind it
# ---------------------------------------------------------------------------------------------------------------------
def wide_bwd(g, arg, W, gate128, taps, skip_entries=(), zero_cols=()):
    """dX[b][ci][m] = gate128 * sum_{co,tap: arg + tap - taps/2 == m} W[co][tap*128 + ci] g[b][co].
    skip_entries: (b, co, tap) terms left out; zero_cols: (b, m) columns whose whole sum is lost."""
    B, _, N = gate128.shape
    dt = W.dtype
    dX = torch.zeros(B, 128, N, dtype=dt)
    mag = torch.zeros(B, 128, N, dtype=dt)
    keep = torch.ones(B, 1024, taps, dtype=torch.bool)
    for (b, co, tap) in skip_entries:
        keep[b, co, tap] = False
    for b in range(B):
        for tap in range(taps):
            m = arg[b].long() + tap - taps // 2
            ok = (m >= 0) & (m < N) & keep[b, :, tap]
            term = (W[ok, tap * 128:(tap + 1) * 128] * g[b, ok].to(dt).unsqueeze(1)).t()      # [128, hits]
            dX[b].index_add_(1, m[ok], term)
            mag[b].index_add_(1, m[ok], term.abs())
    for (b, m) in zero_cols:
        dX[b, :, m] = 0
    gt = gate128.to(dt)
    return dX * gt, mag * gt


def column_terms(g, arg, N, taps):
    """the largest number of non-zero terms in one column's sum"""
    most = 0
    for b in range(arg.shape[0]):
        for_cols = torch.zeros(N, dtype=torch.long)
        for tap in range(taps):
            m = arg[b].long() + tap - taps // 2
            ok = (m >= 0) & (m < N) & (g[b] != 0)
            for_cols += torch.bincount(m[ok], minlength=N)
        most = max(most, int(for_cols.max()))
    return most


def wide_bwd_conv(g, arg, W, gate128, taps, W2t, gate64, **defects):
    """dY[b][o][n] = gate64 * sum_ci W2t[o][ci] dX[b][ci][n], dX as wide_bwd"""
    dX, magX = wide_bwd(g, arg, W, gate128, taps, **defects)
    gt = gate64.to(W.dtype)
    return torch.einsum("oc,bcn->bon", W2t, dX) * gt, torch.einsum("oc,bcn->bon", W2t.abs(), magX) * gt


def first_layer_pre(x3, w1, b1, T3=None):
    """(pre, scale): pre[b][k][n] = w1[k] . p + b1[k] with p = T3^T x (p = x without T3); scale = |w1| . |p| + |b1| with
    |p| bounded by |T3|^T |x| -- the magnitude the rounding of the fp32 evaluation of pre scales with."""
    if T3 is None:
        p, pa = x3, x3.abs()
    else:
        p = torch.einsum("bdc,bdn->bcn", T3, x3)
        pa = torch.einsum("bdc,bdn->bcn", T3.abs(), x3.abs())
    pre = torch.einsum("kc,bcn->bkn", w1, p) + b1.view(1, -1, 1)
    scale = torch.einsum("kc,bcn->bkn", w1.abs(), pa) + b1.abs().view(1, -1, 1)
    return pre, scale


def gate_margin_ok(x3, w1, b1, T3=None):
    """The kernels recompute the first layer's gate in fp32: no pre-activation may lie within 2e-6 of its scale (about eight
    roundings of a three-term fp32 dot product) of zero, or float64 and the kernel could disagree on a gate."""
    pre, scale = first_layer_pre(x3.double(), w1.double(), b1.double(), None if T3 is None else T3.double())
    return bool((pre.abs() > 2e-6 * scale).all())


def wide_bwd_conv_first(g, arg, W, gate128, W2t, x3, w1, b1, dx3_in, gate_first=None, **defects):
    """first-layer form (taps = 1): dx3 = dx3_in + w1^T (gate_first * (W2t dX)), gate_first = (w1 x + b1 > 0)"""
    dX, magX = wide_bwd(g, arg, W, gate128, 1, **defects)
    if gate_first is None:
        gate_first = first_layer_pre(x3, w1, b1)[0] > 0
    gt = gate_first.to(W.dtype)
    y = torch.einsum("oc,bcn->bon", W2t, dX) * gt
    ymag = torch.einsum("oc,bcn->bon", W2t.abs(), magX) * gt
    return (dx3_in + torch.einsum("od,bon->bdn", w1, y),
            dx3_in.abs() + torch.einsum("od,bon->bdn", w1.abs(), ymag))


# ---------------------------------------------------------------------------------------------------------------------
# Gram product, backward chain, fully connected layer
# ---------------------------------------------------------------------------------------------------------------------
def gram(A, G, skip_cols=()):
    """P[b][i][o] = sum_n A[b][i][n] G[b][o][n]; skip_cols: (b, n) columns left out of the sum"""
    if skip_cols:
        A = A.clone()
        for (b, n) in skip_cols:
            A[b, :, n] = 0
    return torch.einsum("bin,bon->bio", A, G), torch.einsum("bin,bon->bio", A.abs(), G.abs())


def bwd_chain(Xa, Wa, Xb, Wb, gate_h2, W2t, x3, T3, w1, b1, gate_first=None, skip_k=None, zero_cols=(),
              omit_dt_block=None):
    """dh2 = gate_h2 (Wa[b]^T Xa + Wb^T Xb); g1 = gate_first (W2t dh2); q = w1^T g1; dx = T3 q; dT[d][c] = sum_n x[d][n] q[c][n];
    gate_first = (w1 (T3^T x) + b1 > 0).  -> (dx, mag_dx, dT, mag_dT).
    skip_k: row o of Xa left out of the first product; zero_cols: (b, n) columns lost (dx and their share of dT);
    omit_dt_block: (b, w) the sum over columns 256 w .. 256 w + 255 left out of dT."""
    dt = Xa.dtype
    B, _, N = Xa.shape
    if skip_k is not None:
        Xa = Xa.clone()
        Xa[:, skip_k] = 0
    if T3 is None:
        T3 = torch.eye(3, dtype=dt).expand(B, 3, 3)
    g2 = gate_h2.to(dt)
    dh2 = (torch.einsum("boi,bon->bin", Wa, Xa) + torch.einsum("oi,bon->bin", Wb, Xb)) * g2
    m = (torch.einsum("boi,bon->bin", Wa.abs(), Xa.abs()) + torch.einsum("oi,bon->bin", Wb.abs(), Xb.abs())) * g2
    if gate_first is None:
        gate_first = first_layer_pre(x3, w1, b1, T3)[0] > 0
    g1 = gate_first.to(dt)
    y = torch.einsum("ck,bkn->bcn", W2t, dh2) * g1
    m = torch.einsum("ck,bkn->bcn", W2t.abs(), m) * g1
    q = torch.einsum("kc,bkn->bcn", w1, y)
    mq = torch.einsum("kc,bkn->bcn", w1.abs(), m)
    for (b, n) in zero_cols:
        q[b, :, n] = 0
    dx = torch.einsum("bdc,bcn->bdn", T3, q)
    mdx = torch.einsum("bdc,bcn->bdn", T3.abs(), mq)
    qs, mqs = q, mq
    if omit_dt_block is not None:
        b, w = omit_dt_block
        qs, mqs = q.clone(), mq.clone()
        qs[b, :, 256 * w:256 * w + 256] = 0
    dT = torch.einsum("bdn,bcn->bdc", x3, qs)
    mdT = torch.einsum("bdn,bcn->bdc", x3.abs(), mqs)
    return dx, mdx, dT, mdT


def fc(X, W, bias=None, relu=False, Zgate=None, skip_k=None):
    """Y[m][o] = gate(relu?(sum_k X[m][k] W[o][k] + bias[o])); batched when X / W are 3-D.  skip_k: that k left out."""
    if skip_k is not None:
        X = X.clone()
        X[..., skip_k] = 0
    y = torch.einsum("...mk,...ok->...mo", X, W)
    mag = torch.einsum("...mk,...ok->...mo", X.abs(), W.abs())
    if bias is not None:
        y = y + bias
        mag = mag + bias.abs()
    if relu:
        y = y.clamp_min(0)
    if Zgate is not None:
        y = y * Zgate.to(y.dtype)
        mag = mag * Zgate.to(y.dtype)
    return y, mag
