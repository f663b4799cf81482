"""A float64 torch restatement of the reference's uniform_loss (Lib/loss_utils.py:151-189) for sizes the fixture cannot
hold: the indices come from the CPU oracle's sampler and ball query (oracle.pointnet2_oracle, the extension's rules) or
are handed in, the group K-NN selects with oracle.geoa3_oracle.knn_points on the float32 coordinates (its tie rule), and
the value and its gradient are formed in float64 by autograd on the device of `x`."""
import math

import torch

from oracle import geoa3_oracle as O
from oracle import pointnet2_oracle as P2

PCTS = (0.004, 0.006, 0.008, 0.010, 0.012)


def indices(x, percentages=PCTS, radius=1.0, contract=False):
    """x [B,3,N] float32 -> (fps [B,npoint], [ball-query rows [B,npoint,nsample_p] per percentage]) by the oracle."""
    B, _, N = x.shape
    pm = x.detach().cpu().float().permute(0, 2, 1).contiguous()
    npoint = int(N * 0.05)
    fps = P2.furthest_point_sampling(pm, npoint, contract=contract).long()
    centres = torch.gather(pm, 1, fps.unsqueeze(-1).expand(B, npoint, 3))
    rows = [P2.ball_query(centres, pm, math.sqrt(p * 4 * radius), int(N * (p * 4)), contract=contract).long()
            for p in percentages]
    return fps, rows


def uniform_ref(x, percentages=PCTS, radius=1.0, k=2, idx=None, chunk=4096):
    """x [B,3,N] -> (U float64 [], dU/dx float64 [B,3,N]); idx = (fps, rows) of indices() or of the device entry points."""
    B, _, N = x.shape
    fps, rows = idx if idx is not None else indices(x, percentages, radius)
    dev = x.device
    x64 = x.detach().to(dev, torch.float64).requires_grad_()
    x32 = x.detach().float()
    npoint = int(N * 0.05)
    total = 0.0
    for p, row in zip(percentages, rows):
        p = p * 4
        nsample = int(N * p)
        expect_len = float(torch.tensor(math.pi * (radius ** 2) * p / nsample, dtype=torch.float32).sqrt())
        row = row.to(dev).long().reshape(B, npoint * nsample)
        g64 = torch.gather(x64, 2, row.unsqueeze(1).expand(B, 3, -1)).view(B, 3, npoint, nsample)
        g32 = torch.gather(x32, 2, row.unsqueeze(1).expand(B, 3, -1)).view(B, 3, npoint, nsample)
        g64 = g64.permute(0, 2, 3, 1).reshape(B * npoint, nsample, 3)
        g32 = g32.permute(0, 2, 3, 1).reshape(B * npoint, nsample, 3)
        terms = []
        for s in range(0, B * npoint, chunk):
            _, nn_idx = O.knn_points(g32[s:s + chunk], g32[s:s + chunk], k + 1)
            a, bq = g64[s:s + chunk], g64[s:s + chunk]
            nb = O.knn_gather(bq, nn_idx[:, :, 1:])                          # [c,ns,k,3]
            d = ((a.unsqueeze(2) - nb) ** 2).sum(-1)
            u = torch.sqrt(torch.abs(d) + 1e-12).mean(-1)
            terms.append(((u - expect_len) ** 2 / (expect_len + 1e-12)).reshape(-1))
        total = total + torch.cat(terms).mean() * (p * 100) ** 2
    loss = total / len(percentages)
    (g,) = torch.autograd.grad(loss, x64)
    return loss.detach(), g


NEAR_TIE = 8 * 2.0 ** -24


def uniform_ref_parts(x, percentages=PCTS, radius=1.0, k=2, idx=None, cells=1 << 22):
    """uniform_ref with the gradient written out pair by pair (no autograd), and what a per-element error bound of the
    kernel needs.  -> dict:
      loss   float64 [],  grad  float64 [B,3,N]      (== uniform_ref's)
      n      int64 [B,N]: the pair terms a cloud point receives per coordinate (one fixed-point add each): a (row, neighbour)
             pair with d != 0 gives one to the row's point and one to the neighbour's
      A      float64 [B,3,N]: the sum over those pairs of the pair term's magnitude with |u - e| replaced by u + e (the
             float32 error of u - e is relative to u + e, not to the difference)
      near   int64 [M,3]: (percentage, group row, slot) of every row whose selection could go either way in float32.  The
             group's slots are sorted by the float64 distance of the float32 coordinates (equal ones by slot); the K-th of
             them is the last one kept.  The row is a near-tie when the next slot BEHIND it that holds other coordinates
             is closer to it than 8 * 2^-24 of the distance.  Slots with the K-th slot's own coordinates are stepped over:
             copies of a padded point (same destination) and repeated cloud points have float32 distances of the same
             bits, so the tie rule decides among them on both sides."""
    B, _, N = x.shape
    fps, rows = idx if idx is not None else indices(x, percentages, radius)
    dev = x.device
    x64 = x.detach().to(dev, torch.float64)
    x32 = x.detach().float()
    npoint, K, P = int(N * 0.05), k + 1, len(percentages)
    grad = torch.zeros(B * N, 3, dtype=torch.float64, device=dev)
    A = torch.zeros_like(grad)
    n = torch.zeros(B * N, dtype=torch.int64, device=dev)
    total, near = 0.0, []
    for pi, (p, row) in enumerate(zip(percentages, rows)):
        p = p * 4
        ns = int(N * p)
        e = float(torch.tensor(math.pi * (radius ** 2) * p / ns, dtype=torch.float32).sqrt())
        scale = (p * 100) ** 2
        w = scale / (P * B * npoint * ns)
        row = row.to(dev).long().reshape(B * npoint, ns)
        dest = row + (torch.arange(B, device=dev).repeat_interleave(npoint) * N).unsqueeze(1)      # [R,ns] into [B N]
        pts64, pts32 = x64.permute(0, 2, 1).reshape(B * N, 3), x32.permute(0, 2, 1).reshape(B * N, 3)
        tsum = torch.zeros((), dtype=torch.float64, device=dev)
        chunk = max(1, cells // (ns * ns))
        for s in range(0, B * npoint, chunk):
            dst = dest[s:s + chunk]
            a, a32 = pts64[dst], pts32[dst]                                   # [c,ns,3]
            _, nn = O.knn_points(a32, a32, K)
            if ns > K:
                d = sum((a[:, :, None, c] - a[:, None, :, c]) ** 2 for c in range(3))
                dv, di = torch.sort(d, dim=2, stable=True)
                lo = dv[:, :, K - 1]
                last = torch.gather(a, 1, di[:, :, K - 1:K].expand(-1, -1, 3))            # [c,ns,3]: the K-th slot's point
                other = (a[:, None, :, :] != last[:, :, None, :]).any(-1)                 # [c,row,slot]: other coordinates
                behind = torch.gather(other, 2, di)                                       # ... in sorted order
                behind[:, :, :K] = False
                hi = torch.where(behind, dv, torch.full_like(dv, float("inf"))).min(2)[0]  # (inf: nothing else in the group)
                hit = (torch.isfinite(hi) & (hi - lo <= NEAR_TIE * hi)).nonzero()
                if hit.numel():
                    near.append(torch.cat([torch.full_like(hit[:, :1], pi), hit[:, :1] + s, hit[:, 1:]], 1))
            nb = O.knn_gather(a, nn[:, :, 1:])                               # [c,ns,K-1,3]
            nd = torch.gather(dst, 1, nn[:, :, 1:].reshape(dst.shape[0], -1)).view(-1, ns, K - 1)
            dv3 = a.unsqueeze(2) - nb
            d = (dv3 ** 2).sum(-1)
            sq = torch.sqrt(torch.abs(d) + 1e-12)
            u = sq.mean(-1)
            tsum = tsum + ((u - e) ** 2 / (e + 1e-12)).sum()
            live = d != 0
            base = w * 2.0 / (e + 1e-12) / (K - 1) / sq * live                # times (u - e): d U / d d_q * 2
            t = ((u - e).unsqueeze(-1) * base).unsqueeze(-1) * dv3
            ta = ((u + e).unsqueeze(-1) * base).unsqueeze(-1) * dv3.abs()
            me = dst.unsqueeze(-1).expand_as(nd)
            for c in range(3):
                grad[:, c].index_add_(0, me.reshape(-1), t[..., c].reshape(-1))
                grad[:, c].index_add_(0, nd.reshape(-1), -t[..., c].reshape(-1))
                A[:, c].index_add_(0, me.reshape(-1), ta[..., c].reshape(-1))
                A[:, c].index_add_(0, nd.reshape(-1), ta[..., c].reshape(-1))
            cnt = live.reshape(-1).long()
            n.index_add_(0, me.reshape(-1), cnt)
            n.index_add_(0, nd.reshape(-1), cnt)
        total = total + tsum / (B * npoint * ns) * scale
    near = torch.cat(near).cpu() if near else torch.zeros(0, 3, dtype=torch.int64)
    return dict(loss=total / P, grad=grad.view(B, N, 3).permute(0, 2, 1).contiguous(), n=n.view(B, N),
                A=A.view(B, N, 3).permute(0, 2, 1).contiguous(), near=near)
