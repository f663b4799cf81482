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
