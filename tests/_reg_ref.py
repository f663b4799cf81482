"""A torch restatement (CPU, any float dtype; the tests use float64) of the neighbour-based regularisers of the reference's
Lib/loss_utils.py:99-149, for sizes the fixture cannot hold.  tests/test_reg_ref.py pins it to
tests/golden/geoa3_golden_reg.npz, which holds what the reference's own functions returned.

All clouds are [b,3,n].  Neighbours: dense squared distances ((a.unsqueeze(3) - a.unsqueeze(2))**2).sum(1), the k + 1
smallest per row, column 0 dropped.  stable=True orders equal distances by ascending index (the K-NN's tie rule);
stable=False takes torch.topk (faster; enough for the functions that read distances only)."""
from __future__ import annotations

import torch


def knn_self(pc, K, stable=True):
    """-> (dists [b,n,K] ascending, differentiable; idx [b,n,K])"""
    d = ((pc.unsqueeze(3) - pc.unsqueeze(2)) ** 2).sum(1)
    if stable:
        idx = torch.sort(d.detach(), dim=2, stable=True)[1][:, :, :K].contiguous()
    else:
        idx = torch.topk(d.detach(), K, dim=2, largest=False, sorted=True)[1]
    return torch.gather(d, 2, idx), idx


def smoothing_parts(pc, k, threshold_coef=1.05, stable=True):
    """-> (s [b,n], thr [b], cond [b,n] bool) of kNN_smoothing_loss"""
    d, _ = knn_self(pc, k + 1, stable)
    s = d[:, :, 1:].mean(-1)
    thr = s.mean(-1) + threshold_coef * s.std(-1)
    return s, thr, s > thr.unsqueeze(1)


def kNN_smoothing_loss(adv_pc, k, threshold_coef=1.05, stable=True):
    s, _, c = smoothing_parts(adv_pc, k, threshold_coef, stable)
    return (s * c.to(s.dtype)).mean(1)


def repulsion_loss(pc, k=4, h=0.03, stable=True):
    d = knn_self(pc, k + 1, stable)[0][:, :, 1:]
    return -(d * torch.exp(-(d ** 2) / (h ** 2))).mean(2)


def displacement_loss(adv_pc, ori_pc, k=16):
    b, _, n = adv_pc.shape
    idx = knn_self(ori_pc.detach(), k + 1)[1][:, :, 1:]
    theta = ((adv_pc - ori_pc) ** 2).sum(1)
    nn = torch.gather(theta, 1, idx.reshape(b, n * k)).view(b, n, k)
    return ((nn - theta.unsqueeze(2)) ** 2).mean(2)


def corresponding_normal_loss(adv_pc, normal, k=2):
    b, _, n = adv_pc.shape
    idx = knn_self(adv_pc.detach(), k + 1)[1][:, :, 1:]
    nn_pts = torch.gather(adv_pc, 2, idx.reshape(b, 1, n * k).expand(b, 3, n * k)).view(b, 3, n, k)
    vec = nn_pts - adv_pc.unsqueeze(3)
    vec = vec / vec.norm(2, 1, keepdim=True).clamp(min=1e-12).expand_as(vec)
    return torch.abs((vec * normal.unsqueeze(3)).sum(1)).mean(2)


def value_and_grad(fn, x, g, *rest, **kw):
    """fn(x, *rest, **kw) and d (sum g . out) / d x"""
    x = x.detach().clone().requires_grad_()
    out = fn(x, *rest, **kw)
    (gx,) = torch.autograd.grad(out, x, g.to(out.dtype))
    return out.detach(), gx
