"""An EdgeConv layer of DGCNN in TRAINING mode -- gather -> cat -> Conv2d(2C -> C', 1x1, no bias) -> BatchNorm2d(batch
statistics) -> LeakyReLU(0.2) -> max over the k neighbours -- as one torch.autograd.Function on the HIP kernels of
csrc/edgeconv_train.hip.  Neither the [B,2C,N,k] edge tensor nor a [B,C',N,k] tensor is written, forward or backward.

With W = [W_a | W_b] over the channels [x_j - x_i ; x_i], U0 = h W_a^T and V0 = h (W_b - W_a)^T are two torch matmuls per
point (autograd takes their gradients to h and W); edge (i, s), j = idx[i,s], has the pre-BatchNorm value z = U0[j] + V0[i].
The kernels take the batch statistics of z over the M = B N k edges, select per (point, channel) the neighbour the maximum
is reached at from the sign of gamma, and write y; the backward's formulas are in csrc/edgeconv_train.hip and
include/geoa3_hip.h.  There is no CPU path for mode "fused": a CPU tensor raises.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .pointnet_train import update_running_stats

Tensor = torch.Tensor
EDGE_TRAIN_MODES = ("fused", "torch")


class EdgeTrainFn(torch.autograd.Function):
    """(U0 [B,N,C'], V0 [B,N,C'], idx int64 [B,N,k], gamma [C'], beta [C'], eps) -> (y [B,C',N], mean [C'], var [C'],
    arg int32 [B,N,C']): y as `max(leaky_relu(batch_norm(U0[idx] + V0[:, :, None], training), 0.2), neighbours)`, mean / var
    the batch statistics over the B N k edges (var biased), arg the selected slot.  Gradients for U0, V0, gamma, beta."""

    @staticmethod
    def forward(ctx, U0: Tensor, V0: Tensor, idx: Tensor, gamma: Tensor, beta: Tensor, eps: float):
        if not U0.is_cuda:
            raise _lib.Geoa3Error("the fused train-mode EdgeConv layer runs on the GPU only (no CPU path)")
        B, N, _ = U0.shape
        if B * N * idx.shape[2] < 2:
            raise ValueError("Expected more than 1 value per channel when training, got %d edges" % (B * N * idx.shape[2]))
        U0, V0 = U0.detach().contiguous().float(), V0.detach().contiguous().float()
        gamma, beta = gamma.detach().contiguous().float(), beta.detach().contiguous().float()
        idx = idx.contiguous()
        y, arg, S1, mean, var, stats = ops.edge_train(U0, V0, idx, gamma, beta, float(eps))
        ctx.save_for_backward(U0, V0, idx, gamma, y, arg, S1, stats)
        ctx.mark_non_differentiable(mean, var, arg)
        return y, mean, var, arg

    @staticmethod
    def backward(ctx, g: Tensor, _gm, _gv, _ga):
        U0, V0, idx, gamma, y, arg, S1, stats = ctx.saved_tensors
        dU0, dV0, dgamma, dbeta = ops.edge_train_grad(g.contiguous().float(), y, U0, V0, arg, S1, idx, gamma, stats)
        return dU0, dV0, None, dgamma, dbeta, None


def split_edge_weight(conv: nn.Conv2d):
    """conv.weight [C',2C,1,1] over [x_j - x_i ; x_i] -> (W_a, W_b - W_a), both [C',C]: U0 = h W_a^T, V0 = h (W_b - W_a)^T"""
    w = conv.weight.view(conv.weight.shape[0], conv.weight.shape[1])
    c = w.shape[1] // 2
    return w[:, :c], w[:, c:] - w[:, :c]


def edge_tensor(h: Tensor, idx: Tensor) -> Tensor:
    """The public model's get_graph_feature on a given table: h [B,N,C], idx [B,N,k] -> [B,2C,N,k], channels [x_j - x_i ; x_i]"""
    B, N, C = h.shape
    k = idx.shape[2]
    nb = torch.gather(h, 1, idx.reshape(B, N * k, 1).expand(B, N * k, C)).view(B, N, k, C)
    ctr = h.view(B, N, 1, C).expand(B, N, k, C)
    return torch.cat((nb - ctr, ctr), 3).permute(0, 3, 1, 2).contiguous()


def edgeconv_train(h: Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, idx: Tensor, mode: str = "fused") -> Tensor:
    """One training-mode EdgeConv layer: h [B,N,C] point-major, idx int64 [B,N,k] -> y [B,C',N]; bn's running statistics are
    updated as nn.BatchNorm2d updates them (its own momentum, the unbiased variance M / (M - 1), num_batches_tracked + 1).
    mode 'fused': the HIP layer above; 'torch': the plain materialising composition (gather, cat, conv2d,
    batch_norm(training=True), leaky_relu, max), the on-device baseline and the fallback, in h's dtype.  Not differentiable
    in idx."""
    if mode == "torch":
        z = F.conv2d(edge_tensor(h, idx), conv.weight)
        m = 0.0
        if bn.track_running_stats and bn.running_mean is not None:
            bn.num_batches_tracked += 1
            m = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else float(bn.momentum)
        z = F.batch_norm(z, bn.running_mean if bn.track_running_stats else None,
                         bn.running_var if bn.track_running_stats else None, bn.weight, bn.bias, True, m, bn.eps)
        return F.leaky_relu(z, 0.2).max(-1)[0]
    if mode != "fused":
        raise ValueError("edge_train must be 'fused' or 'torch', got %r" % (mode,))
    wa, wd = split_edge_weight(conv)
    y, mean, var, _ = EdgeTrainFn.apply(torch.matmul(h, wa.t()), torch.matmul(h, wd.t()), idx, bn.weight, bn.bias, bn.eps)
    update_running_stats(bn, mean, var, h.shape[0] * h.shape[1] * idx.shape[2])
    return y
