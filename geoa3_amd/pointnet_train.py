"""The 1024-wide PointNet layers in TRAINING mode: conv(128 -> 1024, T taps) -> BatchNorm1d(batch statistics) -> [relu] -> max
over points as one torch.autograd.Function on the HIP kernels of csrc/pointnet_wide_train.hip (Model/PointNet.py:81-82 and
:146-147 under net.train()).  The [B,1024,N] activation is never written, forward or backward.

Kernels: the forward pass (statistics, selected point, output), the gather sum_b coef U[:, a] of dW, the ordered scatter of
coef W into dX.  The dense terms of the backward (S1, G = U U^T, the T*128-square and T*128 x 1024 products, the tap fold)
are torch operators ("Training").  There is no CPU path: a CPU tensor raises.

Notation (W [1024, T*128], k = tap*128 + ci; U the unfolded input; M = B*N; a[b,c] the selected point):
  dbeta = sum_b g~,  dgamma = sum_b g~ xhat_sel,  coef = g~ gamma / sigma,  k1 = gamma dbeta / (sigma M),
  k2 = gamma dgamma / (sigma^2 M),  m = mean(W U) (= mu - bias)
  dW = sum_b coef U[b,:,a] - k1 S1 - k2 (W G - m S1)
  dU = scatter(coef W) - (W^T diag(k2) W) U - W^T (k1 - k2 m),  dX = fold(dU),  d bias = 0
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import check

Tensor = torch.Tensor
WIDE_CO, WIDE_CI = 1024, 128


def unfold_taps(x: Tensor, taps: int) -> Tensor:
    """[B,128,N] -> U [B, taps*128, N]: U[b, tap*128 + ci, p] = x[b, ci, p + tap - taps//2], zero past the ends."""
    if taps == 1:
        return x
    N = x.shape[2]
    xp = F.pad(x, (taps // 2, taps // 2))
    return torch.cat([xp[:, :, t:t + N] for t in range(taps)], 1)


def fold_taps(dU: Tensor, taps: int) -> Tensor:
    """The transpose of unfold_taps: dX[b,i,q] = sum_t dU[b, t*128 + i, q - t + taps//2]."""
    if taps == 1:
        return dU
    N, h = dU.shape[2], taps // 2
    dX = torch.zeros_like(dU[:, :WIDE_CI])
    for t in range(taps):
        d = dU[:, t * WIDE_CI:(t + 1) * WIDE_CI]
        s = t - h                                    # q = p + s
        lo, hi = max(0, -s), min(N, N - s)           # the p range whose q lies in [0, N)
        if hi > lo:
            dX[:, :, lo + s:hi + s] += d[:, :, lo:hi]
    return dX


def tap_sums(x: Tensor, taps: int) -> Tensor:
    """S1 = sum_{b,p} U[b,:,p] [taps*128] without forming U: the row totals less the columns a tap never sees."""
    tot = x.sum((0, 2))
    if taps == 1:
        return tot
    out, N, h = [], x.shape[2], taps // 2
    for t in range(taps):
        s = t - h
        cut = x[:, :, :min(s, N)].sum((0, 2)) if s > 0 else (x[:, :, max(N + s, 0):].sum((0, 2)) if s < 0 else 0)
        out.append(tot - cut)
    return torch.cat(out)


def _workspace(B: int, N: int, taps: int, device) -> Tensor:
    nbytes = _lib.load().geoa3_wide_train_workspace_bytes(B, N, taps)
    if nbytes < 0:
        check(int(nbytes), "geoa3_wide_train_workspace_bytes")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


class WideTrainFn(torch.autograd.Function):
    """(x [B,128,N], w [1024, T*128], bias [1024], gamma, beta, eps, relu, taps) -> (out [B,1024], mean [1024], var [1024],
    arg [B,1024]): out as `max(relu(batch_norm(conv1d(x)), training), -1)`, mean / var the batch statistics of the conv
    output (var biased), arg the selected point (int32).  Gradients for x, w, bias (zeros), gamma, beta."""

    @staticmethod
    def forward(ctx, x: Tensor, w: Tensor, bias: Tensor, gamma: Tensor, beta: Tensor, eps: float, relu: bool, taps: int):
        if not x.is_cuda:
            raise _lib.Geoa3Error("the fused train-mode wide layer runs on the GPU only (no CPU path)")
        B, ci, N = x.shape
        if ci != WIDE_CI or tuple(w.shape) != (WIDE_CO, taps * WIDE_CI) or taps not in (1, 3):
            raise ValueError("wide train layer: x [B,128,N] and w [1024, taps*128] with taps 1 or 3 expected, got %s, %s"
                             % (tuple(x.shape), tuple(w.shape)))
        if B * N < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
        x, w = x.detach().contiguous().float(), w.detach().contiguous().float()
        gamma, beta = gamma.detach().contiguous().float(), beta.detach().contiguous().float()
        shift = torch.mv(w, tap_sums(x, taps) / float(B * N)).contiguous()
        out = torch.empty(B, WIDE_CO, device=x.device, dtype=torch.float32)
        xhat = torch.empty_like(out)
        arg = torch.empty(B, WIDE_CO, device=x.device, dtype=torch.int32)
        mean = torch.empty(WIDE_CO, device=x.device, dtype=torch.float32)
        var = torch.empty_like(mean)
        ws = _workspace(B, N, taps, x.device)
        check(_lib.load().geoa3_wide_train_forward(
            x.data_ptr(), w.data_ptr(), shift.data_ptr(), gamma.data_ptr(), beta.data_ptr(), float(eps), int(bool(relu)),
            B, N, taps, out.data_ptr(), arg.data_ptr(), xhat.data_ptr(), mean.data_ptr(), var.data_ptr(), ws.data_ptr(),
            torch.cuda.current_stream().cuda_stream), "geoa3_wide_train_forward")
        ctx.save_for_backward(x, w, gamma, out, arg, xhat, mean, var)
        ctx.eps, ctx.relu, ctx.taps = float(eps), bool(relu), taps
        mean_y = mean + bias.detach().float()
        ctx.mark_non_differentiable(mean_y, var, arg)
        return out, mean_y, var, arg

    @staticmethod
    def backward(ctx, g: Tensor, _gm, _gv, _ga):
        x, w, gamma, out, arg, xhat, mean, var = ctx.saved_tensors
        taps, (B, _, N) = ctx.taps, x.shape
        M = float(B * N)
        lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
        g = g.contiguous().float()
        gt = g * (out > 0).to(g.dtype) if ctx.relu else g
        dbeta = gt.sum(0)
        dgamma = (gt * xhat).sum(0)
        inv = torch.rsqrt(var.double() + ctx.eps).float()
        coef = (gt * (gamma * inv)).contiguous()
        k1 = gamma * dbeta * inv / M
        k2 = gamma * dgamma * inv * inv / M
        K = taps * WIDE_CI
        dW = torch.empty(WIDE_CO, K, device=x.device, dtype=torch.float32)
        check(lib.geoa3_wide_train_gather(x.data_ptr(), coef.data_ptr(), arg.data_ptr(), B, N, taps, dW.data_ptr(), s),
              "geoa3_wide_train_gather")
        dX = torch.empty_like(x)
        check(lib.geoa3_wide_train_scatter(w.data_ptr(), coef.data_ptr(), arg.data_ptr(), B, N, taps, dX.data_ptr(), s),
              "geoa3_wide_train_scatter")
        U = unfold_taps(x, taps)
        Uf = U.permute(1, 0, 2).reshape(K, B * N)
        S1 = tap_sums(x, taps)
        G = Uf @ Uf.t()
        dW -= k1[:, None] * S1[None, :] + k2[:, None] * (w @ G - mean[:, None] * S1[None, :])
        P = w.t() @ (k2[:, None] * w)
        v = torch.mv(w.t(), k1 - k2 * mean)
        dX -= fold_taps(torch.matmul(P, U) + v[None, :, None], taps)
        return dX, dW, torch.zeros(WIDE_CO, device=x.device, dtype=torch.float32), dgamma, dbeta, None, None, None


def _conv_matrix(conv: nn.Conv1d) -> Tensor:
    """conv.weight [1024,128,T] -> [1024, T*128] with k = tap*128 + ci (the order of the wide kernels)"""
    return conv.weight.permute(0, 2, 1).reshape(conv.weight.shape[0], -1)


@torch.no_grad()
def update_running_stats(bn: nn.BatchNorm1d, mean: Tensor, var_biased: Tensor, count: int) -> None:
    """What nn.BatchNorm1d does to its buffers in a training forward: its own momentum (None: the cumulative average),
    the UNBIASED variance, num_batches_tracked + 1."""
    if not bn.track_running_stats or bn.running_mean is None:
        return
    bn.num_batches_tracked += 1
    m = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else float(bn.momentum)
    bn.running_mean.mul_(1.0 - m).add_(mean.to(bn.running_mean.dtype), alpha=m)
    bn.running_var.mul_(1.0 - m).add_(var_biased.to(bn.running_var.dtype) * (count / (count - 1.0)), alpha=m)


def wide_layer_train(x: Tensor, conv: nn.Conv1d, bn: nn.BatchNorm1d, relu: bool = True, mode: str = "fused") -> Tensor:
    """`max(relu(bn(conv(x))), -1)[0]` in training mode, [B,128,N] -> [B,1024]; bn's running statistics are updated.
    mode 'fused': the HIP layer above; 'torch': the plain composition (what the tests and tools/bench_train.py compare with)."""
    if mode == "torch":
        y = bn(conv(x))
        return (F.relu(y) if relu else y).max(-1)[0]
    if mode != "fused":
        raise ValueError("wide_train must be 'fused' or 'torch', got %r" % (mode,))
    taps = conv.kernel_size[0]
    bias = conv.bias if conv.bias is not None else torch.zeros(WIDE_CO, device=x.device)
    out, mean, var, _ = WideTrainFn.apply(x, _conv_matrix(conv), bias, bn.weight, bn.bias, bn.eps, relu, taps)
    update_running_stats(bn, mean, var, x.shape[0] * x.shape[2])
    return out
