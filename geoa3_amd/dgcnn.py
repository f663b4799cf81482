"""DGCNN (Wang et al., "Dynamic Graph CNN for Learning on Point Clouds", the classification model) as a victim: an
nn.Module with the parameter names of the public model, so published checkpoints load with `load_state_dict`, whose
EVAL-mode forward runs the dynamic-graph part in the HIP library:

    graph      knn_points(h, h, K=k) on each EdgeConv layer's own input (D = 3, 64, 64, 128: geoa3_knn / geoa3_knn_nd);
               the point itself is a neighbour; no gradient flows through the indices
    EdgeConv   max_k LeakyReLU_0.2(BN(W [x_j - x_i ; x_i])) with the BatchNorm folded on the host in float64 and W = [W_a | W_b]:
               U = (s W_a) x, V = (s (W_b - W_a)) x (two torch matmuls per point), then geoa3::edge_max -- the [B,2C,N,k]
               edge tensor never exists, and the backward (geoa3::edge_max_grad) sums in a fixed order
    conv5, pooling and the head: torch operators on the folded weights.

The training-mode forward (batch statistics, dropout) raises by default, as before; `net.edge_train = "fused"` or "torch"
turns it on: the four EdgeConv layers through geoa3_amd.dgcnn_train.edgeconv_train (the fused HIP layer of
csrc/edgeconv_train.hip, or the plain materialising torch composition), everything after them through the module's own torch
layers.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

Tensor = torch.Tensor

EDGE_LAYERS = ((6, 64), (128, 64), (128, 128), (256, 256))   # (2C, C') of conv1 .. conv4


def checkpoint_state_dict(obj) -> Dict[str, Tensor]:
    """The state_dict inside a loaded checkpoint: under 'state_dict' or 'model_state_dict', or the object itself; a
    `module.` prefix (a DataParallel save, what the public training script writes) is stripped."""
    sd = obj
    if isinstance(obj, dict):
        for key in ("state_dict", "model_state_dict"):
            if key in obj and isinstance(obj[key], dict):
                sd = obj[key]
                break
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def _bn_affine(bn: nn.modules.batchnorm._BatchNorm):
    """(scale, shift) in float64 of an eval-mode BatchNorm"""
    s = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return s, bn.bias.detach().double() - bn.running_mean.detach().double() * s


def fold_edgeconv(weight: Tensor, bn: nn.modules.batchnorm._BatchNorm):
    """An EdgeConv layer's Conv2d weight [C',2C,1,1] (channels [x_j - x_i ; x_i]) and eval-mode BatchNorm as the float64
    right-hand sides of U = h wa, V = h wd (both [C,C']) and the shift t [C']: the layer is max_j lrelu(U[j] + V[i] + t)."""
    s, t = _bn_affine(bn)
    w = weight.detach().double().view(weight.shape[0], weight.shape[1]) * s.view(-1, 1)
    c = w.shape[1] // 2
    return w[:, :c].t(), (w[:, c:] - w[:, :c]).t(), t


def edgeconv(h: Tensor, wa: Tensor, wd: Tensor, t: Tensor, idx: Tensor) -> Tensor:
    """One fused eval-mode EdgeConv layer: h [B,N,C] point-major, wa / wd [C,C'], t [C'] (fold_edgeconv, float32 on the
    device), idx int64 [B,N,k] -> y [B,C',N].  Differentiable in h, wa, wd, t; not in idx."""
    from . import library  # noqa: F401  (registers geoa3::edge_max with its autograd formula)
    y, _ = torch.ops.geoa3.edge_max(torch.matmul(h, wa), torch.matmul(h, wd), t, idx)
    return y


class DGCNN(nn.Module):
    """DGCNN(k=20, emb_dims=1024, dropout=0.5, output_channels=40): forward(x [B,3,N]) -> logits [B,output_channels] in
    eval mode.  graph_hook(layer, idx), if given, is called with every layer's neighbour table (int64 [B,N,k]); a tensor
    it returns takes the table's place.  edge_train (None | "fused" | "torch"): how a TRAINING-mode forward runs the EdgeConv
    layers; None, the default, refuses it."""

    edge_train = None       # (a class default: a module pickled before the attribute existed refuses training as it did)

    def __init__(self, k: int = 20, emb_dims: int = 1024, dropout: float = 0.5, output_channels: int = 40,
                 graph_hook: Optional[Callable[[int, Tensor], Optional[Tensor]]] = None):
        super().__init__()
        self.k = int(k)
        self.emb_dims = int(emb_dims)
        self.num_class = int(output_channels)
        self.bn1, self.bn2, self.bn3, self.bn4 = (nn.BatchNorm2d(c) for _, c in EDGE_LAYERS)
        self.bn5 = nn.BatchNorm1d(emb_dims)
        for i, (cin, cout) in enumerate(EDGE_LAYERS, 1):
            setattr(self, "conv%d" % i, nn.Sequential(nn.Conv2d(cin, cout, kernel_size=1, bias=False),
                                                      getattr(self, "bn%d" % i), nn.LeakyReLU(negative_slope=0.2)))
        self.conv5 = nn.Sequential(nn.Conv1d(512, emb_dims, kernel_size=1, bias=False), self.bn5,
                                   nn.LeakyReLU(negative_slope=0.2))
        self.linear1 = nn.Linear(emb_dims * 2, 512, bias=False)
        self.bn6 = nn.BatchNorm1d(512)
        self.dp1 = nn.Dropout(p=dropout)
        self.linear2 = nn.Linear(512, 256)
        self.bn7 = nn.BatchNorm1d(256)
        self.dp2 = nn.Dropout(p=dropout)
        self.linear3 = nn.Linear(256, output_channels)
        self.graph_hook = graph_hook
        self._folded = None
        self._folded_key = None

    @property
    def classes(self) -> int:
        return self.num_class

    def __getstate__(self):
        state = dict(self.__dict__)
        for name in ("_folded", "_folded_key"):
            state.pop(name, None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._folded, self._folded_key = None, None

    def load_state_dict(self, state_dict, *args, **kwargs):
        """nn.Module.load_state_dict; a `module.` prefix on the keys is stripped."""
        return super().load_state_dict(checkpoint_state_dict(state_dict), *args, **kwargs)

    def _weights_key(self, device):
        return (str(device),) + tuple((p.data_ptr(), p._version) for p in list(self.parameters()) + list(self.buffers()))

    def folded(self, device) -> Dict[str, Tensor]:
        """The eval-mode weights with every BatchNorm folded in (float64 on the host, float32 on `device`), cached per
        weight version: wa<l> / wd<l> [C,C'] (the right-hand sides of U = h wa, V = h wd), t<l> [C'], w5 [emb,512], t5,
        f1 [2 emb,512], fb1, f2 [512,256], fb2, f3 [256,classes], fb3."""
        key = self._weights_key(device)
        if self._folded is not None and key == self._folded_key:
            return self._folded
        out: Dict[str, Tensor] = {}
        for l in range(1, 5):
            conv = getattr(self, "conv%d" % l)
            out["wa%d" % l], out["wd%d" % l], out["t%d" % l] = fold_edgeconv(conv[0].weight, conv[1])
        s, out["t5"] = _bn_affine(self.conv5[1])
        out["w5"] = self.conv5[0].weight.detach().double().view(self.emb_dims, 512) * s.view(-1, 1)
        s, out["fb1"] = _bn_affine(self.bn6)
        out["f1"] = (self.linear1.weight.detach().double() * s.view(-1, 1)).t()
        s, t = _bn_affine(self.bn7)
        out["f2"] = (self.linear2.weight.detach().double() * s.view(-1, 1)).t()
        out["fb2"] = self.linear2.bias.detach().double() * s + t
        out["f3"], out["fb3"] = self.linear3.weight.detach().double().t(), self.linear3.bias.detach().double()
        self._folded = {n: v.float().contiguous().to(device) for n, v in out.items()}
        self._folded_key = key
        return self._folded

    def forward(self, x: Tensor) -> Tensor:
        assert x.dim() == 3 and x.size(1) == 3
        if self.training:
            if self.edge_train is None:
                raise NotImplementedError("only the eval-mode forward (the attack's victim) is implemented")
            return self.forward_train(x)
        if not x.is_cuda:
            raise RuntimeError("DGCNN.forward needs a device tensor: the graph search and the EdgeConv layers have no CPU path")
        w = self.folded(x.device)
        h = x.float().transpose(1, 2).contiguous()                   # [B,N,C] point-major: what the search and U / V take
        feats = []
        for l in range(1, 5):
            hd = h.detach()
            idx = ops.knn_points(hd, hd, K=self.k).idx
            if self.graph_hook is not None:
                other = self.graph_hook(l - 1, idx)
                if other is not None:
                    idx = other
            y = edgeconv(h, w["wa%d" % l], w["wd%d" % l], w["t%d" % l], idx)
            feats.append(y)                                         # [B,C',N]
            h = y.transpose(1, 2).contiguous()
        z = F.leaky_relu(torch.matmul(w["w5"], torch.cat(feats, 1)) + w["t5"].view(1, -1, 1), 0.2)
        z = torch.cat((z.max(2)[0], z.mean(2)), 1)
        z = F.leaky_relu(torch.matmul(z, w["f1"]) + w["fb1"], 0.2)
        z = F.leaky_relu(torch.matmul(z, w["f2"]) + w["fb2"], 0.2)
        return torch.matmul(z, w["f3"]) + w["fb3"]

    def forward_train(self, x: Tensor) -> Tensor:
        """The training-mode forward (batch statistics, running-statistics updates, dropout) under self.edge_train: the graph
        of every EdgeConv layer is the K-NN of its own detached input, as in eval mode."""
        from .dgcnn_train import EDGE_TRAIN_MODES, edgeconv_train
        if self.edge_train not in EDGE_TRAIN_MODES:
            raise ValueError("edge_train must be None, 'fused' or 'torch', got %r" % (self.edge_train,))
        if not x.is_cuda:
            raise RuntimeError("DGCNN.forward needs a device tensor: the graph search and the EdgeConv layers have no CPU path")
        h = x.transpose(1, 2).contiguous()                           # [B,N,C] point-major
        if self.edge_train == "fused":
            h = h.float()
        feats = []
        for l in range(1, 5):
            hd = h.detach().float()
            idx = ops.knn_points(hd, hd, K=self.k).idx
            if self.graph_hook is not None:
                other = self.graph_hook(l - 1, idx)
                if other is not None:
                    idx = other
            conv = getattr(self, "conv%d" % l)
            y = edgeconv_train(h, conv[0], conv[1], idx, self.edge_train)
            feats.append(y)                                         # [B,C',N]
            h = y.transpose(1, 2).contiguous()
        z = self.conv5(torch.cat(feats, 1))
        z = torch.cat((z.max(2)[0], z.mean(2)), 1)
        z = self.dp1(F.leaky_relu(self.bn6(self.linear1(z)), 0.2))
        z = self.dp2(F.leaky_relu(self.bn7(self.linear2(z)), 0.2))
        return self.linear3(z)
