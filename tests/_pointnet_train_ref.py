"""A float64 plain-torch restatement of the PointNet classifier in TRAINING mode (two T-Nets, five convolutions, three
fully connected layers, BatchNorm with batch statistics everywhere, dropout off), evaluated from a state_dict in the
reference layout.  No project code, no reference program text.  tests/test_gpu_pointnet_train.py holds the module to it.

Bound of the module test.  Between the cloud and a parameter's gradient lie L = 40 layer applications (20 forward, 20
backward), each a sum of at most K = 1024 float32 products: a relative rounding of sqrt(K) u per layer (u = 2^-24, the
statistical growth `tolerance` of _pointnet_bwd_ref.py uses), first order, gives L sqrt(K) u; every BatchNorm divides a
centred value by sigma, which amplifies the relative error of its input by |y| / |y - mu|, allowed for by kappa = 8, and
the factor 2 covers |ref| being compared against the tensor's largest entry rather than entry by entry:
    |got - ref| <= MODULE_REL max|ref|,  MODULE_REL = 2 L sqrt(K) kappa u = 2 * 40 * 32 * 8 * 2^-24 = 1.2e-3
for logits and transform, and for a parameter's gradient with max|ref| taken over its GROUP -- a convolution or linear
layer together with the BatchNorm behind it (`group_of`).  The group, not the tensor: a bias in front of a BatchNorm, and
a BatchNorm bias whose channel is live in every instance in front of another BatchNorm, have gradients that are zero in
exact arithmetic -- sums over the batch of the same per-position terms that make up the group's weight gradients (times
activations of order one), cancelling.  The float64 value is ~1e-17, the float32 one a rounding of those terms, so the
group's largest entry is the scale that error has.  That holds only while no max-pool selection flips, so the
test asserts on the float64 side that in each of the three wide layers the selected activation leads the runner-up by
more than the layer's own forward bound (_wide_train_ref.tol_out, which the kernel alone reaches 0.05 of:
tests/test_gpu_wide_train.py).  With 3 x 4 x 1024 selections the smallest lead of a random input is rarely that large:
CASE_SEED was found by evaluating this file's float64 forward for seeds 1 .. 59 on the CPU (no kernel involved)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import _wide_train_ref as R
from _pointnet_bwd_ref import U24

MODULE_REL = 2 * 40 * 32 * 8 * U24
GAP_FACTOR = 1.0
CASE_SEED = 52


def make_state_dict(classes, seed):
    """float32 values in the reference layout: Xavier-uniform weights, small biases, BatchNorm weights in +-[0.5, 1.5]
    (a sixth negative), running statistics at their initial values."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def layer(name, shape):
        fan = (shape[0] + shape[1]) * (shape[2] if len(shape) > 2 else 1)
        sd[name + ".weight"] = (torch.rand(shape, generator=g) * 2 - 1) * (6.0 / fan) ** 0.5
        sd[name + ".bias"] = torch.randn(shape[0], generator=g) * 0.05

    def bn(name, c):
        w = torch.rand(c, generator=g) + 0.5
        w[::6] *= -1
        sd[name + ".weight"], sd[name + ".bias"] = w, torch.randn(c, generator=g) * 0.1
        sd[name + ".running_mean"], sd[name + ".running_var"] = torch.zeros(c), torch.ones(c)
        sd[name + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.long)

    for prefix, K in (("input_transform.", 3), ("feature_transform.", 64)):
        for n, s in (("conv1", (64, K, 1)), ("conv2", (128, 64, 1)), ("conv3", (1024, 128, 1)), ("fc1", (512, 1024)), ("fc2", (256, 512))):
            layer(prefix + n, s)
        sd[prefix + "fc3.weight"] = torch.randn(K * K, 256, generator=g) * (0.02 / K)
        sd[prefix + "fc3.bias"] = torch.eye(K).view(-1).clone()
        for i, c in enumerate([64, 128, 1024, 512, 256], 1):
            bn(prefix + "bn%d" % i, c)
    for n, s in (("conv1", (64, 3, 1)), ("conv2", (64, 64, 1)), ("conv3", (64, 64, 1)), ("conv4", (128, 64, 1)), ("conv5", (1024, 128, 3)),
                 ("fc1", (512, 1024)), ("fc2", (256, 512)), ("fc3", (classes, 256))):
        layer(n, s)
    for i, c in enumerate([64, 64, 64, 128, 1024, 512, 256], 1):
        bn("bn%d" % i, c)
    return sd


_TRUNK = {"conv1": "bn1", "conv2": "bn2", "conv3": "bn3", "conv4": "bn4", "conv5": "bn5", "fc1": "bn6", "fc2": "bn7", "fc3": "fc3"}
_TNET = {"conv1": "bn1", "conv2": "bn2", "conv3": "bn3", "fc1": "bn4", "fc2": "bn5", "fc3": "fc3"}


def group_of(name):
    """'feature_transform.fc1.bias' -> 'feature_transform.bn4': the BatchNorm a layer feeds names the group (fc3: itself)"""
    *prefix, layer, _ = name.split(".")
    table = _TNET if prefix else _TRUNK
    return ".".join(prefix + [table.get(layer, layer)])


def make_cloud(B, N, seed):
    g = torch.Generator().manual_seed(100 + seed)
    pc = torch.randn(B, 3, N, generator=g)
    return (pc / pc.norm(dim=1).max()).float()


def forward(p, pc, wide_inputs=None):
    """p: name -> float64 tensor (parameters may require grad); pc [B,3,N] -> (logits, transform [B,64,64]).
    wide_inputs: a list that receives (prefix, input of the 1024-wide layer) three times."""
    def cbr(x, pre, conv, bnn, eps, relu=True):
        w = p[pre + conv + ".weight"]
        y = F.conv1d(x, w, p[pre + conv + ".bias"], padding=w.shape[2] // 2) if w.dim() == 3 else F.linear(x, w, p[pre + conv + ".bias"])
        y = F.batch_norm(y, None, None, p[pre + bnn + ".weight"], p[pre + bnn + ".bias"], True, 0.1, eps)
        return y.relu() if relu else y

    def tnet(x, pre, K):
        f = cbr(cbr(x, pre, "conv1", "bn1", 1e-3), pre, "conv2", "bn2", 1e-3)
        if wide_inputs is not None:
            wide_inputs.append((pre + "conv3", pre + "bn3", f))
        f = cbr(f, pre, "conv3", "bn3", 1e-3).max(-1)[0]
        f = cbr(cbr(f, pre, "fc1", "bn4", 1e-3), pre, "fc2", "bn5", 1e-3)
        return F.linear(f, p[pre + "fc3.weight"], p[pre + "fc3.bias"]).view(-1, K, K)

    t3 = tnet(pc, "input_transform.", 3)
    f = torch.bmm(pc.permute(0, 2, 1), t3).permute(0, 2, 1)
    f = cbr(cbr(f, "", "conv1", "bn1", 1e-3), "", "conv2", "bn2", 1e-3)
    t64 = tnet(f, "feature_transform.", 64)
    f = torch.bmm(f.permute(0, 2, 1), t64).permute(0, 2, 1)
    f = cbr(cbr(f, "", "conv3", "bn3", 1e-3), "", "conv4", "bn4", 1e-3)
    if wide_inputs is not None:
        wide_inputs.append(("conv5", "bn5", f))
    f = cbr(f, "", "conv5", "bn5", 1e-3).max(-1)[0]
    f = cbr(cbr(f, "", "fc1", "bn6", 1e-5), "", "fc2", "bn7", 1e-5)
    return F.linear(f, p["fc3.weight"], p["fc3.bias"]), t64


def selection_margins(p, wide_inputs):
    """per wide layer: min over the live (b, c) of (lead of the selected activation over the runner-up) / (GAP_FACTOR *
    the layer's forward bound); > 1 means no selection can flip.  Live: gamma != 0 and the selected activation positive
    (a relu-dead channel passes no gradient whichever point is taken)."""
    out = {}
    for conv, bnn, x in wide_inputs:
        w = p[conv + ".weight"].detach()
        taps = w.shape[2]
        W = w.permute(0, 2, 1).reshape(1024, -1)
        ga, be = p[bnn + ".weight"].detach(), p[bnn + ".bias"].detach()
        f = R.wide_train_forward(x.detach(), W, p[conv + ".bias"].detach(), ga, be, 1e-3, True, taps)
        z = (ga / f["sigma"]).view(1, -1, 1) * (f["y0"] - (f["mean"] - p[conv + ".bias"].detach()).view(1, -1, 1)) + be.view(1, -1, 1)
        top2 = z.topk(2, dim=-1).values
        lead = top2[..., 0] - top2[..., 1]
        live = (top2[..., 0] > 0) & (ga != 0).view(1, -1)
        out[conv] = float((lead / (GAP_FACTOR * f["tol_out"]))[live].min())
    return out
