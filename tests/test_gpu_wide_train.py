"""The fused train-mode wide layer (geoa3_amd/pointnet_train.py WideTrainFn on csrc/pointnet_wide_train.hip) alone against
the float64 restatements of tests/_wide_train_ref.py, with that file's bounds (fp32 matrix core: `tolerance` with c = 4,
extra = 0, carried through sigma; derivation in its docstring and in DESIGN.md, "Training").

Cases (_wide_train_ref.CASES): (B, N) in {(1, 64), (3, 33), (2, 200)} x taps {1, 3} x relu on / off; each with negative
gamma, one zero gamma, relu-dead channels, exact duplicate points, one input channel offset by 32 standard deviations.
The backward reference is evaluated at the kernel's own indices, so no entry is left out for a near-tie."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _wide_train_ref as R          # noqa: E402
from _pointnet_bwd_ref import worst_ratio   # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(B, N, taps, relu):
    c = R.make_case(B, N, taps, relu)
    c["fwd"] = R.wide_train_forward(c["X"], c["W"], c["bias"], c["gamma"], c["beta"], c["eps"], relu, taps)
    return c


def run(c, X=None, need_grad=True):
    from geoa3_amd.pointnet_train import WideTrainFn
    dev = lambda t: t.float().cuda().requires_grad_(need_grad)
    x, w, b, ga, be = (dev(X if X is not None else c["X"]), dev(c["W"]), dev(c["bias"]), dev(c["gamma"]), dev(c["beta"]))
    out, mean, var, arg = WideTrainFn.apply(x, w, b, ga, be, c["eps"], c["relu"], c["taps"])
    return (x, w, b, ga, be), out, mean, var, arg


@pytest.mark.parametrize("B,N,taps,relu", R.CASES)
def test_layer_against_float64(B, N, taps, relu):
    c = case(B, N, taps, relu)
    f = c["fwd"]
    leaves, out, mean, var, arg = run(c)
    a = arg.cpu().long()
    # forward values
    r = worst_ratio(out.detach().cpu(), f["out"], f["tol_out"])
    print("out err/tol %.3f" % r)
    assert r <= 1.0
    r_m = worst_ratio(mean.cpu(), f["mean"], f["tol_mu"] + 2.0 ** -23 * f["mean"].abs())
    r_v = worst_ratio(var.cpu(), f["var"], f["tol_var"] + 2.0 ** -23 * f["var"])
    print("mean err/tol %.3f var err/tol %.3f" % (r_m, r_v))
    assert r_m <= 1.0 and r_v <= 1.0
    # indices: within the bound of the float64 extremum; exact duplicates go to the lower index
    y = f["y0"]
    ysel = torch.gather(y, 2, a.unsqueeze(-1)).squeeze(-1)
    pos, neg, zero = c["gamma"] > 0, c["gamma"] < 0, c["gamma"] == 0
    bound = 2 * f["tol_y"]
    assert bool((ysel >= y.max(-1).values - bound)[:, pos].all())
    assert bool((ysel <= y.min(-1).values + bound)[:, neg].all())
    assert bool((a[:, zero] == 0).all())
    # points 20..24 repeat 10..14: every column of the run coincides for one tap, the inner three for three taps
    dup = (a >= 20) & (a < 25) if taps == 1 else (a >= 21) & (a < 24)
    assert not bool(dup[:, ~zero].any()), "a duplicate point won over its lower original"
    assert int(pos.sum()) > 0 and int(neg.sum()) > 0 and int(zero.sum()) == 1
    # backward at the kernel's indices
    g = c["g"].float().cuda()
    (out * g).sum().backward()
    ref = R.wide_train_backward(c["X"], c["W"], c["bias"], c["gamma"], c["beta"], c["eps"], relu, taps, c["g"], a)
    if relu:   # the kernel gates by its own float32 output: the float64 pre-activation must be clear of zero
        z, tz = ref["gate_margin"]
        assert bool((z.abs() > tz).all()), "case has a pre-activation within the forward bound of the relu's kink"
    x, w, b, ga, be = leaves
    for name, got in (("dbeta", be.grad), ("dgamma", ga.grad), ("dW", w.grad), ("dX", x.grad)):
        val, tol = ref[name]
        r = worst_ratio(got.cpu(), val, tol)
        print("%s err/tol %.3f" % (name, r))
        assert r <= 1.0, name
    assert b.grad is not None and bool((b.grad == 0).all())
    if relu:
        assert bool((out.detach()[:, R.DEAD] == 0).all()) and bool((w.grad[R.DEAD] == 0).all())


@pytest.mark.parametrize("B,N,taps,relu", [(3, 33, 3, True), (2, 200, 1, False)])
def test_running_statistics_equal_batchnorm(B, N, taps, relu):
    """bn's buffers after the fused layer == nn.BatchNorm1d's own update from the float64 conv output (its momentum,
    the unbiased variance, num_batches_tracked), to the forward's bounds."""
    import torch.nn as nn
    from geoa3_amd.pointnet_train import wide_layer_train
    c = case(B, N, taps, relu)
    conv = nn.Conv1d(128, 1024, taps, 1, taps // 2)
    bn = nn.BatchNorm1d(1024, eps=c["eps"], momentum=0.3)
    with torch.no_grad():
        conv.weight.copy_(c["W"].view(1024, taps, 128).permute(0, 2, 1))
        conv.bias.copy_(c["bias"])
        bn.weight.copy_(c["gamma"])
        bn.bias.copy_(c["beta"])
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
    ref_bn = nn.BatchNorm1d(1024, eps=c["eps"], momentum=0.3).double()
    ref_bn.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in bn.state_dict().items()})
    ref_bn.train()(c["fwd"]["y0"] + c["bias"].view(1, -1, 1))
    conv, bn = conv.cuda(), bn.cuda().train()
    wide_layer_train(c["X"].float().cuda(), conv, bn, relu=relu, mode="fused")
    f = c["fwd"]
    M = B * N
    assert int(bn.num_batches_tracked) == int(ref_bn.num_batches_tracked) == 1
    assert worst_ratio(bn.running_mean.cpu(), ref_bn.running_mean, 0.3 * f["tol_mu"] + 2.0 ** -22 * ref_bn.running_mean.abs()) <= 1.0
    assert worst_ratio(bn.running_var.cpu(), ref_bn.running_var, 0.3 * M / (M - 1) * f["tol_var"] + 2.0 ** -22 * ref_bn.running_var) <= 1.0


def test_two_runs_give_identical_bits():
    c = case(2, 200, 3, True)
    res = []
    for _ in range(2):
        leaves, out, mean, var, arg = run(c)
        (out * c["g"].float().cuda()).sum().backward()
        res.append([out.detach(), mean, var, arg] + [t.grad for t in leaves])
    for p, q in zip(*res):
        assert torch.equal(p, q)


@pytest.mark.parametrize("taps", [1, 3])
def test_one_nan_poisons_every_channel(taps):
    c = case(2, 200, taps, True)
    X = c["X"].clone()
    X[1, 17, 130] = float("nan")
    _, out, mean, var, _ = run(c, X=X, need_grad=False)
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(mean).all()) and bool(torch.isnan(var).all())


def test_single_value_per_channel_is_refused():
    from geoa3_amd.pointnet_train import WideTrainFn
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        WideTrainFn.apply(z(1, 128, 1), z(1024, 128), z(1024), z(1024), z(1024), 1e-3, True, 1)
