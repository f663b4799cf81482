"""CPU: the float64 restatements of tests/_wide_train_ref.py pinned to torch autograd of conv1d -> batch_norm(training) ->
[relu] -> max, and the sensitivity of the bounds of tests/test_gpu_wide_train.py: for every case of that file at least one
defect variant (minimum branch lost, k2 term lost, relu gate lost, tap fold shifted) moves an entry past the case's bound."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(__file__))
import _wide_train_ref as R          # noqa: E402
from _pointnet_bwd_ref import worst_ratio   # noqa: E402


def autograd(c):
    T = c["taps"]
    leaves = [c[k].clone().requires_grad_() for k in ("X", "W", "bias", "gamma", "beta")]
    X, W, b, ga, be = leaves
    y = F.conv1d(X, W.view(1024, T, 128).permute(0, 2, 1), b, padding=T // 2)
    z = F.batch_norm(y, None, None, ga, be, True, 0.1, c["eps"])
    out = (z.relu() if c["relu"] else z)
    return leaves, out


@pytest.mark.parametrize("B,N,taps,relu", [(3, 33, 3, True), (1, 64, 1, True), (2, 200, 3, False), (3, 33, 1, False)])
def test_restatements_equal_torch_autograd(B, N, taps, relu):
    c = R.make_case(B, N, taps, relu)
    f = R.wide_train_forward(c["X"], c["W"], c["bias"], c["gamma"], c["beta"], c["eps"], relu, taps)
    leaves, full = autograd(c)
    assert torch.allclose(full.max(-1).values, f["out"], rtol=0, atol=1e-11)
    # the restatement's own selection (first extremum of y by gamma's sign) holds the maximum of the activation
    sel = torch.gather(full, 2, f["arg"].unsqueeze(-1)).squeeze(-1)
    assert torch.equal(sel, full.max(-1).values)
    # batch statistics as nn.BatchNorm1d tracks them
    bn = torch.nn.BatchNorm1d(1024, eps=c["eps"], momentum=1.0).double().train()
    bn(f["y0"] + c["bias"].view(1, -1, 1))
    M = B * N
    assert torch.allclose(bn.running_mean, f["mean"], rtol=0, atol=1e-12)
    assert torch.allclose(bn.running_var, f["var"] * M / (M - 1), rtol=1e-12, atol=0)
    # backward at the restatement's indices
    (sel * c["g"]).sum().backward()
    r = R.wide_train_backward(c["X"], c["W"], c["bias"], c["gamma"], c["beta"], c["eps"], relu, taps, c["g"], f["arg"])
    X, W, b, ga, be = leaves
    for name, got in (("dX", X.grad), ("dW", W.grad), ("dgamma", ga.grad), ("dbeta", be.grad)):
        assert torch.allclose(got, r[name][0], rtol=0, atol=1e-10), name
    assert float(b.grad.abs().max()) < 1e-12 and bool((r["dbias"][0] == 0).all())


@pytest.mark.parametrize("B,N,taps,relu", R.CASES)
def test_a_defect_exceeds_the_bound_of_every_case(B, N, taps, relu):
    c = R.make_case(B, N, taps, relu)
    args = (c["X"], c["W"], c["bias"], c["gamma"], c["beta"], c["eps"], relu, taps)
    f = R.wide_train_forward(*args)
    ok = R.wide_train_backward(*args, c["g"], f["arg"])
    assert worst_ratio(R.wide_train_forward(*args, skip_min=True)["out"], f["out"], f["tol_out"]) > 1.0
    worst = {}
    for defect, names in (("omit_k2", ("dW", "dX")), ("shift_fold", ("dX",)), ("skip_relu_gate", ("dbeta", "dgamma", "dW", "dX"))):
        if defect == "shift_fold" and taps == 1:
            continue
        if defect == "skip_relu_gate" and not relu:
            continue
        bad = R.wide_train_backward(*args, c["g"], f["arg"], **{defect: True})
        worst[defect] = max(worst_ratio(bad[n][0], ok[n][0], ok[n][1]) for n in names)
        assert worst[defect] > 1.0, (defect, worst)
    assert "omit_k2" in worst
