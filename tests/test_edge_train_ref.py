"""CPU: the float64 restatements of tests/_edge_train_ref.py pinned to torch autograd of the materialised composition
(gather -> batch_norm(training) -> leaky_relu -> value at the selected slot), the selection pinned to the true extremum, and
the sensitivity of the bounds of tests/test_gpu_edge_train.py: in every case of that file each defect variant (minimum
branch lost, dgamma term lost, the list's sum of V0 lost) moves an entry past the case's bound, and no pre-activation
lies within the forward bound of the LeakyReLU's kink."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _edge_train_ref as R          # noqa: E402
from _pointnet_bwd_ref import worst_ratio   # noqa: E402


def _args(c):
    return c["U0"], c["V0"], c["idx"], c["gamma"], c["beta"], c["eps"]


@pytest.mark.parametrize("B,N,C,K", R.CASES)
def test_restatements_equal_torch_autograd(B, N, C, K):
    c = R.make_case(B, N, C, K)
    f = R.edge_train_forward(*_args(c))
    leaves = [c[k].clone().requires_grad_() for k in ("U0", "V0", "gamma", "beta")]
    U0, V0, ga, be = leaves
    y, full = R.materialised(U0, V0, c["idx"], ga, be, c["eps"], f["arg"])
    # the gathered value IS the maximum over the neighbours, and the restatement's y is that value
    assert torch.equal(y, full.max(-1).values)
    assert torch.allclose(y, f["y"], rtol=0, atol=1e-11)
    # ties go to the lower slot: the repeated row never selects a later copy of the repeated entry
    a = f["arg"][:, R.REPEAT_ROW]
    assert bool((a <= 1).all())
    assert bool((f["arg"][:, :, R.ZERO_GAMMA] == 0).all())
    # batch statistics as nn.BatchNorm2d tracks them
    z = (R.gather_rows(c["U0"], c["idx"]) + c["V0"].unsqueeze(2)).permute(0, 3, 1, 2)
    bn = torch.nn.BatchNorm2d(C, eps=c["eps"], momentum=1.0).double().train()
    bn(z)
    M = B * N * K
    assert torch.allclose(bn.running_mean, f["mean"], rtol=0, atol=1e-12)
    assert torch.allclose(bn.running_var, f["var"] * M / (M - 1), rtol=1e-12, atol=0)
    # backward at the restatement's slots
    (y * c["g"]).sum().backward()
    r = R.edge_train_backward(*_args(c), c["g"], f["arg"])
    for name, got in (("dU0", U0.grad), ("dV0", V0.grad), ("dgamma", ga.grad), ("dbeta", be.grad)):
        assert torch.allclose(got, r[name][0], rtol=0, atol=1e-10), name
    # the structure every case must hold
    deg = r["indeg"]
    assert bool((deg[:, R.lonely(N)] == 0).all()) and bool((deg[:, R.HUB] >= N).all())
    assert bool((r["dU0"][0][:, R.lonely(N)] == 0).all()) and bool((r["dU0"][1][:, R.lonely(N)] == 0).all())
    assert int((c["gamma"] < 0).sum()) > 0 and int((c["gamma"] == 0).sum()) == 1 and int((c["gamma"] > 0).sum()) > 0
    off = (f["mean"].abs() / torch.sqrt(f["var"]))
    assert float(off[R.OFFSET_CH]) > 31.0 and float(off.sort().values[-2]) < 1.0


@pytest.mark.parametrize("B,N,C,K", R.CASES)
def test_no_preactivation_at_the_kink(B, N, C, K):
    c = R.make_case(B, N, C, K)
    f = R.edge_train_forward(*_args(c))
    assert bool((f["a"].abs() > f["tol_a"]).all()), "case has a pre-activation within the forward bound of the LeakyReLU's kink"


@pytest.mark.parametrize("B,N,C,K", R.CASES)
def test_every_defect_exceeds_the_bound_of_every_case(B, N, C, K):
    c = R.make_case(B, N, C, K)
    f = R.edge_train_forward(*_args(c))
    ok = R.edge_train_backward(*_args(c), c["g"], f["arg"])
    bad = R.edge_train_forward(*_args(c), skip_min=True)
    assert not torch.equal(bad["arg"], f["arg"])
    assert worst_ratio(bad["y"], f["y"], f["tol_y"]) > 1.0
    worst = {}
    for defect, names in (("omit_dgamma_term", ("dV0", "dU0")), ("omit_list_v", ("dU0",))):
        got = R.edge_train_backward(*_args(c), c["g"], f["arg"], **{defect: True})
        for n in names:
            worst[defect, n] = worst_ratio(got[n][0], ok[n][0], ok[n][1])
            assert worst[defect, n] > 1.0, worst
    # the bounds themselves: no wider than a relative 1e-5 of the largest magnitude of their tensor (dU0, whose hub sums
    # thousands of float32 terms one after the other: 1e-4)
    for n, rel in (("dbeta", 1e-5), ("dgamma", 1e-5), ("dV0", 1e-5), ("dU0", 1e-4)):
        assert float(ok[n][1].max()) < rel * float(ok[n][0].abs().max()), n
    assert float(f["tol_y"].max()) < 1e-5 * float(f["y"].abs().max())
