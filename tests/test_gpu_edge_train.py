"""The fused train-mode EdgeConv layer (geoa3_amd/dgcnn_train.py EdgeTrainFn on csrc/edgeconv_train.hip) alone against the
float64 restatements of tests/_edge_train_ref.py, with that file's bounds (derived in its docstring from the float32
roundings behind each entry; tests/test_edge_train_ref.py shows that they notice a lost term).

Cases (_edge_train_ref.CASES, (B,N,C,K)): (2,33,64,4), (3,40,70,5), (1,64,128,20), (2,200,256,20) -- a ragged point tile, a
ragged channel tile, a second channel tile, the workload's K; each with channels of negative gamma, one zero gamma, one
channel offset by 32 standard deviations, a row of idx with repeated entries, a point nobody lists and a hub every point
lists.  The selection compares the float32 inputs themselves, so `arg` must equal the reference's exactly."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _edge_train_ref as R          # noqa: E402
from _pointnet_bwd_ref import tolerance, worst_ratio   # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(B, N, C, K):
    c = R.make_case(B, N, C, K)
    c["fwd"] = R.edge_train_forward(c["U0"], c["V0"], c["idx"], c["gamma"], c["beta"], c["eps"])
    c["bwd"] = R.edge_train_backward(c["U0"], c["V0"], c["idx"], c["gamma"], c["beta"], c["eps"], c["g"], c["fwd"]["arg"])
    return c


def run(c, U0=None, idx=None, need_grad=True):
    from geoa3_amd.dgcnn_train import EdgeTrainFn
    dev = lambda t: t.float().cuda().requires_grad_(need_grad)
    u, v, ga, be = dev(c["U0"] if U0 is None else U0), dev(c["V0"]), dev(c["gamma"]), dev(c["beta"])
    y, mean, var, arg = EdgeTrainFn.apply(u, v, (c["idx"] if idx is None else idx).cuda(), ga, be, c["eps"])
    return (u, v, ga, be), y, mean, var, arg


@pytest.mark.parametrize("B,N,C,K", R.CASES)
def test_layer_against_float64(B, N, C, K):
    c = case(B, N, C, K)
    f, ref = c["fwd"], c["bwd"]
    leaves, y, mean, var, arg = run(c)
    assert torch.equal(arg.cpu().long(), f["arg"]), "the selection is exact: float32 inputs compared with themselves"
    ratios = {"y": worst_ratio(y.detach().cpu(), f["y"], f["tol_y"]),
              "mean": worst_ratio(mean.cpu(), f["mean"], f["tol_mean"]),
              "var": worst_ratio(var.cpu(), f["var"], f["tol_var"])}
    assert bool((f["a"].abs() > f["tol_a"]).all()), "case has a pre-activation within the forward bound of the kink"
    (y * c["g"].float().cuda()).sum().backward()
    u, v, ga, be = leaves
    for name, got in (("dbeta", be.grad), ("dgamma", ga.grad), ("dV0", v.grad), ("dU0", u.grad)):
        ratios[name] = worst_ratio(got.cpu(), *ref[name])
    print("(%d,%d,%d,%d) err/tol " % (B, N, C, K) + "  ".join("%s %.3f" % kv for kv in ratios.items()))
    for name, r in ratios.items():
        assert r <= 1.0, (name, r)
    assert bool((u.grad[:, R.lonely(N)] == 0).all())          # nobody lists it: every term of its dU0 is zero


def test_saved_neighbour_sums():
    """S1 of the raw entry point: the sequential float32 sum over the K slots"""
    from geoa3_amd import ops
    c = case(3, 40, 70, 5)
    d = lambda t: t.float().cuda()
    _, _, S1, _, _, stats = ops.edge_train(d(c["U0"]), d(c["V0"]), c["idx"].cuda(), d(c["gamma"]), d(c["beta"]), c["eps"])
    assert worst_ratio(S1.cpu(), c["fwd"]["S1"], c["fwd"]["tol_S1"]) <= 1.0
    assert stats.dtype == torch.float64 and tuple(stats.shape) == (3, 70)
    assert torch.allclose(stats[0].cpu(), c["fwd"]["mean"], rtol=0, atol=float(c["fwd"]["tol_mean"].max()))


@pytest.mark.parametrize("B,N,C,K", [R.CASES[0], R.CASES[3]])
def test_running_statistics_equal_batchnorm(B, N, C, K):
    """bn's buffers after edgeconv_train == nn.BatchNorm2d's own update from the float64 edge values (its momentum, the
    unbiased variance, num_batches_tracked).  h holds small integers and the weight multiples of 1/8, so U0 and V0 are exact
    in float32 whatever the order of the matmul's sums: both sides see the same edge values."""
    import torch.nn as nn
    from geoa3_amd.dgcnn_train import edgeconv_train
    c = case(B, N, C, K)
    Cin, mom = 6, 0.3
    gen = torch.Generator().manual_seed(B * N + C)
    h = torch.randint(-4, 5, (B, N, Cin), generator=gen).double()
    W = torch.randint(-8, 9, (C, 2 * Cin), generator=gen).double() / 8
    conv = nn.Conv2d(2 * Cin, C, 1, bias=False)
    bn = nn.BatchNorm2d(C, eps=c["eps"], momentum=mom)
    with torch.no_grad():
        conv.weight.copy_(W.view(C, 2 * Cin, 1, 1))
        bn.weight.copy_(c["gamma"])
        bn.bias.copy_(c["beta"])
        bn.running_mean.normal_(generator=gen)
        bn.running_var.uniform_(0.5, 2.0, generator=gen)
    old_mean, old_var = bn.running_mean.double().clone(), bn.running_var.double().clone()
    ref_bn = nn.BatchNorm2d(C, eps=c["eps"], momentum=mom).double()
    ref_bn.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in bn.state_dict().items()})
    U0, V0 = h @ W[:, :Cin].t(), h @ (W[:, Cin:] - W[:, :Cin]).t()
    z = (R.gather_rows(U0, c["idx"]) + V0.unsqueeze(2)).permute(0, 3, 1, 2)
    ref_bn.train()(z)
    f = R.edge_train_forward(U0, V0, c["idx"], c["gamma"], c["beta"], c["eps"])
    conv, bn = conv.cuda(), bn.cuda().train()
    y = edgeconv_train(h.float().cuda(), conv, bn, c["idx"].cuda(), mode="fused")
    assert worst_ratio(y.detach().cpu(), f["y"], f["tol_y"]) <= 1.0
    M = B * N * K
    assert int(bn.num_batches_tracked) == int(ref_bn.num_batches_tracked) == 1
    # new = (1 - m) old + m stat in float32: three roundings on top of the statistic's own bound
    tol_m = tolerance(ref_bn.running_mean, (1 - mom) * old_mean.abs() + mom * f["mean"].abs(), 3) + mom * f["tol_mean"]
    tol_v = tolerance(ref_bn.running_var, (1 - mom) * old_var + mom * f["var"] * M / (M - 1), 3) + mom * M / (M - 1) * f["tol_var"]
    r_m = worst_ratio(bn.running_mean.cpu(), ref_bn.running_mean, tol_m)
    r_v = worst_ratio(bn.running_var.cpu(), ref_bn.running_var, tol_v)
    print("running mean err/tol %.3f var err/tol %.3f" % (r_m, r_v))
    assert r_m <= 1.0 and r_v <= 1.0


def test_two_runs_give_identical_bits():
    c = case(2, 200, 256, 20)
    res = []
    for _ in range(2):
        leaves, y, mean, var, arg = run(c)
        (y * c["g"].float().cuda()).sum().backward()
        res.append([y.detach(), mean, var, arg] + [t.grad for t in leaves])
    for p, q in zip(*res):
        assert torch.equal(p, q)


def test_one_nan_poisons_its_channel_only():
    c = case(3, 40, 70, 5)
    _, y0, mean0, var0, _ = run(c, need_grad=False)
    U0 = c["U0"].clone()
    U0[1, R.HUB, 66] = float("nan")
    _, y, mean, var, _ = run(c, U0=U0, need_grad=False)
    other = torch.arange(70) != 66
    assert bool(torch.isnan(y[:, 66]).all()) and bool(torch.isnan(mean[66])) and bool(torch.isnan(var[66]))
    assert torch.equal(y[:, other], y0[:, other]) and torch.equal(mean[other], mean0[other]) and torch.equal(var[other], var0[other])
    assert bool(torch.isfinite(y0).all())


@pytest.mark.parametrize("bad", [-1, 40, 2 ** 40])
def test_one_index_out_of_range_poisons_the_layer(bad):
    c = case(3, 40, 70, 5)
    idx = c["idx"].clone()
    idx[2, 17, 3] = bad
    leaves, y, mean, var, arg = run(c, idx=idx)
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(mean).all()) and bool(torch.isnan(var).all())
    (y * c["g"].float().cuda()).sum().backward()          # the backward skips the entry: nothing is dereferenced
    torch.cuda.synchronize()
    assert all(t.grad is not None and tuple(t.grad.shape) == tuple(t.shape) for t in leaves)


def test_single_value_per_channel_is_refused():
    from geoa3_amd import _lib, ops
    from geoa3_amd.dgcnn_train import EdgeTrainFn
    z = lambda *s: torch.zeros(*s, device="cuda")
    i = torch.zeros(1, 1, 1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        EdgeTrainFn.apply(z(1, 1, 64), z(1, 1, 64), i, z(64), z(64), 1e-5)
    assert _lib.load().geoa3_edge_train_workspace_bytes(1, 1, 64, 1) == -1      # GEOA3_EINVAL
    with pytest.raises(_lib.Geoa3Error, match="invalid argument"):
        ops.edge_train(z(1, 1, 64), z(1, 1, 64), i, z(64), z(64), 1e-5)
    assert _lib.load().geoa3_edge_train_workspace_bytes(1, 1, 64, 2) > 0
