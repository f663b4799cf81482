"""geoa3_amd.dgcnn.DGCNN in TRAINING mode (net.edge_train) at B 3, N 48, k 4, emb_dims 64, dropout 0: logits and every
parameter gradient of edge_train = "fused" and "torch" against a float64 run of the torch composition on the device, fed
the fused run's four neighbour tables through graph_hook -- so the comparison sees float32 rounding, never another graph.

The bar: the error of a run may be at most 4 times the float32 torch composition's own error against that float64 run (on
the same tables), plus a floor of 2^-20 of the tensor's largest magnitude.  Both are float32 with different summation orders,
which is what the factor allows for.  The measured ratios are printed (DESIGN.md 8e records them).  For mode "torch" the
run IS the float32 torch composition on those tables, so its error equals its own and the ratio is at most 0.25 by
construction: that case checks that the mode runs, honours graph_hook and gives finite values, nothing more."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, K, EMB, CLASSES = 3, 48, 4, 64, 40


def make_net(seed=21):
    from geoa3_amd.dgcnn import DGCNN
    torch.manual_seed(seed)
    net = DGCNN(k=K, emb_dims=EMB, dropout=0.0, output_channels=CLASSES)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.copy_((torch.rand(m.weight.shape, generator=g) + 0.5) * (1 - 2 * (torch.rand(m.weight.shape, generator=g) < 0.25).float()))
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return net


def _cloud(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, N, generator=g)
    return (x / x.norm(dim=1, keepdim=True).amax(2, keepdim=True)).float()


def _step(net, x, w):
    net.zero_grad(set_to_none=True)
    logits = net(x)
    (logits * w).sum().backward()
    return logits.detach(), {n: p.grad.detach().clone() for n, p in net.named_parameters()}


@functools.lru_cache(maxsize=None)
def runs():
    """the fused run (its tables recorded), then float32 'torch' and float64 'torch' on THOSE tables: computed once, shared"""
    assert torch.cuda.is_available(), "needs the MI355X"
    base = make_net()
    x = _cloud(50).cuda()
    w = torch.randn(B, CLASSES, generator=torch.Generator().manual_seed(60)).cuda()
    tables = []
    fused = copy.deepcopy(base).cuda().train()
    fused.edge_train = "fused"
    fused.graph_hook = lambda layer, idx: tables.append(idx.clone()) or None
    out = {"fused": _step(fused, x, w)}
    assert len(tables) == 4 and all(tuple(t.shape) == (B, N, K) and t.dtype == torch.int64 for t in tables)
    plain = copy.deepcopy(base).cuda().train()
    plain.edge_train = "torch"
    plain.graph_hook = lambda layer, idx: tables[layer]
    out["torch"] = _step(plain, x, w)
    ref = copy.deepcopy(base).double().cuda().train()
    ref.edge_train = "torch"
    ref.graph_hook = lambda layer, idx: tables[layer]
    out["float64"] = _step(ref, x.double(), w.double())
    out["nets"] = {"fused": fused, "torch": plain, "float64": ref}
    out["x"], out["tables"] = x, tables
    return out


def test_edge_train_none_still_raises():
    net = make_net().train()
    assert net.edge_train is None
    with pytest.raises(NotImplementedError):
        net(_cloud(1))                       # on CPU tensors too
    with pytest.raises(NotImplementedError):
        net.cuda()(_cloud(1).cuda())
    net.edge_train = "neither"
    with pytest.raises(ValueError):
        net(_cloud(1).cuda())


@pytest.mark.parametrize("mode", ["fused", "torch"])
def test_logits_and_parameter_gradients_against_float64(mode):
    r = runs()
    (lg, gr), (lt, gt), (l64, g64) = r[mode], r["torch"], r["float64"]
    assert set(gr) == set(g64) and len(gr) > 20
    worst = ("", 0.0)
    for name in ["logits"] + list(g64):
        got, base, ref = (lg, lt, l64) if name == "logits" else (gr[name], gt[name], g64[name])
        err = float((got.double() - ref).abs().max())
        own = float((base.double() - ref).abs().max())
        bar = 4.0 * own + 2.0 ** -20 * float(ref.abs().max())
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
        print("%s %-22s err %.3e  torch float32 err %.3e  err/bar %.3f" % (mode, name, err, own, ratio))
        worst = max(worst, (name, ratio), key=lambda t: t[1])
        assert torch.isfinite(got).all()
    print("%s: worst err/bar %.3f (%s)" % (mode, worst[1], worst[0]))
    assert worst[1] <= 1.0, worst


def test_running_statistics_move_as_the_torch_layers_do():
    r = runs()
    sf, s64 = r["nets"]["fused"].state_dict(), r["nets"]["float64"].state_dict()
    for k in sf:
        if k.endswith("num_batches_tracked"):
            assert int(sf[k]) == int(s64[k]) == 1
        elif "running_" in k:
            assert torch.allclose(sf[k].double(), s64[k], rtol=1e-5, atol=1e-6), k


def test_state_dict_keys_and_eval_after_training():
    from tests import _dgcnn_ref as R
    from tests.test_dgcnn_api import PUBLIC_STATE_KEYS      # the public model's keys, written out there
    r = runs()
    net = copy.deepcopy(r["nets"]["fused"])
    assert list(net.state_dict().keys()) == PUBLIC_STATE_KEYS
    net.graph_hook = None
    x = r["x"]
    before = net.eval()(x)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    net.train()
    opt.zero_grad()
    net(x).square().mean().backward()
    opt.step()
    # .eval(): the eval kernels on the trained weights and running statistics (refolded), against the float64 model
    tables = []
    net.graph_hook = lambda layer, idx: tables.append(idx.clone()) or None
    after = net.eval()(x)
    assert not torch.equal(before, after) and bool(torch.isfinite(after).all())
    ref, _ = R.dgcnn_f64(net.state_dict(), x.cpu(), [t.cpu() for t in tables])
    assert float((after.cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
