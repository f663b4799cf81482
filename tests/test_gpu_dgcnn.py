"""geoa3_amd.dgcnn.DGCNN on the device against the float64 restatement of the public model (tests/_dgcnn_ref.py), fed the
device's own four neighbour tables through graph_hook -- so what the comparison sees is fp32 rounding, never a different graph."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import _dgcnn_ref as R

pytestmark = pytest.mark.gpu

# (B, N, k, seed): the issue's shape, k = N (every point is everybody's neighbour), and a batch of one
CASES = {"b2_k20": (2, 64, 20, 1), "k_is_n": (2, 64, 64, 2), "b1": (1, 64, 20, 3)}
# Largest relative deviation max|device - float64| / max|float64| over CASES, measured on one MI355X in one run of this
# file at the commit that added it (logits 2.07e-7 / 3.54e-7 / 4.26e-7, input gradient 7.47e-7 / 7.80e-7 / 4.54e-7 for the
# three cases).  Not derived: fp32 rounding through nine layers with the graphs held fixed.  The bars are four times the
# largest measured values (the DGCNN rows).
MEASURED_LOGITS, MEASURED_GRAD = 4.259e-7, 7.795e-7
BAR_LOGITS, BAR_GRAD = 4 * MEASURED_LOGITS, 4 * MEASURED_GRAD


def make_net(seed, k=20, **kw):
    """a DGCNN with seeded default init and non-trivial BatchNorm affine maps and statistics, in eval mode on the CPU"""
    from geoa3_amd.dgcnn import DGCNN
    torch.manual_seed(seed)
    net = DGCNN(k=k, **kw)
    g = torch.Generator().manual_seed(seed + 1000)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
    return net.eval()


def _cloud(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, N, generator=g)
    return (x / x.norm(dim=1, keepdim=True).amax(2, keepdim=True)).float()


@functools.lru_cache(maxsize=None)
def run_case(tag):
    """forward and input gradient on the device with the tables recorded, and the float64 values on THOSE tables: computed
    once, shared, never modified"""
    B, N, k, seed = CASES[tag]
    assert torch.cuda.is_available(), "needs the MI355X"
    net = make_net(seed, k)
    sd = {n: v.clone() for n, v in net.state_dict().items()}
    tables = []
    net.graph_hook = lambda layer, idx: tables.append((layer, idx.clone())) or None
    net = net.cuda()
    x = _cloud(B, N, seed + 50)
    w = torch.randn(B, 40, generator=torch.Generator().manual_seed(seed + 60))
    xd = x.cuda().requires_grad_()
    logits = net(xd)
    (gx,) = torch.autograd.grad((logits * w.cuda()).sum(), xd)
    assert [l for l, _ in tables] == [0, 1, 2, 3]
    idxs = [t.cpu() for _, t in tables]
    x64 = x.double().requires_grad_()
    ref_logits, ref_feats = R.dgcnn_f64(sd, x64, idxs)
    (ref_gx,) = torch.autograd.grad((ref_logits * w.double()).sum(), x64)
    return dict(net=net, sd=sd, x=x, w=w, idxs=idxs, logits=logits.detach().cpu(), gx=gx.cpu(),
                ref_logits=ref_logits.detach(), ref_gx=ref_gx, ref_feats=[f.detach() for f in ref_feats])


@functools.lru_cache(maxsize=None)
def chain(tag):
    """the four EdgeConv layers one by one on the device, on the recorded tables: every layer's input h [B,N,C] (CPU), output
    y [B,C',N] and arg [B,N,C'] -- the module's forward is this chain (test_every_layer_... holds it to that)"""
    from geoa3_amd import ops
    c = run_case(tag)
    w = c["net"].folded(torch.device("cuda", torch.cuda.current_device()))
    h = c["x"].cuda().transpose(1, 2).contiguous()
    out = []
    for l in range(1, 5):
        y, arg = ops.edge_max(torch.matmul(h, w["wa%d" % l]), torch.matmul(h, w["wd%d" % l]), w["t%d" % l],
                              c["idxs"][l - 1].cuda())
        out.append((h.cpu(), y.cpu(), arg.cpu().long()))
        h = y.transpose(1, 2).contiguous()
    return out


@pytest.mark.parametrize("tag", list(CASES))
def test_tables_are_the_searches_of_each_layers_input(tag):
    """every recorded table IS the K-NN of that layer's own input (D = 3, 64, 64, 128), recomputed by the float32 loop of
    tests/_knn_nd_ref.py on the device's activations: a forward that searched another tensor would differ"""
    from tests import _knn_nd_ref as KR
    c = run_case(tag)
    B, N, k, _ = CASES[tag]
    for l, (idx, (h, _, _)) in enumerate(zip(c["idxs"], chain(tag))):
        assert idx.dtype == torch.int64 and tuple(idx.shape) == (B, N, k)
        assert tuple(h.shape) == (B, N, R.EDGE_LAYERS[l][0] // 2)
        assert (idx == torch.arange(N).view(1, N, 1)).any(2).all()      # the point itself is a neighbour
        _, want = KR.knn_nd(h.numpy(), h.numpy(), k)
        assert np.array_equal(idx.numpy(), want), "layer %d" % (l + 1)
    assert not torch.equal(c["idxs"][0], c["idxs"][1]) or k == N        # the graph is dynamic


@pytest.mark.parametrize("tag", list(CASES))
def test_every_layer_within_the_rounding_bound(tag):
    """Each EdgeConv layer alone, on the DEVICE's input of that layer, against the float64 standard formulation: within
    (C + 4) 2^-23 A, C = 3, 64, 64, 128, A the sum of the absolute values of the terms of the element's own pre-activation --
    the edge that reaches the maximum in float64; where the device's arg is another edge, the larger of the two edges'
    bounds (as in tests/test_gpu_edgeconv.py).  The chain of the four is the module's forward."""
    from geoa3_amd.dgcnn import edgeconv
    c = run_case(tag)
    net, sd = c["net"], c["sd"]
    w = net.folded(torch.device("cuda", torch.cuda.current_device()))
    for l, ((cin, cout), (h, y, arg)) in enumerate(zip(R.EDGE_LAYERS, chain(tag)), 1):
        idx = c["idxs"][l - 1]
        assert torch.equal(edgeconv(h.cuda(), w["wa%d" % l], w["wd%d" % l], w["t%d" % l], idx.cuda()).cpu(), y)
        p = "conv%d.1." % l
        ref = R.edgeconv_f64(h.double().transpose(1, 2), idx, sd["conv%d.0.weight" % l].view(cout, cin), sd[p + "weight"],
                             sd[p + "bias"], sd[p + "running_mean"], sd[p + "running_var"])
        bound = (cin // 2 + 4) * 2.0 ** -23 * ref["A"]                    # [B,N,k,C'] per edge
        bound = torch.maximum(torch.gather(bound, 2, ref["arg"].unsqueeze(2)), torch.gather(bound, 2, arg.unsqueeze(2))).squeeze(2)
        err = (y.double().transpose(1, 2) - ref["y"].transpose(1, 2)).abs()
        ratio = float((err / bound).max())
        print("%s layer %d: max error / bound = %.3f" % (tag, l, ratio))
        assert ratio <= 1.0
    # the module's own forward on the same tables (substituted through the hook) runs exactly this chain
    net2 = copy.deepcopy(net)
    net2.graph_hook = lambda layer, _idx: c["idxs"][layer].cuda()
    assert torch.equal(net2(c["x"].cuda()).cpu(), c["logits"])


@pytest.mark.parametrize("tag", list(CASES))
def test_logits_and_input_gradient_against_float64(tag):
    c = run_case(tag)
    dl = float((c["logits"].double() - c["ref_logits"]).abs().max() / c["ref_logits"].abs().max())
    dg = float((c["gx"].double() - c["ref_gx"]).abs().max() / c["ref_gx"].abs().max())
    print("%s: relative deviation logits %.3e, input gradient %.3e" % (tag, dl, dg))
    assert dl <= BAR_LOGITS
    assert dg <= BAR_GRAD


def test_state_dict_keys_and_round_trips():
    net = make_net(5)
    from tests.test_dgcnn_api import PUBLIC_STATE_KEYS      # the public model's keys, written out there
    assert list(net.state_dict().keys()) == PUBLIC_STATE_KEYS
    sd = {k: v.clone() for k, v in make_net(6).state_dict().items()}
    net.load_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    other = make_net(7)
    other.load_state_dict({"module." + k: v for k, v in sd.items()})
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())
    x = _cloud(2, 64, 8).cuda()
    assert torch.equal(net.cuda()(x), other.cuda()(x))


def test_loading_new_weights_refolds():
    """the folded weights are cached per weight version: an in-place update of a parameter is seen by the next forward"""
    net = make_net(9).cuda()
    x = _cloud(2, 64, 10).cuda()
    a = net(x)
    with torch.no_grad():
        net.linear3.bias.add_(1.0)
    assert torch.allclose(net(x), a + 1.0, atol=1e-5) and not torch.equal(net(x), a)


def test_two_runs_are_bit_identical():
    net = make_net(11).cuda()
    x = _cloud(2, 64, 12).cuda()
    w = torch.randn(2, 40, generator=torch.Generator().manual_seed(13)).cuda()
    res = []
    for _ in range(2):
        xd = x.clone().requires_grad_()
        logits = net(xd)
        (g,) = torch.autograd.grad((logits * w).sum(), xd)
        res.append((logits.detach(), g))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert bool(res[0][1].abs().sum() > 0)


def test_training_mode_and_cpu_input_raise():
    net = make_net(14).cuda()
    with pytest.raises(NotImplementedError):
        net.train()(_cloud(2, 64, 15).cuda())
    with pytest.raises(RuntimeError):
        net.eval()(_cloud(2, 64, 15))


def test_main_attack_arch_dgcnn_end_to_end(tmp_path, monkeypatch):
    """--arch DGCNN --synthetic without a checkpoint: the module's own seeded init, the loop through autograd, the
    reference's output tree under the arch's name"""
    import os
    import main_attack
    monkeypatch.chdir(tmp_path)
    args = ["--attack", "GeoA3", "--attack_label", "Untarget", "-b", "125", "--npoint", "64", "--arch", "DGCNN", "--synthetic",
            "--data_dir_file", str(tmp_path / "Data" / "syn64.mat"), "--binary_max_steps", "1", "--iter_max_steps", "3",
            "--lr", "0.005", "--curv_loss_knn", "8", "--quiet"]
    saved_dir = main_attack.main(main_attack.build_parser().parse_args(args))
    assert saved_dir.startswith(os.path.join("Exps", "DGCNN_npoint64", "Untarget", "GeoA3_0_BiStep1_IterStep3_"))
    res = open(os.path.join(saved_dir, "attack_result.txt")).read()
    assert res.startswith("attack success: ") and 0.0 <= float(res.split(":")[1]) <= 100.0


def test_attack_runner_is_reproducible():
    """AttackRunner drives the module through autograd (no native path for it): 1 binary step x 5 iterations at B = 4,
    N = 64, twice from the same state -- every tensor of runner.t bit-identical.  (All but the `*scratch` entries: those are
    the uninitialised work buffers of geoa3_knn_self -- "contents irrelevant" in include/geoa3_hip.h -- which a fresh
    runner allocates anew; they hold no state of the attack.)"""
    from geoa3_amd.attack import AttackRunner
    from oracle import geoa3_oracle as O
    net = make_net(16).cuda()
    B, N = 4, 64
    pc = _cloud(B, N, 17)
    nrm = pc / pc.norm(dim=1, keepdim=True)
    gt = torch.tensor([0, 3, 7, 11])
    init = torch.randn(B, 3, N, generator=torch.Generator().manual_seed(18)) * 1e-3
    cfg = O.AttackCfg(binary_max_steps=1, iter_max_steps=5, npoint=N, curv_loss_knn=8)
    states = []
    for _ in range(2):
        r = AttackRunner(net, B, N, cfg, torch.device("cuda"))
        assert not r.native
        r.setup(pc, nrm, gt, gt)
        r.run([init.cuda()])
        torch.cuda.synchronize()
        state = {}
        for k, v in r.t.items():
            if k.endswith("scratch"):
                continue
            if isinstance(v, torch.Tensor):
                state[k] = v.detach().cpu().clone()
            else:   # a list / tuple of tensors: the double-buffered K-NN tables
                assert isinstance(v, (list, tuple)) and all(isinstance(e, torch.Tensor) for e in v), (k, type(v))
                state.update({"%s[%d]" % (k, n): e.detach().cpu().clone() for n, e in enumerate(v)})
        states.append(state)
    assert states[0].keys() == states[1].keys() and len(states[0]) > 20
    assert any("[" in k for k in states[0])               # the list-valued tables are among them
    for k in states[0]:
        a, b = states[0][k], states[1][k]
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(a.numpy().view(np.uint8), b.numpy().view(np.uint8)), k
    assert not torch.equal(states[0]["x"], pc)           # the iterate moved
