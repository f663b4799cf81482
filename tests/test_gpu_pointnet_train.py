"""geoa3_amd.pointnet.PointNet in training mode against the float64 restatement of tests/_pointnet_train_ref.py (B = 4,
N = 128, 5 classes, dropout off): logits, transform and every parameter's gradient within that file's bound, for the fused
wide layers and for wide_train = 'torch'; no selection can flip (asserted on the float64 side).  Then three optimiser steps,
save, load into a fresh module: the eval forward through the existing kernels is the trained module's, bit for bit."""
import functools
import io
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import _pointnet_train_ref as M      # noqa: E402

pytestmark = pytest.mark.gpu
B, N, CLASSES = 4, 128, 5


def objective(logits, transform, G, H):
    return (logits * G).sum() + (transform * H).sum()


@functools.lru_cache(maxsize=None)
def reference():
    sd = M.make_state_dict(CLASSES, M.CASE_SEED)
    pc = M.make_cloud(B, N, M.CASE_SEED)
    g = torch.Generator().manual_seed(9)
    G, H = torch.randn(B, CLASSES, generator=g), torch.randn(B, 64, 64, generator=g) * 0.05
    p = {k: v.double() for k, v in sd.items()}
    names = [k for k, v in p.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    for k in names:
        p[k].requires_grad_()
    wide = []
    logits, transform = M.forward(p, pc.double(), wide)
    margins = M.selection_margins(p, wide)
    objective(logits, transform, G.double(), H.double()).backward()
    return dict(sd=sd, pc=pc, G=G, H=H, logits=logits.detach(), transform=transform.detach(),
                grads={k: p[k].grad for k in names}, margins=margins)


def make_net(sd, mode):
    from geoa3_amd.pointnet import PointNet
    net = PointNet(CLASSES)
    net.load_state_dict(sd)
    net.drop1.p = net.drop2.p = 0.0
    net.wide_train = mode
    return net.cuda().train()


def test_no_selection_of_the_case_can_flip():
    margins = reference()["margins"]
    print(margins)
    assert len(margins) == 3 and all(m > 1.0 for m in margins.values()), margins


@pytest.mark.parametrize("mode", ["fused", "torch"])
def test_training_forward_and_gradients_against_float64(mode):
    r = reference()
    net = make_net(r["sd"], mode)
    out = net(r["pc"].cuda())
    assert isinstance(out, tuple) and len(out) == 2
    logits, transform = out
    assert tuple(logits.shape) == (B, CLASSES) and tuple(transform.shape) == (B, 64, 64)
    objective(logits, transform, r["G"].cuda(), r["H"].cuda()).backward()
    worst = {}

    def hold(name, got, ref, scale):
        assert got is not None and scale > 0, name
        worst[name] = float((got.detach().cpu().double() - ref).abs().max()) / (M.MODULE_REL * scale)

    hold("logits", logits, r["logits"], float(r["logits"].abs().max()))
    hold("transform", transform, r["transform"], float(r["transform"].abs().max()))
    params = dict(net.named_parameters())
    assert set(params) == set(r["grads"])
    scale = {}
    for k, ref in r["grads"].items():        # a group's largest entry (_pointnet_train_ref's docstring)
        scale[M.group_of(k)] = max(scale.get(M.group_of(k), 0.0), float(ref.abs().max()))
    assert len(scale) == 20
    for k, ref in r["grads"].items():
        hold(k, params[k].grad, ref, scale[M.group_of(k)])
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:5]
    print(mode, "worst err/bound:", ["%s %.3f" % kv for kv in top])
    assert top[0][1] <= 1.0, top
    if mode == "fused":      # the fused layer returns the conv bias gradient as exact zeros
        for k in ("conv5.bias", "input_transform.conv3.bias", "feature_transform.conv3.bias"):
            assert bool((params[k].grad == 0).all())
    assert int(net.bn5.num_batches_tracked) == 1 and int(net.input_transform.bn3.num_batches_tracked) == 1


def test_trained_weights_reload_into_the_eval_kernels_bit_for_bit():
    from geoa3_amd.pointnet import PointNet
    r = reference()
    net = make_net(r["sd"], "fused")
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    pc = r["pc"].cuda()
    for _ in range(3):
        opt.zero_grad()
        logits, transform = net(pc)
        objective(logits, transform, r["G"].cuda(), r["H"].cuda()).backward()
        opt.step()
    assert int(net.bn5.num_batches_tracked) == 3
    with torch.no_grad():
        trained = net.eval()(pc)
    assert torch.isfinite(trained).all()
    buf = io.BytesIO()
    torch.save({"state_dict": net.state_dict()}, buf)
    buf.seek(0)
    fresh = PointNet(CLASSES)
    fresh.load_state_dict(torch.load(buf, map_location="cpu")["state_dict"])
    with torch.no_grad():
        again = fresh.cuda().eval()(pc)
    assert torch.equal(trained, again)
    assert not torch.equal(trained, make_net(r["sd"], "fused").eval()(pc).detach())     # the steps moved the weights


def test_adjust_bn_momentum_follows_the_reference_schedule():
    from geoa3_amd.pointnet import PointNet
    net = PointNet(CLASSES)
    for epoch, want in ((1, 0.5), (20, 0.25), (45, 0.125), (200, 0.01)):
        net.adjust_bn_momentum(epoch, 0.5)
        moms = {m.momentum for m in net.modules() if isinstance(m, torch.nn.BatchNorm1d)}
        assert moms == {want}
    assert len([m for m in net.modules() if isinstance(m, torch.nn.BatchNorm1d)]) == 17
    assert not any(k.startswith("drop") for k in net.state_dict())
