"""conv5's work units (pointnet_wide16.hip: one unit = instance x 128-point tile x all 1024 channels, one staging pass per
tile): the PointNet forward and input gradient against the CPU oracle at the smallest shapes where the unit logic can go
wrong, at the bars of tests/test_gpu_pointnet.py, plus bit-level repeatability and batch independence.

The CPU oracle's result of a (cloud set, weights) pair is computed once and shared by both arithmetic modes."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import geoa3_oracle as O

pytestmark = pytest.mark.gpu

MODES = ["f16x2", "f32"]      # conv5 runs wide16_kernel in f16x2 only; f32 is held to the same bars beside it


@functools.lru_cache(maxsize=None)
def state_dict():
    from geoa3_amd.data import synthetic_state_dict
    return {k: v.cpu() for k, v in synthetic_state_dict(40, seed=0).items()}


@functools.lru_cache(maxsize=None)
def net(mode):
    from geoa3_amd.pointnet import PointNet
    n = PointNet(40)
    n.load_state_dict(state_dict())
    n.wide_mode = mode
    return n.cuda().eval()


def weights(B):
    return torch.randn(B, 40, generator=torch.Generator().manual_seed(1))


def oracle(pc):
    """logits, d(logits . w)/d pc of the CPU oracle."""
    x = pc.clone().requires_grad_()
    lo = O.pointnet_forward(state_dict(), x)
    (lo * weights(pc.shape[0])).sum().backward()
    return lo.detach().numpy(), x.grad.numpy()


@functools.lru_cache(maxsize=None)
def shape_case(B, N):
    from geoa3_amd.data import synthetic_clouds
    pc, _ = synthetic_clouds(B, N, seed=B * 1000 + N)
    return (pc,) + oracle(pc)


def gpu_run(n, pc, w):
    x = pc.cuda().requires_grad_()
    lg = n(x)
    (lg * w.cuda()).sum().backward()
    return lg.detach().clone(), x.grad.clone()


def assert_grad_close(got, ref):
    """The bar of tests/test_gpu_pointnet.py: rtol 2e-3 / atol 2e-4 of the largest entry, 18 entries per allowed arg-max
    flip, ceil(5e-5 * 3072 * B) flips."""
    scale = np.abs(ref).max()
    bad = np.abs(got - ref) > 2e-3 * np.abs(ref) + 2e-4 * scale
    flips = int(np.ceil(5e-5 * 3072 * got.shape[0]))
    assert bad.sum() <= 18 * flips, "%d of %d gradient entries differ" % (bad.sum(), bad.size)


def check_against_oracle_and_itself(mode, pc, lo, go):
    n, w = net(mode), weights(pc.shape[0])
    lg, dx = gpu_run(n, pc, w)
    np.testing.assert_allclose(lg.cpu().numpy(), lo, rtol=1e-4, atol=3e-4)
    assert_grad_close(dx.cpu().numpy(), go)
    lg2, dx2 = gpu_run(n, pc, w)
    assert torch.equal(lg, lg2) and torch.equal(dx, dx2), "two runs of the same batch differ"
    for b in range(pc.shape[0]):
        l1, d1 = gpu_run(n, pc[b:b + 1].contiguous(), w[b:b + 1])
        assert torch.equal(l1[0], lg[b]), "logits of row %d differ from its batch-1 run" % b
        assert torch.equal(d1[0], dx[b]), "input gradient of row %d differs from its batch-1 run" % b


# N: part of one tile; one point short of a tile; exactly one tile; one point into the second tile (a tile that is all
# halo but one row); two tiles and one point (halo rows at both ends of the middle tile).
# B: fewer instances than XCDs; fewer units than workgroup slots (most workgroups own nothing); one XCD with two
# instances (and, on that XCD, a late workgroup whose only unit is run in two halves)
@pytest.mark.parametrize("N", [32, 127, 128, 129, 257])
@pytest.mark.parametrize("B", [1, 7, 9])
@pytest.mark.parametrize("mode", MODES)
def test_units_against_oracle(mode, B, N):
    check_against_oracle_and_itself(mode, *shape_case(B, N))


def conv5_activations(sd, pc):
    """The oracle's conv5 + bn5 + relu output [B,1024,N] before the max over points (pointnet_forward up to there)."""
    eps = 1e-3
    t3 = O._tnet_forward(sd, "input_transform.", pc, 3)
    f = torch.bmm(pc.permute(0, 2, 1), t3).permute(0, 2, 1)
    f = F.relu(O._bn(F.conv1d(f, sd["conv1.weight"], sd["conv1.bias"]), sd, "bn1", eps))
    f = F.relu(O._bn(F.conv1d(f, sd["conv2.weight"], sd["conv2.bias"]), sd, "bn2", eps))
    t64 = O._tnet_forward(sd, "feature_transform.", f, 64)
    f = torch.bmm(f.permute(0, 2, 1), t64).permute(0, 2, 1)
    f = F.relu(O._bn(F.conv1d(f, sd["conv3.weight"], sd["conv3.bias"]), sd, "bn3", eps))
    f = F.relu(O._bn(F.conv1d(f, sd["conv4.weight"], sd["conv4.bias"]), sd, "bn4", eps))
    return F.relu(O._bn(F.conv1d(f, sd["conv5.weight"], sd["conv5.bias"], padding=1), sd, "bn5", eps))


@functools.lru_cache(maxsize=None)
def boundary_case():
    """Two clouds of 257 points (tiles 0..127, 128..255, 256).
    Cloud 0: a small ellipsoid with two far outliers at points 127 and 128, so that many channels peak in the windows
    around them: a maximum at 127 needs the right halo row of tile 0 (point 128), one at 128 the left halo row of tile 1.
    Cloud 1: 64 points repeated with period 64: every interior window occurs four times, in both full tiles, with the
    same bits (the tiles hold the same values, so the same scale); each channel's maximum is an exact tie and the
    gradient must land on the first occurrence, as torch's max does."""
    from geoa3_amd.data import synthetic_clouds
    N = 257
    base, _ = synthetic_clouds(2, N, seed=77)
    a = base[0] * 0.3
    a[:, 127] = torch.tensor([0.9, 0.1, -0.3])
    a[:, 128] = torch.tensor([-0.2, -0.95, 0.1])
    b = base[1][:, torch.arange(N) % 64]
    pc = torch.stack([a, b]).contiguous()
    z = conv5_activations(state_dict(), pc)
    top, arg = z.max(-1)
    second = z.scatter(2, arg.unsqueeze(2), -float("inf")).max(-1).values
    clear = (top - second) > 1e-3 * top.abs()
    # the clouds do what they are built for (oracle side; measured: 54 / 44 clear channels at 127 / 128)
    assert int(((arg[0] == 127) & clear[0]).sum()) >= 8 and int(((arg[0] == 128) & clear[0]).sum()) >= 8
    assert torch.equal(z[1][:, 1:64], z[1][:, 65:128]) and torch.equal(z[1][:, 65:128], z[1][:, 129:192])
    live = top[1] > 0
    assert int(live.sum()) > 256 and int(((arg[1] >= 1) & (arg[1] < 64) & live).sum()) > 256   # tied maxima, first occurrence
    return (pc,) + oracle(pc)


@pytest.mark.parametrize("mode", MODES)
def test_maxima_at_the_tile_boundary_and_ties(mode):
    check_against_oracle_and_itself(mode, *boundary_case())


@pytest.mark.parametrize("mode", MODES)
def test_nan_coordinate_stays_in_its_instance(mode):
    """One NaN coordinate (instance 1 of 3, a point of the second tile).  A NaN coordinate does not reach the 1024-wide
    layers as a NaN: the relu of the narrow convolutions in front of them returns 0 for it, and the instance's logits
    are finite numbers (measured on the parent commit and on this one).  What holds, and is held here: the row is what
    it was -- bit for bit its batch-1 result, NaN or not --, and the other two rows are bit for bit theirs.  The
    poisoning of conv5's pooled features by a non-finite value in conv5's own input is test_conv5_layer_nan_rows_and_ties."""
    from geoa3_amd.data import synthetic_clouds
    pc, _ = synthetic_clouds(3, 257, seed=5)
    pc[1, 2, 130] = float("nan")
    n = net(mode)
    with torch.no_grad():
        lg = n(pc.cuda()).clone()
        for b in range(3):
            alone = n(pc[b:b + 1].cuda().contiguous())[0]
            assert torch.equal(alone.view(torch.int32), lg[b].view(torch.int32)), "row %d differs from its batch-1 run" % b
        assert torch.isfinite(lg[[0, 2]]).all()


def test_conv5_layer_nan_rows_and_ties():
    """The layer alone (geoa3_debug_wide_fwd, split-fp16 packing): activations with period 64 along the points tie every
    maximum, and the arg-max is the first occurrence (< 65); a NaN or an inf activation poisons all 1024 features of its
    instance and leaves the other rows bit for bit what they are alone."""
    from geoa3_amd import _lib
    from geoa3_amd.pointnet import pack_wide_fragments, pack_wide_split16
    lib = _lib.load()
    B, N = 3, 257
    g = torch.Generator().manual_seed(3)
    X = torch.randn(B, 128, 64, generator=g).relu()[:, :, torch.arange(N) % 64].contiguous()
    W = torch.randn(1024, 3 * 128, generator=g) * 0.05
    bias = torch.randn(1024, generator=g)
    Wp, (Wh, uns) = pack_wide_fragments(W, 3).cuda(), pack_wide_split16(W)
    Wh, bd = Wh.cuda(), bias.cuda()
    s = torch.cuda.current_stream().cuda_stream

    def run(x):
        b = x.shape[0]
        out = torch.empty(b, 1024, device="cuda")
        arg = torch.empty(b, 1024, device="cuda", dtype=torch.int32)
        keys = torch.empty(b, 1024, device="cuda", dtype=torch.int64)
        xd = x.cuda().contiguous()
        _lib.check(lib.geoa3_debug_wide_fwd(xd.data_ptr(), Wp.data_ptr(), Wh.data_ptr(), uns, bd.data_ptr(),
                                            out.data_ptr(), arg.data_ptr(), keys.data_ptr(), b, N, 3, None, s),
                   "geoa3_debug_wide_fwd")
        return out.cpu(), arg.cpu()

    out, arg = run(X)
    conv = F.conv1d(X.double(), W.double().view(1024, 3, 128).permute(0, 2, 1), padding=1)
    ref, ref_arg = conv.max(dim=2)     # (first occurrence)
    interior = (ref_arg >= 1) & (ref_arg < 64)
    second = conv[:, :, :65].scatter(2, ref_arg.clamp(max=64).unsqueeze(2), -float("inf")).max(dim=2).values
    clear = interior & ((ref - second) > 1e-4 * ref.abs())     # the runner-up among the DISTINCT windows is not within rounding
    assert clear.float().mean() > 0.5
    assert torch.equal(arg.long()[clear], ref_arg[clear])
    for poison, where in ((float("nan"), (1, 100, 0)), (float("inf"), (1, 5, 128)), (float("nan"), (1, 0, 256))):
        bad = X.clone()
        bad[where] = poison
        o, a = run(bad)
        assert torch.isnan(o[1]).all()
        assert torch.equal(o[[0, 2]], out[[0, 2]]) and torch.equal(a[[0, 2]], arg[[0, 2]])
    for b in range(B):
        o1, a1 = run(X[b:b + 1])
        assert torch.equal(o1[0], out[b]) and torch.equal(a1[0], arg[b])
