"""The arg-max epilogue of the two max-fused 1024-wide split-fp16 kernels, driven through the layer alone
(geoa3_debug_wide_fwd): taps = 3 is conv5 (wide16_kernel, 16x16x32 accumulators: a lane holds 32 points of one channel),
taps = 1 the T-Nets' conv3 (wide_split_kernel, 32x32x16: 64 points per lane).

The epilogue takes the lane's maximum first and then the lowest point whose accumulator equals it; lanes are merged by
shuffles, point tiles and units by the 64-bit atomicMax keys.  What is held here: the FIRST maximal point wins at every
one of those levels (periodic activations tie the maxima at a chosen distance), ragged tiles and the late workgroup's
split unit, zero and negative maxima, the NaN / inf poisoning, batch-row independence and repeatability.

Values: the bar of tests/test_gpu_pointnet.py::test_wide_layer_shipped_packing_against_float64 (4e-6 sum |a w| + 2e-7
(|max| + |bias|)).  Arg-max: the float64 convolution's first arg-max wherever the runner-up among the DISTINCT windows
is clearly below the maximum.

The file checks behaviour the one-pass epilogue it was written against had as well: 34 / 34 cases pass on the build
before the two-pass epilogue and on the one with it (MI355X, 2.6 s)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TAPS = [3, 1]


def pack(W, bias, taps):
    from geoa3_amd.pointnet import pack_wide_fragments, pack_wide_split, pack_wide_split16
    Wh, uns = (pack_wide_split16 if taps == 3 else pack_wide_split)(W)
    return pack_wide_fragments(W, taps).cuda(), Wh.cuda(), uns, bias.cuda()


@functools.lru_cache(maxsize=None)
def periodic_case(taps, P, B=3, N=257):
    """Activations of period P along the points, weights and bias, drawn as tests/test_gpu_wide16_units.py::
    test_conv5_layer_nan_rows_and_ties draws them (one generator, seed 3: activations, weights, bias)."""
    g = torch.Generator().manual_seed(3)
    X = torch.randn(B, 128, P, generator=g).relu()[:, :, torch.arange(N) % P].contiguous()
    W = torch.randn(1024, taps * 128, generator=g) * 0.05
    bias = torch.randn(1024, generator=g)
    return X, W, bias, pack(W, bias, taps)


@functools.lru_cache(maxsize=None)
def layer(taps, negative=False):
    g = torch.Generator().manual_seed(30 + taps)
    W = torch.randn(1024, taps * 128, generator=g) * 0.05
    if negative:
        W = -W.abs()
    bias = torch.randn(1024, generator=g)
    return W, bias, pack(W, bias, taps)


def run(taps, x, dev):
    from geoa3_amd import _lib
    lib = _lib.load()
    Wp, Wh, uns, bd = dev
    b, _, n = x.shape
    out = torch.empty(b, 1024, device="cuda")
    arg = torch.empty(b, 1024, device="cuda", dtype=torch.int32)
    keys = torch.empty(b, 1024, device="cuda", dtype=torch.int64)
    xd = x.cuda().contiguous()
    _lib.check(lib.geoa3_debug_wide_fwd(xd.data_ptr(), Wp.data_ptr(), Wh.data_ptr(), uns, bd.data_ptr(), out.data_ptr(),
                                        arg.data_ptr(), keys.data_ptr(), b, n, taps, None,
                                        torch.cuda.current_stream().cuda_stream), "geoa3_debug_wide_fwd")
    return out.cpu(), arg.cpu()


def conv64(X, W, taps):
    return F.conv1d(X.double(), W.double().view(1024, taps, 128).permute(0, 2, 1), padding=taps // 2)


def value_tol(X, W, bias, taps, top):
    mag = conv64(X.abs(), W.abs(), taps).max(dim=2).values          # bound on sum |a w|
    return 4e-6 * mag + 2e-7 * (top.abs() + bias.double().abs())


@functools.lru_cache(maxsize=None)
def tie_reference(taps, P):
    """Periodic activations: the first point of every distinct window, the float64 maximum over those, its point (the
    first arg-max), the runner-up among them, and the value tolerance."""
    B, N = 3, 257
    X, W, bias, _ = periodic_case(taps, P, B, N)
    conv = conv64(X, W, taps)
    # distinct windows.  One tap: point n repeats point n mod P.  Three taps (zero padded): point 0 and point N - 1 are
    # windows of their own, points 1 .. N - 2 repeat with period P
    reps = torch.arange(P) if taps == 1 else torch.cat([torch.arange(P + 1), torch.tensor([N - 1])])
    vals = conv[:, :, reps]
    top, k = vals.max(dim=2)
    second = vals.scatter(2, k.unsqueeze(2), -float("inf")).max(dim=2).values     # -inf when there is one window only
    return X, reps[k], top, second, value_tol(X, W, bias, taps, top)


@pytest.mark.parametrize("P", [1, 2, 4, 8, 16, 32, 128])
@pytest.mark.parametrize("taps", TAPS)
def test_ties_go_to_the_first_point(taps, P):
    """Period P along the points ties each maximum N / P times: P < 4 inside a lane's registers of one accumulator tile
    (conv5: points 16 t + 4 q + r; T-Net: 32 t + 8 (r >> 2) + 4 h + (r & 3)), P = 4 .. 32 across the lanes the shuffles
    merge and across accumulator tiles, P = 128 across point tiles and units (equal keys differ in the point bits only)."""
    X, ref_arg, top, second, tol = tie_reference(taps, P)
    _, _, bias, dev = periodic_case(taps, P)
    out, arg = run(taps, X, dev)
    ref_out = (top + bias.double()).clamp_min(0)
    err = ((out.double() - ref_out).abs() / tol).max()
    clear = (top - second) > 1e-4 * top.abs()
    wrong = int((arg.long()[clear] != ref_arg[clear]).sum())
    print("taps %d P %3d: clear share %.4f, wrong arg-max %d of %d, value error / bar %.3f"
          % (taps, P, float(clear.float().mean()), wrong, int(clear.sum()), float(err)))
    assert float(clear.float().mean()) >= 0.99
    assert wrong == 0
    assert float(err) <= 1.0


@functools.lru_cache(maxsize=None)
def shape_reference(taps, N, kind):
    """B = 9: XCD 0 holds instances 0 and 8, and its late workgroup runs its only unit in two halves."""
    B = 9
    g = torch.Generator().manual_seed(taps * 1000 + N)
    X = torch.randn(B, 128, N, generator=g).relu()
    if kind == "zero":
        X[1] = 0.0                                   # every tile of the instance
        if N > 128:
            X[2][:, 128:256] = 0.0                   # one whole tile between two that are not
    W, bias, _ = layer(taps, negative=kind == "negative")
    conv = conv64(X, W, taps)
    top, ref_arg = conv.max(dim=2)                   # (first occurrence)
    second = conv.masked_fill(conv == top.unsqueeze(2), -float("inf")).max(dim=2).values   # among the other VALUES
    return X, ref_arg, top, second, value_tol(X, W, bias, taps, top)


def check_shape_case(taps, N, kind):
    X, ref_arg, top, second, tol = shape_reference(taps, N, kind)
    W, bias, dev = layer(taps, negative=kind == "negative")
    out, arg = run(taps, X, dev)
    ref_out = (top + bias.double()).clamp_min(0)
    assert ((out.double() - ref_out).abs() <= tol).all(), float(((out.double() - ref_out).abs() / tol).max())
    clear = (top - second) > 2 * tol
    assert float(clear.float().mean()) > 0.7
    assert torch.equal(arg.long()[clear], ref_arg[clear])
    assert int(arg.min()) >= 0 and int(arg.max()) < N
    out2, arg2 = run(taps, X, dev)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(arg, arg2), "two calls differ"
    return X, out, arg, bias


# N: one point; one point short of a tile; one tile; one point into the second tile; two tiles and one point
@pytest.mark.parametrize("N", [1, 127, 128, 129, 257])
@pytest.mark.parametrize("taps", TAPS)
def test_ragged_tiles_and_the_split_unit(taps, N):
    check_shape_case(taps, N, "random")


@pytest.mark.parametrize("N", [127, 257])
@pytest.mark.parametrize("taps", TAPS)
def test_all_zero_tiles(taps, N):
    """An instance of zeros: every accumulator of every tile is a zero, so every channel's arg-max is point 0 and the
    feature is relu(bias); and an instance whose middle tile is zeros between two that are not (a channel whose other
    windows are all negative peaks on the first zero window)."""
    X, out, arg, bias = check_shape_case(taps, N, "zero")
    assert int(arg[1].abs().max()) == 0
    assert torch.equal(out[1], bias.clamp_min(0))


@pytest.mark.parametrize("N", [129, 257])
@pytest.mark.parametrize("taps", TAPS)
def test_all_negative_preactivations(taps, N):
    """Weights <= 0 on activations >= 0: every maximum is negative (the keys' other branch of the order-preserving map)."""
    X, out, arg, bias = check_shape_case(taps, N, "negative")
    top = shape_reference(taps, N, "negative")[2]
    assert float(top.max()) < 0


@pytest.mark.parametrize("taps", TAPS)
def test_poisoning_and_row_independence(taps):
    """A NaN or an inf activation poisons all 1024 features of its instance and leaves the other rows bit for bit what
    they are; every row is bit for bit its batch-1 result."""
    B, N = 3, 257
    X, _, _, dev = periodic_case(taps, 64, B, N)
    out, arg = run(taps, X, dev)
    for poison, where in ((float("nan"), (1, 100, 0)), (float("inf"), (1, 5, 128)), (float("nan"), (1, 0, 256)),
                          (-float("inf"), (1, 77, 200))):
        bad = X.clone()
        bad[where] = poison
        o, a = run(taps, bad, dev)
        assert torch.isnan(o[1]).all()
        assert torch.equal(o[[0, 2]], out[[0, 2]]) and torch.equal(a[[0, 2]], arg[[0, 2]])
    for b in range(B):
        o1, a1 = run(taps, X[b:b + 1], dev)
        assert torch.equal(o1[0], out[b]) and torch.equal(a1[0], arg[b])
