"""The T-Nets' 1024-wide layer (wide_split_kernel, taps = 1) at shapes where a workgroup owns MORE THAN ONE work unit,
driven through the layer alone (geoa3_debug_wide_fwd, pack_wide_split / pack_wide_fragments).

The kernel carries its A fragments (k-step 0 of the LDS image) from one channel group to the next and issues one more,
dead, refill after a unit's last group; its weight ring runs across the groups.  The other layer tests
(test_gpu_wide_epilogue.py, test_gpu_wide16_units.py, test_gpu_pointnet.py) run at most one unit per workgroup, so
state that leaks from one unit into the next shows only here.

Work units: instance b runs on XCD b % 8; an XCD's units (instance, 128-point tile) are dealt to its 64 workgroup slots
round robin, unit u to slot u % 64.
  B = 72, N = 1024 / 1000: 9 instances x 8 tiles = 72 units per XCD, so slots 0 .. 7 take a second unit (a tile of
    instance xcd + 64), among them late workgroups, which run their first unit in two halves; N = 1000 has a ragged tile.
  B = 9, N = 4225: XCD 0 holds instances 0 and 8 with 34 tiles each = 68 units, so slots 0 .. 3 run a tile of instance 0
    and then tiles 30 .. 33 of instance 8 (the last one ragged: one point).

Bars.  Values: |got - ref| <= 1e-5 |ref| + 1e-5 max_row |ref| against a float64 einsum + max (the split-fp16 product
drops 2^-24-relative terms: 6e-8 of sum |a w|, which is a few times the maximum here).  Arg-max: the float64 one wherever
it leads the runner-up by more than 1e-4 relative."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def layer():
    from geoa3_amd.pointnet import pack_wide_fragments, pack_wide_split
    g = torch.Generator().manual_seed(41)
    W = torch.randn(1024, 128, generator=g) * 0.05
    bias = torch.randn(1024, generator=g)
    Wh, uns = pack_wide_split(W)
    return W, bias, (pack_wide_fragments(W, 1).cuda(), Wh.cuda(), uns, bias.cuda())


def run(x, dev):
    from geoa3_amd import _lib
    lib = _lib.load()
    Wp, Wh, uns, bd = dev
    b, _, n = x.shape
    out = torch.empty(b, 1024, device="cuda")
    arg = torch.empty(b, 1024, device="cuda", dtype=torch.int32)
    keys = torch.empty(b, 1024, device="cuda", dtype=torch.int64)
    xd = x.cuda().contiguous()
    _lib.check(lib.geoa3_debug_wide_fwd(xd.data_ptr(), Wp.data_ptr(), Wh.data_ptr(), uns, bd.data_ptr(), out.data_ptr(),
                                        arg.data_ptr(), keys.data_ptr(), b, n, 1, None,
                                        torch.cuda.current_stream().cuda_stream), "geoa3_debug_wide_fwd")
    return out.cpu(), arg.cpu()


def reference(X, W, bias):
    """float64: pooled feature relu(max + bias), first arg-max, relative lead of the maximum over the next VALUE."""
    tops, args, leads = [], [], []
    for x in X.double().split(8):                   # (8 instances at a time: 64 MB of float64 products)
        conv = torch.einsum("oc,bcn->bon", W.double(), x)
        top, arg = conv.max(dim=2)                  # (first occurrence)
        second = conv.masked_fill(conv == top.unsqueeze(2), -float("inf")).max(dim=2).values
        tops.append(top), args.append(arg), leads.append((top - second) / top.abs())
    top, arg, lead = torch.cat(tops), torch.cat(args), torch.cat(leads)
    return (top + bias.double()).clamp_min(0), arg, lead


def assert_values(out, ref):
    tol = 1e-5 * ref.abs() + 1e-5 * ref.abs().max(dim=1, keepdim=True).values
    err = (out.double() - ref).abs()
    print("largest value error / bar %.3f" % float((err / tol).max()))
    assert (err <= tol).all()


def assert_same_bits(o1, a1, o2, a2, what):
    assert torch.equal(o1.view(torch.int32), o2.view(torch.int32)) and torch.equal(a1, a2), what


@functools.lru_cache(maxsize=None)
def two_unit_case(N):
    B = 72
    W, bias, dev = layer()
    X = torch.randn(B, 128, N, generator=torch.Generator().manual_seed(N)).relu()
    out, arg = run(X, dev)
    return (X, out, arg) + reference(X, W, bias)


@pytest.mark.parametrize("N", [1024, 1000])
def test_two_units_per_workgroup_against_float64(N):
    X, out, arg, ref, ref_arg, lead = two_unit_case(N)
    assert_values(out, ref)
    clear = lead > 1e-4
    print("N %d: clear share %.4f" % (N, float(clear.float().mean())))
    assert float(clear.float().mean()) > 0.9
    assert torch.equal(arg.long()[clear], ref_arg[clear])
    assert int(arg.min()) >= 0 and int(arg.max()) < N


@pytest.mark.parametrize("N", [1024, 1000])
def test_two_units_per_workgroup_rows_and_repeat(N):
    """Every row bit for bit its batch-1 run (alone, an instance's 8 units have a workgroup each); two runs equal."""
    X, out, arg = two_unit_case(N)[:3]
    dev = layer()[2]
    out2, arg2 = run(X, dev)
    assert_same_bits(out, arg, out2, arg2, "two runs of the same batch differ")
    for b in range(X.shape[0]):
        o1, a1 = run(X[b:b + 1], dev)
        assert_same_bits(o1[0], a1[0], out[b], arg[b], "row %d differs from its batch-1 run" % b)


@functools.lru_cache(maxsize=None)
def tie_draw():
    """One generator, seed 3: activations [3, 128, 64], then the weights (the draw of tests/test_gpu_wide_epilogue.py)."""
    g = torch.Generator().manual_seed(3)
    X64 = torch.randn(3, 128, 64, generator=g).relu()
    W = torch.randn(1024, 128, generator=g) * 0.05
    bias = torch.randn(1024, generator=g)
    from geoa3_amd.pointnet import pack_wide_fragments, pack_wide_split
    Wh, uns = pack_wide_split(W)
    return X64, W, bias, (pack_wide_fragments(W, 1).cuda(), Wh.cuda(), uns, bias.cuda())


@pytest.mark.parametrize("N", [1, 32, 127, 128, 129, 257])
def test_tied_maxima_land_on_the_first_occurrence(N):
    """Activations of period 64 along the points: point n repeats point n % 64 with the same bits, so beyond 64 points
    every maximum is tied (inside a tile, across tiles and across the units' keys) and the first occurrence must win.
    Left out: (instance, channel) pairs whose best two DISTINCT points are within 1e-4 relative -- 0.03 % of them by the
    float64 reference at N >= 64; at most 1 % may be."""
    X64, W, bias, dev = tie_draw()
    X = X64[:, :, torch.arange(N) % 64].contiguous()
    out, arg = run(X, dev)
    P = min(N, 64)
    conv = torch.einsum("oc,bcn->bon", W.double(), X[:, :, :P].double())     # the distinct points
    top, ref_arg = conv.max(dim=2)
    second = conv.scatter(2, ref_arg.unsqueeze(2), -float("inf")).max(dim=2).values   # -inf when there is one point only
    clear = (top - second) > 1e-4 * top.abs()
    left_out = 1.0 - float(clear.float().mean())
    print("N %d: left out %.4f %%" % (N, 100 * left_out))
    assert left_out <= 0.01
    assert torch.equal(arg.long()[clear], ref_arg[clear])
    assert_values(out, (top + bias.double()).clamp_min(0))


def test_a_unit_that_follows_a_unit():
    """B = 9, N = 4225: the workgroups in slots 0 .. 3 of XCD 0 run a tile of instance 0 and then a tile of instance 8.
    Every activation of instance 8 is smaller than every activation of instance 0 (>= 8 against <= 1), so an A fragment
    left over from the previous unit shows as a maximum that is too large, not as noise."""
    W, bias, dev = layer()
    B, N = 9, 4225
    g = torch.Generator().manual_seed(9)
    X = torch.randn(B, 128, N, generator=g).relu()
    X[0] = 8.0 + X[0]
    X[8] = X[8].clamp_max(1.0)
    assert float(X[8].max()) < float(X[0].min())
    out, arg = run(X, dev)
    o8, a8 = run(X[8:9], dev)
    assert_same_bits(o8[0], a8[0], out[8], arg[8], "instance 8 differs from its batch-1 run")
    o0, a0 = run(X[0:1], dev)
    assert_same_bits(o0[0], a0[0], out[0], arg[0], "instance 0 differs from its batch-1 run")
    ref, ref_arg, lead = reference(X[8:9], W, bias)
    assert_values(out[8:9], ref)
    clear = lead[0] > 1e-4
    assert float(clear.float().mean()) > 0.9
    assert torch.equal(arg[8].long()[clear], ref_arg[0][clear])


def test_nan_and_inf_in_a_second_unit_poison_their_instance_only():
    """B = 72: instances 64 .. 71 are made of second units only (slots 0 .. 7 of their XCD, behind a tile of instance
    xcd).  A NaN / an inf there turns that instance's 1024 features into NaN and leaves every other row bit for bit."""
    X, out, arg = two_unit_case(1024)[:3]
    dev = layer()[2]
    for poison, where in ((float("nan"), (66, 5, 300)), (float("inf"), (70, 127, 1023)), (-float("inf"), (64, 0, 0))):
        bad = X.clone()
        bad[where] = poison
        o, a = run(bad, dev)
        assert torch.isnan(o[where[0]]).all()
        rest = [b for b in range(X.shape[0]) if b != where[0]]
        assert_same_bits(o[rest], a[rest], out[rest], arg[rest], "a poisoned instance changed another row")
