"""conv5's 1024-wide layer (wide16_kernel, taps = 3) at shapes where a workgroup owns MORE THAN ONE work unit, driven
through the layer alone (geoa3_debug_wide_fwd, pack_wide_split16 / pack_wide_fragments): the counterpart of
test_gpu_tnet_wide_pipeline.py, whose account of the unit schedule (wide_unit.h) holds here word for word.

What a unit leaves behind for the next one in this kernel: its packed maxima in the pad bytes of the LDS image's rows
while the next tile is staged over the image, the two halo rows, the A fragments carried across the channel groups (and
the dead refill after the last group), the weight ring, and a late workgroup's first unit run in two halves.  The other
conv5 tests (test_gpu_wide16_units.py, test_gpu_pointnet.py) run at most one unit per workgroup below full size.

  B = 72, N = 1024 / 1000: 72 units per XCD on 64 slots, so slots 0 .. 7 take a second unit (a tile of instance
    xcd + 64), late workgroups among them; N = 1000 has a ragged tile.
  B = 9, N = 4225: XCD 0 holds instances 0 and 8 with 34 tiles each = 68 units, so slots 0 .. 3 run a tile of instance 0
    and then tiles 30 .. 33 of instance 8 (the last one ragged: one point, the rest of its image and its right halo zero).

Bars.  Values: |got - ref| <= 1e-5 |ref| + 1e-5 max_row |ref| against a float64 conv1d + max, the bar of the T-Net
test.  With K = 384 the dropped lo * lo terms and the fp32 accumulation are of order 1e-7 of sum |a w| (about 6 for this
draw): roughly 1e-6 against a bar of roughly 3e-5.  Arg-max: the float64 one wherever it leads the next value by more
than 1e-4 relative; at least 90 % of the (instance, channel) pairs must be that clear (the float64 reference's share for
these draws is 0.9987 or more in every block of 8 instances)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def layer():
    """The weight layout of test_conv5_layer_nan_rows_and_ties (test_gpu_wide16_units.py): W [1024][tap * 128 + ci]."""
    from geoa3_amd.pointnet import pack_wide_fragments, pack_wide_split16
    g = torch.Generator().manual_seed(41)
    W = torch.randn(1024, 3 * 128, generator=g) * 0.05
    bias = torch.randn(1024, generator=g)
    Wh, uns = pack_wide_split16(W)
    return W, bias, (pack_wide_fragments(W, 3).cuda(), Wh.cuda(), uns, bias.cuda())


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
                                        arg.data_ptr(), keys.data_ptr(), b, n, 3, None,
                                        torch.cuda.current_stream().cuda_stream), "geoa3_debug_wide_fwd")
    return out.cpu(), arg.cpu()


def reference(X, W, bias):
    """float64: pooled feature relu(max + bias), first arg-max, relative lead of the maximum over the next VALUE."""
    Wk = W.double().view(1024, 3, 128).permute(0, 2, 1)
    tops, args, leads = [], [], []
    for x in X.double().split(8):                   # (8 instances at a time)
        conv = F.conv1d(x, Wk, padding=1)
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


def assert_argmax(arg, ref_arg, lead, what):
    clear = lead > 1e-4
    print("%s: clear share %.4f" % (what, float(clear.float().mean())))
    assert float(clear.float().mean()) >= 0.9
    assert torch.equal(arg.long()[clear], ref_arg[clear])


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
    assert_argmax(arg, ref_arg, lead, "N %d" % N)
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


def test_a_unit_that_follows_a_unit():
    """B = 9, N = 4225: the workgroups in slots 0 .. 3 of XCD 0 run a tile of instance 0 and then a tile of instance 8.
    Every activation of instance 8 is smaller than every activation of instance 0 (<= 1 against >= 8), so an A fragment
    or a halo row left over from the previous unit shows as a maximum that is too large, not as noise."""
    W, bias, dev = layer()
    B, N = 9, 4225
    X = torch.randn(B, 128, N, generator=torch.Generator().manual_seed(9)).relu()
    X[0] = 8.0 + X[0]
    X[8] = X[8].clamp_max(1.0)
    assert float(X[8].max()) < float(X[0].min())
    out, arg = run(X, dev)
    for b in (0, 8):
        o1, a1 = run(X[b:b + 1], dev)
        assert_same_bits(o1[0], a1[0], out[b], arg[b], "instance %d differs from its batch-1 run" % b)
    ref, ref_arg, lead = reference(X[8:9], W, bias)
    assert_values(out[8:9], ref)
    assert_argmax(arg[8:9], ref_arg, lead, "instance 8")


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
