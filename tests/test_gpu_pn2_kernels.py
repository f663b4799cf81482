"""Kernels of the PointNet++ SSG native path ALONE (the geoa3_debug_pn2_* entries of include/geoa3_hip_debug.h) against the
float64 restatements of tests/_pn2_native_ref.py, at the cases of tests/_pn2_native_cases.py.

Bound, as for the PointNet kernels (tests/test_gpu_pointnet_bwd.py): |got - ref| <= 4 sqrt(n) 2^-24 mag + 2^-22 |ref|, n = the
terms of the longest sum behind an entry, mag = the float64 sum of the absolute products behind it, plus 2^-21 mag for a
product of split-fp16 operands: a value v scaled by a power of two into the binade [2^e, 2^(e+1)) is carried as hi = fp16(v)
and lo = fp16(v - hi); |v - hi| <= 2^(e-11) is exact in fp32 and rounds to fp16 within 2^(e-23), so |v - hi - lo| <= 2^-23 |v|;
a w = a_hi w_hi + a_hi w_lo + a_lo w_hi carries both representation errors (2 x 2^-23 |a w|) and lacks a_lo w_lo (at most
2^-22 |a w|): 2^-21 |a w|, summed over the products 2^-21 mag.  An entry whose mag is zero must be exactly zero.

Two chained layers (sa2_fwd8_kernel: y2 = W2 relu(z1) + b2, z1 = W1 a0 + b1, a0 exact): layer 1 alone is the bound above,
tol(z1).  relu is 1-Lipschitz, so the a1 the second product reads is within tol(z1) of the reference's, entry by entry, and
that error passes through W2 as sum_k |W2[c][k]| tol(z1)[k]; on top comes layer 2's own bound on ITS products, with mag(y2) =
sum_k |W2| mag(z1) over the open gates + |b2|: tol(y2) = bound(y2, mag(y2)) + |W2| tol(z1).  relu and the max over the samples
are 1-Lipschitz: tol(out) = max_s tol(y2).  tests/test_pn2_native_ref.py shows on the CPU that these bounds notice one lost
k of either product and hold an emulation of the split arithmetic.  Every test prints its worst err / tol."""
import numpy as np
import pytest
import torch

from tests import _pn2_native_cases as C
from tests import _pn2_native_ref as R

pytestmark = pytest.mark.gpu


def lib_stream():
    from geoa3_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def check_bound(got, ref, tol, what):
    ratio = R.worst_ratio(got.cpu(), ref, tol)
    print("worst err/tol %-48s %.4f" % (what, ratio))
    assert ratio <= 1.0, "%s: worst err / tol = %g" % (what, ratio)
    return ratio


def frag_image(W):
    """-> (img uint8 [4 R K] on the device, un [1] on the device)"""
    _lib, lib, s = lib_stream()
    Rw, K = W.shape
    Wd = W.cuda().contiguous()
    img = torch.full((4 * Rw * K,), 0xA5, dtype=torch.uint8, device="cuda")
    un = torch.full((1,), float("nan"), device="cuda")
    _lib.check(lib.geoa3_debug_pn2_frag_image(P(Wd), Rw, K, P(img), P(un), s), "geoa3_debug_pn2_frag_image")
    return img, un


@pytest.mark.parametrize("Rw,K,variant", C.FRAG_CASES)
def test_frag_image_bit_for_bit(Rw, K, variant):
    """pieces and un against the restatement, bit for bit (a matrix of zeros: finite un, zero image; a single entry 2^20
    times the rest: low pieces in fp16's subnormals)"""
    W = C.frag_case(Rw, K, variant)
    img, un = frag_image(W)
    want_un, want = R.frag_image_flat(W.numpy())
    got = img.cpu().numpy().view(np.float16)
    assert np.float32(un.item()).view(np.uint32) == want_un.view(np.uint32)
    assert np.isfinite(un.item()) and un.item() > 0
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))


def sa2_pre(c, with_xyz=True):
    _lib, lib, s = lib_stream()
    img, un = frag_image(c["Wf"])
    f, xyz, Wx = c["f"].cuda(), c["xyz"].cuda(), c["Wx"].cuda()
    Y = torch.full((c["P"], 128), float("nan"), device="cuda")
    _lib.check(lib.geoa3_debug_pn2_sa2_pre(P(f), int(c["channel_major"]), c["Np"], P(xyz) if with_xyz else None, P(img),
                                           P(un), P(Wx) if with_xyz else None, P(Y), c["P"], s), "geoa3_debug_pn2_sa2_pre")
    return Y


@pytest.mark.parametrize("Pn,Np", C.PRE_SHAPES)
def test_sa2_pre_against_float64(Pn, Np):
    """one wavefront, a partial workgroup, several workgroups, a second pass of a workgroup's wavefronts; both layouts of
    the features; with and without the coordinate term; the same bits on a second launch"""
    c = C.pre_case(Pn, Np)
    for with_xyz in (True, False):
        ref, tol = C.pre_reference(c, with_xyz)
        Y = sa2_pre(c, with_xyz)
        check_bound(Y, ref, tol, "sa2_pre P %d Np %d xyz %d" % (Pn, Np, with_xyz))
        assert torch.equal(Y, sa2_pre(c, with_xyz))


@pytest.mark.parametrize("variant", C.PRE_STRESS)
def test_sa2_pre_stress(variant):
    """one point 2^12 times its 31 tile neighbours; a tile of all-zero features with non-zero coordinates"""
    c = C.pre_case(96, 0, variant)
    ref, tol = C.pre_reference(c)
    check_bound(sa2_pre(c), ref, tol, "sa2_pre " + variant)


@pytest.mark.parametrize("ratio", C.WX_RATIOS)
def test_sa2_pre_wx_magnitude(ratio):
    """max|W_x| = ratio max|W_f|: finite and inside the bound for every ratio (W_x rides at the scale of W_f's image, where
    fp16 ends at 65504: tests/test_pn2_native_ref.py::test_sa2_pre_wx_magnitude)"""
    c = C.pre_case(96, 0, "random", ratio)
    ref, tol = C.pre_reference(c)
    Y = sa2_pre(c)
    print("sa2_pre W_x ratio %g: finite %s" % (ratio, bool(torch.isfinite(Y).all())))
    assert bool(torch.isfinite(Y).all())
    check_bound(Y, ref, tol, "sa2_pre W_x ratio %g" % ratio)


def sa2_fwd(c):
    _lib, lib, s = lib_stream()
    B, M, N1 = c["B"], c["M"], c["N1"]
    i1, u1 = frag_image(c["W1"])
    i2, u2 = frag_image(c["W2"])
    d = {k: c[k].cuda().contiguous() for k in ("rT", "gidx", "shift", "b1", "b2")}
    out = torch.full((B, 256, M), float("nan"), device="cuda")
    arg = torch.full((B, 256, M), -1, dtype=torch.int32, device="cuda")
    m0 = torch.full((B * M, 64, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    m1 = m0.clone()
    _lib.check(lib.geoa3_debug_pn2_sa2_fwd(P(d["rT"]), P(d["gidx"]), P(d["shift"]), P(i1), P(u1), P(d["b1"]), P(i2), P(u2),
                                           P(d["b2"]), P(out), P(arg), P(m0), P(m1), B, N1, M, s), "geoa3_debug_pn2_sa2_fwd")
    return out, arg, m0, m1


@pytest.mark.parametrize("B,M,N1,stress", [s + (False,) for s in C.FWD_SHAPES] + [(1, 8, 40, True)])
def test_sa2_fwd_against_float64(B, M, N1, stress):
    """m0 == the float32 a0 > 0 bit for bit; m1 == sign(z1) outside the band |z1| <= tol(z1) (at most 1e-3 of the entries);
    out under the bound; y2 at the kernel's arg within 2 tol of the maximum; arg never a padded sample; an exact tie goes
    to the lower sample; a ball of one live sample, a full ball; stress: a centre 2^10 times its pair partner.  The same bits
    on a second launch."""
    c, r = C.fwd_case(B, M, N1, stress), C.fwd_reference(B, M, N1, stress)
    out, arg, m0, m1 = sa2_fwd(c)
    res = C.fwd_checks(c, r, out.cpu(), arg.cpu(), m0.cpu(), m1.cpu())
    print("worst err/tol %-48s %.4f (band %.2e)" % ("sa2_fwd B %d M %d N1 %d stress %d" % (B, M, N1, stress), res["out"],
                                                    res["band"]))
    again = sa2_fwd(c)
    assert all(torch.equal(x, y) for x, y in zip((out, arg, m0, m1), again))
    if B > 1:       # instance 1 of the batch == its batch-1 run
        one = dict(c, B=1, **{k: c[k][1:2].contiguous() for k in ("rT", "gidx", "shift")})
        o1, a1, g0, g1 = sa2_fwd(one)
        assert torch.equal(o1[0], out[1]) and torch.equal(a1[0], arg[1])
        assert torch.equal(g0, m0[M:2 * M]) and torch.equal(g1, m1[M:2 * M])


# ---------------------------------------------------------------------------------------------------------------------
# the level's backward: sa2b_prep_kernel, sa2b_bwd_kernel, affine3_grad_pm_kernel, sa2b_centre_kernel
# ---------------------------------------------------------------------------------------------------------------------
def sa2b(c, rows=None):
    """-> (dr, dnx1, dnx2, scratch as uint8 [B][bytes]) on the device; rows: a subset of the case's clouds"""
    _lib, lib, s = lib_stream()
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    dev = {k: sel(c[k]).cuda().contiguous() for k in ("dout", "out", "arg", "gidx")}
    B = dev["dout"].shape[0]
    m0 = R.pack_gate_words(sel(c["gate0"])).to(torch.int32).reshape(B * 128, 64, 4).cuda().contiguous()
    m1 = R.pack_gate_words(sel(c["gate1"])).to(torch.int32).reshape(B * 128, 64, 4).cuda().contiguous()
    W2, Wx = c["W2"].cuda().contiguous(), c["Wx"].cuda().contiguous()
    img, un = frag_image(c["W1"].t().contiguous())         # W1^T: the backward's product d a0 = W1^T d a1
    per = int(lib.geoa3_debug_pn2_sa2b_scratch_bytes(1))
    assert per == R.sa2b_scratch_layout()[1] and int(lib.geoa3_debug_pn2_sa2b_scratch_bytes(B)) == B * per
    scratch = torch.full((B, per), 0xEE, dtype=torch.uint8, device="cuda")
    dr = torch.full((B, 512, 128), float("nan"), device="cuda")
    dnx1 = torch.full((B, 512, 3), float("nan"), device="cuda")
    dnx2 = sel(c["dnx2_in"]).cuda().contiguous().clone()
    assert scratch.data_ptr() % 256 == 0
    _lib.check(lib.geoa3_debug_pn2_sa2b(P(dev["dout"]), P(dev["out"]), P(dev["arg"]), P(dev["gidx"]), P(m1), P(m0), P(W2), P(img),
                                        P(un), P(Wx), P(scratch), P(dr), P(dnx1), P(dnx2), B, s), "geoa3_debug_pn2_sa2b")
    return dr, dnx1, dnx2, scratch


@pytest.mark.parametrize("launch", range(len(C.SA2B_LAUNCHES)))
def test_sa2b_against_float64(launch):
    """Three clouds per launch (patterns: tests/_pn2_native_cases.py).  The scratch decoded by the layout of
    include/geoa3_hip_debug.h equals the restatement's tables exactly -- hit mask, row keys (order, last-of-destination marks),
    entries (order, column, last-of-row marks) and their gradients, part cuts, tile descriptors; dr, dnx1, dnx2 and the hit
    rows' coordinate terms are under the bound; rows of dr nobody gathers from are exactly zero (mag == 0); the same bits on a
    second launch; cloud 1 of the batch equals its batch-1 run bit for bit."""
    c = C.sa2b_case(launch)
    ref, tol = C.sa2b_reference(c)
    dr, dnx1, dnx2, scratch = sa2b(c)
    off, per = R.sa2b_scratch_layout()
    raw = scratch.cpu().numpy()
    for b, pat in enumerate(c["patterns"]):
        tb = R.sa2b_tables(c["dout"][b], c["out"][b], c["arg"][b], c["gidx"][b])
        sc = raw[b]
        view = lambda name, dtype, n: sc[off[name]:].view(dtype)[:n]
        Rn, En, Tn = len(tb["keys"]), len(tb["ec"]), len(tb["td"])
        assert np.array_equal(view("hit", np.uint64, 128), tb["hit"]), pat
        assert np.array_equal(view("keys", np.int32, Rn), tb["keys"]), pat
        assert np.array_equal(view("ptile", np.int32, 5), tb["ptile"]), pat
        assert np.array_equal(view("td", np.int32, 4 * Tn).reshape(-1, 4), tb["td"].reshape(-1, 4)), pat
        assert np.array_equal(view("ec", np.int32, En), tb["ec"]), pat
        assert np.array_equal(view("eg", np.uint32, En), tb["eg"].view(np.uint32)), pat
        y = torch.from_numpy(view("y", np.float32, 128 * 64 * 3).reshape(128, 64, 3).copy())
        hitrow = torch.zeros(128, 64, dtype=torch.bool)
        if Rn:
            hitrow[tb["rows"][:, 1], tb["rows"][:, 2]] = True
        ry = R.worst_ratio(y[hitrow], ref["y"][0][b][hitrow], tol["y"][b][hitrow]) if Rn else 0.0
        print("worst err/tol %-48s %.4f" % ("sa2b y rows %s" % pat, ry))
        assert ry <= 1.0, (pat, ry)
        for name, got in (("dr", dr), ("dnx1", dnx1), ("dnx2", dnx2)):
            check_bound(got[b], ref[name][0][b], tol[name][b], "sa2b %s %s (%d rows)" % (name, pat, Rn))
        if pat == "zero":
            assert not dr[b].any() and torch.equal(dnx2[b].cpu(), c["dnx2_in"][b])
    again = sa2b(c)
    assert all(torch.equal(x, y) for x, y in zip((dr, dnx1, dnx2), again[:3]))
    one = sa2b(c, rows=[1])
    assert torch.equal(one[0][0], dr[1]) and torch.equal(one[1][0], dnx1[1]) and torch.equal(one[2][0], dnx2[1])
    y0 = off["y"]
    assert torch.equal(one[3][0, :y0], scratch[1, :y0])


def test_pn2ssg_workspace_layout_is_the_workspace():
    """the layout entry: ascending offsets, 256-byte aligned, `end` == geoa3_pn2ssg_workspace_bytes (no GPU work)"""
    import ctypes
    _lib, lib, _ = lib_stream()
    names = (ctypes.c_char_p * 64)()
    offs = (ctypes.c_int64 * 64)()
    for B, N in ((1, 32), (3, 1024), (2, 100)):
        n = lib.geoa3_debug_pn2ssg_workspace_layout(B, N, names, offs, 64)
        got = [names[i].decode() for i in range(n)]
        assert got[0] == "xyz" and got[-1] == "end" and len(set(got)) == n and {"r", "df1", "d1", "f1", "m0", "m1"} <= set(got)
        o = [offs[i] for i in range(n)]
        assert o == sorted(o) and all(v % 256 == 0 for v in o) and o[-1] == lib.geoa3_pn2ssg_workspace_bytes(B, N)
    assert lib.geoa3_debug_pn2ssg_workspace_layout(1, 16, names, offs, 64) == -1
