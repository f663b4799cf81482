"""Every kernel geoa3_pointnet_backward launches, ALONE (debug entries of include/geoa3_hip_debug.h), against a float64
restatement of what it computes (tests/_pointnet_bwd_ref.py; cases: tests/_pointnet_bwd_cases.py).

Bound, as for the forward kernels: |got - ref| <= 4 sqrt(n) 2^-24 mag + 2^-22 |ref|, n = the number of terms in the longest
sum behind an entry, mag = the float64 sum of the absolute values of the products behind the entry (zero where a gate
closes the entry: such an entry must be exactly zero).  tests/test_pointnet_bwd_ref.py shows on the CPU that each bound
notices one lost term and that a plain fp32 evaluation stays inside it.  Every test prints its worst err / tol."""
import ctypes

import pytest
import torch

from tests import _pointnet_bwd_cases as C
from tests import _pointnet_bwd_ref as R

pytestmark = pytest.mark.gpu


def lib_stream():
    from geoa3_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def check_bound(got, ref, tol, what):
    ratio = R.worst_ratio(got.cpu(), ref, tol)
    print("worst err/tol %-40s %.4f" % (what, ratio))
    assert ratio <= 1.0, "%s: worst err / tol = %g" % (what, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# sparse arg-max backward: wide_max_bwd2_kernel, wide_bwd_conv_kernel<1/3, PRE/no-PRE>, wide_bwd_conv_first_kernel
# ---------------------------------------------------------------------------------------------------------------------
class Sparse:
    """a sparse case on the device"""

    def __init__(self, c, rows=None):
        from geoa3_amd.pointnet import pack_wide_split
        sel = (lambda t: t) if rows is None else (lambda t: t[rows].contiguous())
        self.c, self.taps, self.N = c, c["taps"], c["N"]
        self.g, self.arg = sel(c["g"]).cuda(), sel(c["arg"]).cuda()
        self.B = self.g.shape[0]
        self.W, self.W2t = c["W"].cuda(), c["W2t"].cuda()
        w2th, self.uns = pack_wide_split(c["W2t"])
        self.W2th = w2th.cuda()
        self.gate128, self.gate64 = sel(c["gate128"]), sel(c["gate64"])
        self.m128 = R.pack_gate_bits(self.gate128, tail_ones=True).cuda()     # bits beyond N set: they must not leak
        self.m64 = R.pack_gate_bits(self.gate64, tail_ones=True).cuda()
        self.lists(sel(c["g"]) != 0)
        if "x3" in c:
            self.x3, self.w1, self.b1 = sel(c["x3"]).cuda(), c["w1"].cuda(), c["b1"].cuda()
            self.dx3_in = sel(c["dx3_in"]).cuda()

    def lists(self, live):
        hits, hoff = R.build_hits(self.arg.cpu(), live, self.N, self.taps)
        self.hits, self.hoff = hits.cuda(), hoff.cuda()

    def wide_bwd(self):
        _lib, lib, s = lib_stream()
        Z = torch.where(self.gate128, 1.0, -1.0).cuda()
        dX = torch.full((self.B, 128, self.N), float("nan"), device="cuda")
        _lib.check(lib.geoa3_debug_wide_bwd(P(self.g), P(self.arg), P(self.W), P(Z), P(dX), self.B, self.N, self.taps, s),
                   "geoa3_debug_wide_bwd")
        return dX

    def fused(self, pre, first=False):
        _lib, lib, s = lib_stream()
        if first:
            out = self.dx3_in.clone()
            extra = (None, None, P(self.x3), P(self.w1), P(self.b1), P(out))
        else:
            out = torch.full((self.B, 64, self.N), float("nan"), device="cuda")
            extra = (P(self.m64), P(out), None, None, None, None)
        _lib.check(lib.geoa3_debug_wide_bwd_conv(P(self.g), P(self.arg), P(self.W), P(self.m128), P(self.W2t), P(self.W2th),
                                                 self.uns, *extra, P(self.hits) if pre else None,
                                                 P(self.hoff) if pre else None, self.B, self.N, self.taps, s),
                   "geoa3_debug_wide_bwd_conv")
        return out

    def two_kernels(self, dX):
        """the path the fused kernel replaces: the gated 128 -> 64 convolution (split arithmetic) on the written dX"""
        _lib, lib, s = lib_stream()
        Z = torch.where(self.gate64, 1.0, -1.0).cuda()
        Y = torch.full((self.B, 64, self.N), float("nan"), device="cuda")
        _lib.check(lib.geoa3_debug_conv_cm(P(dX), P(self.W2t), None, P(Z), P(Y), self.B, self.N, 128, 64, 0, 1, s),
                   "geoa3_debug_conv_cm")
        return Y


@pytest.mark.parametrize("taps,N", C.SPARSE_SHAPES)
def test_sparse_backward_against_float64(taps, N):
    """wide_bwd and the fused kernel with and without the forward's hit lists (built here by the Python builder), every
    arg-max pattern of the shape; random gate bits with an all-zero row and the last word's tail set; g with zeros and both
    signs.  Also: the lists change no bit; the fused kernel gives the bits of wide_bwd + the split 128 -> 64 convolution;
    row 1 of the batch is the batch-1 run of instance 1; lists that hold channels with g == 0 stay inside the bound."""
    for pattern in C.sparse_patterns(taps, N):
        c = C.sparse_case(taps, N, pattern)
        dev = Sparse(c)
        tag = "taps %d N %d %s" % (taps, N, pattern)
        ref, tol = C.wide_bwd_reference(c)
        dX = dev.wide_bwd()
        check_bound(dX, ref, tol, "wide_bwd " + tag)
        ref, tol = C.wide_bwd_conv_reference(c)
        plain, pre = dev.fused(False), dev.fused(True)
        check_bound(plain, ref, tol, "wide_bwd_conv " + tag)
        check_bound(pre, ref, tol, "wide_bwd_conv PRE " + tag)
        assert torch.equal(plain, pre), tag
        assert torch.equal(plain, dev.two_kernels(dX)), tag
        if pattern in ("uniform", "col63"):
            one = Sparse(c, rows=[1])
            assert torch.equal(one.wide_bwd()[0], dX[1]), tag
            assert torch.equal(one.fused(False)[0], plain[1]) and torch.equal(one.fused(True)[0], plain[1]), tag
            dev.lists(torch.ones(C.B, 1024, dtype=torch.bool))      # as if every channel's pooled output were positive
            check_bound(dev.fused(True), ref, tol, "wide_bwd_conv PRE, g == 0 listed " + tag)


def test_sparse_backward_stress_sibling():
    """g over twelve decades (1e-6 .. 1e6) at the shape of a uniform-magnitude case above.  The split product scales a tile
    by its own maximum and keeps 2^-38 of that maximum (fp16 subnormals under a 2^13 scale), so a column only holds the
    bound while its largest term is within ~2^-19 of the tile's: with 3 x 1024 taps over 77 columns every column has one."""
    taps, N = C.STRESS_SHAPE
    c = C.sparse_case(taps, N, "uniform", stress=True)
    dev = Sparse(c)
    ref, tol = C.wide_bwd_reference(c)
    check_bound(dev.wide_bwd(), ref, tol, "wide_bwd stress")
    ref, tol = C.wide_bwd_conv_reference(c)
    plain, pre = dev.fused(False), dev.fused(True)
    check_bound(plain, ref, tol, "wide_bwd_conv stress")
    assert torch.equal(plain, pre)


@pytest.mark.parametrize("N,pattern", C.FIRST_SHAPES)
def test_first_layer_form_against_float64(N, pattern):
    """wide_bwd_conv_first_kernel<PRE / no-PRE>: dx3 is prefilled (the kernel adds into it); the gate is recomputed in fp32
    from the cloud (the CPU test holds every pre-activation of these cases away from zero)."""
    c = C.first_case(N, pattern)
    dev = Sparse(c)
    ref, tol = C.first_reference(c)
    plain, pre = dev.fused(False, first=True), dev.fused(True, first=True)
    check_bound(plain, ref, tol, "first-layer form N %d %s" % (N, pattern))
    assert torch.equal(plain, pre)
    one = Sparse(c, rows=[1])
    assert torch.equal(one.fused(True, first=True)[0], plain[1])


@pytest.mark.parametrize("N", [77, 200, 1024])
def test_hit_lists_of_the_forward_are_the_documented_ones(N):
    """wide_finalize_hits_kernel<1/3>: the lists the forward leaves in the workspace, read out by name, are exactly what the
    Python builder makes of the arg-max tables and pooled outputs beside them (include/geoa3_hip_debug.h)."""
    from oracle import geoa3_oracle as O
    from geoa3_amd.pointnet import PointNet
    _lib, lib, _ = lib_stream()
    net = PointNet(40)
    net.load_state_dict(O.make_pointnet_state_dict(40, seed=0))
    net.wide_mode = "f16x2"
    net = net.cuda().eval()
    Bn = 2
    pc, _ = O.make_synthetic_clouds(Bn, N, seed=3 * Bn + N)
    pc[0, :, N // 2:] = pc[0, :, :1]        # half of the first cloud is one point: long lists on few columns
    x = pc.cuda().requires_grad_()
    net(x).sum().backward()                  # (the backward reads the lists; it must not change them)
    torch.cuda.synchronize()
    ws = net._ws_cache["ws"]
    names, offs = (ctypes.c_char_p * 64)(), (ctypes.c_int64 * 64)()
    n = lib.geoa3_debug_pointnet_workspace_layout(Bn, N, 40, names, offs, 64)
    at = {names[i].decode(): offs[i] for i in range(n)}

    def read(name, dtype, *shape):
        count = 1
        for s in shape:
            count *= s
        return ws[at[name]:at[name] + 4 * count].view(dtype).view(*shape).cpu()

    for arg_n, out_n, hl, ho, taps in (("i3", "p3", "hl3", "ho3", 1), ("iq3", "q3", "hlq", "hoq", 1), ("i5", "p5", "hl5", "ho5", 3)):
        arg, out = read(arg_n, torch.int32, Bn, 1024), read(out_n, torch.float32, Bn, 1024)
        assert 0 < int((out > 0).sum()) and int(arg.min()) >= 0 and int(arg.max()) < N
        hits, hoff = R.build_hits(arg.long(), ~(out <= 0), N, taps)
        got_off, got = read(ho, torch.int32, Bn, N + 1), read(hl, torch.int32, Bn, 1024 * taps)
        assert torch.equal(got_off, hoff), hl
        for b in range(Bn):
            cnt = int(hoff[b, N])
            assert torch.equal(got[b, :cnt], hits[b, :cnt]), (hl, b)


# ---------------------------------------------------------------------------------------------------------------------
# gram64_kernel + gram64_reduce_kernel
# ---------------------------------------------------------------------------------------------------------------------
def run_gram(A, G, N, scratch):
    _lib, lib, s = lib_stream()
    Bn = A.shape[0]
    chunks = (N + 127) // 128
    parts = 8 if chunks >= 8 else (4 if chunks >= 4 else 1)
    sc = torch.full((Bn * parts * 4096,), float("nan"), device="cuda") if scratch else None
    out = torch.full((Bn, 64, 64), float("nan"), device="cuda")
    _lib.check(lib.geoa3_debug_gram64(P(A), P(G), Bn, N, P(out), P(sc), s), "geoa3_debug_gram64")
    return out


@pytest.mark.parametrize("N", C.GRAM_N)
def test_gram_against_float64(N):
    """P = A G^T with and without the partial-sum scratch (1, 4 and 8 parts; a ragged half-chunk, a ragged chunk).

    Bound: n = N, plus 2^-21 mag for the operands' representation.  A value v (scaled by a power of two: exact) in the
    binade [2^e, 2^(e+1)) is carried as hi = fp16(v) and lo = fp16(v - hi).  fp16 has 11 significant bits, so |v - hi| <=
    2^(e-11); v - hi is exact in fp32, and either equals 2^(e-11) (an fp16 value) or lies in a binade at or below [2^(e-12),
    2^(e-11)), where fp16 rounds by at most 2^(e-23): |v - hi - lo| <= 2^-23 |v|.  A product a g is formed as a_hi g_hi +
    a_hi g_lo + a_lo g_hi: it carries the two representation errors, 2 x 2^-23 |a g|, and lacks a_lo g_lo, at most 2^-11 |a|
    2^-11 |g| = 2^-22 |a g|: 2^-21 |a g| in all, summed over the products = 2^-21 mag.  (fp16's subnormal spacing under the
    2^13 scale costs a value 2^38 below its chunk's maximum its low piece; the 1e6 case has its large values in a chunk of
    their own, and 2^-38 of a chunk's maximum per term is far below the bound of an entry that holds that chunk.)"""
    for variant in C.gram_variants(N):
        c = C.gram_case(N, variant)
        ref, tol = C.gram_reference(c)
        A, G = c["A"].cuda(), c["G"].cuda()
        for scratch in (True, False):
            out = run_gram(A, G, N, scratch)
            check_bound(out, ref, tol, "gram N %d %s %s" % (N, variant, "scratch" if scratch else "one part"))
            one = run_gram(A[1:2].contiguous(), G[1:2].contiguous(), N, scratch)
            assert torch.equal(one[0], out[1]), (variant, scratch)
        if variant == "inst_zero":
            assert not bool(out[1].any())


# ---------------------------------------------------------------------------------------------------------------------
# conv_bwd_chain_kernel + reduce_dT_kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", C.CHAIN_N)
def test_backward_chain_against_float64(N):
    """dx and dT of the trunk's front with the input transform, per-instance Wa, gate bits with the last word's tail set;
    n of dT = N (the sum over the points).  Twenty launches give the same bits (the kernel once computed wrong values in a
    few workgroups per 1e4 when built with packed-FP32 instructions: NOTEBOOK 5a; the shipped flags form none)."""
    _lib, lib, s = lib_stream()
    c = C.chain_case(N)
    dx_ref, dx_tol, dT_ref, dT_tol = C.chain_reference(c)
    t = {k: c[k].contiguous().cuda() for k in ("Xa", "Wa", "Xb", "Wb", "W2t", "x3", "T3", "w1", "b1")}
    mask = R.pack_gate_bits(c["gate_h2"], tail_ones=True).cuda()
    nparts = (N + 255) // 256

    def run():
        dx = torch.full((C.B, 3, N), float("nan"), device="cuda")
        part = torch.full((C.B * nparts * 32,), float("nan"), device="cuda")
        dT = torch.full((C.B, 9), float("nan"), device="cuda")
        _lib.check(lib.geoa3_debug_conv_bwd_chain(P(t["Xa"]), P(t["Wa"]), 4096, P(t["Xb"]), P(t["Wb"]), P(mask), P(t["W2t"]),
                                                  P(t["x3"]), P(t["T3"]), P(t["w1"]), P(t["b1"]), P(dx), P(part), P(dT), C.B,
                                                  N, s), "geoa3_debug_conv_bwd_chain")
        return dx, dT.view(C.B, 3, 3)

    dx, dT = run()
    check_bound(dx, dx_ref, dx_tol, "chain dx N %d" % N)
    check_bound(dT, dT_ref, dT_tol, "chain dT N %d" % N)
    for _ in range(19):
        dx2, dT2 = run()
        assert torch.equal(dx2, dx) and torch.equal(dT2, dT)


# ---------------------------------------------------------------------------------------------------------------------
# fc_kernel<16 / 32, S>, fc_kernel<16, 4, 4> + fc_ksplit_reduce_kernel
# ---------------------------------------------------------------------------------------------------------------------
def run_fc(X, W, bias, Z, M, Nout, K, relu, tile=0, kscratch=False, batch=0, ld=None, strides=(0, 0, 0)):
    _lib, lib, s = lib_stream()
    ldX, ldW, ldY = ld if ld else (K, K, Nout)
    Y = torch.full((max(batch, 1), M, Nout), float("nan"), device="cuda")
    sc = None
    if kscratch:
        sc = torch.full((((Nout + 15) // 16) * ((M + 15) // 16) * 4096,), float("nan"), device="cuda")
    _lib.check(lib.geoa3_debug_fc_ex(P(X), ldX, strides[0], P(W), ldW, strides[1], P(bias), P(Z), Nout, P(Y), ldY, strides[2],
                                     M, Nout, K, batch, relu, tile << 8, P(sc), s), "geoa3_debug_fc_ex")
    return Y if batch else Y[0]


@pytest.mark.parametrize("Nout,K", C.FC_SHAPES)
def test_fc_shapes_of_both_directions_against_float64(Nout, K):
    """Every (Nout, K) of the network's heads, forward (bias + relu) and backward (Z gate) form, M in {1, 5, 17, 33}: both
    tiles and the shipped choice give the same bits; K = 4096 through kscratch (fc_kernel<16,4,4> + the reduce kernel) gives
    the bits of one workgroup per tile; geoa3_debug_fc (the entry tools/bench_fc.py times) gives them too."""
    _lib, lib, s = lib_stream()
    worst = 0.0
    for M in C.FC_M:
        for mode in ("z", "br"):
            c = C.fc_case(M, Nout, K, mode)
            ref, mag = C.fc_reference(c)
            tol = R.tolerance(ref, mag, K + 1)
            X, W = c["X"].cuda(), c["W"].cuda()
            bias = None if c["bias"] is None else c["bias"].cuda()
            Z = None if c["Z"] is None else c["Z"].cuda()
            relu = int(mode == "br")
            y16 = run_fc(X, W, bias, Z, M, Nout, K, relu, tile=16)
            worst = max(worst, check_bound(y16, ref, tol, "fc M %d Nout %d K %d %s" % (M, Nout, K, mode)))
            assert torch.equal(y16, run_fc(X, W, bias, Z, M, Nout, K, relu, tile=32)), (M, mode)
            assert torch.equal(y16, run_fc(X, W, bias, Z, M, Nout, K, relu, tile=0)), (M, mode)
            if K >= 2048:
                assert torch.equal(y16, run_fc(X, W, bias, Z, M, Nout, K, relu, tile=16, kscratch=True)), (M, mode)
                assert torch.equal(y16, run_fc(X, W, bias, Z, M, Nout, K, relu, tile=0, kscratch=True)), (M, mode)
            if mode == "br":
                Y = torch.full((M, Nout), float("nan"), device="cuda")
                _lib.check(lib.geoa3_debug_fc(P(X), P(W), P(bias), P(Y), M, Nout, K, 1, 0, s), "geoa3_debug_fc")
                assert torch.equal(Y, y16), M


def test_fc_batched_and_gram_forms_against_float64():
    """The per-instance 64 x 64 x 64 products (W3eff = W3 T64^T: shared X, sWb = 4096; dT64 = P W3: per-instance X, shared W)
    and the K = N product h2 G^T the f32 mode computes with this kernel (rows of 77 floats: unaligned)."""
    gen = torch.Generator().manual_seed(11)
    Bn = C.B
    S, Pm = torch.randn(64, 64, generator=gen), torch.randn(Bn, 64, 64, generator=gen)
    for X, W, strides in ((S, Pm, (0, 4096, 4096)), (Pm, S, (4096, 0, 4096))):
        ref, mag = R.fc(X.double(), W.double())
        out = run_fc(X.cuda(), W.cuda(), None, None, 64, 64, 64, 0, batch=Bn, strides=strides)
        check_bound(out, ref.expand(Bn, 64, 64), R.tolerance(ref, mag, 64).expand(Bn, 64, 64), "fc batched 64^3 %s" % (strides,))
    for N in (77, 200):
        c = C.gram_case(N, "uniform")
        ref, mag = R.gram(c["A"].double(), c["G"].double())
        out = run_fc(c["A"].cuda(), c["G"].cuda(), None, None, 64, 64, N, 0, batch=Bn, ld=(N, N, 64),
                     strides=(64 * N, 64 * N, 4096))
        check_bound(out, ref, R.tolerance(ref, mag, N), "fc K = N Gram form N %d" % N)
