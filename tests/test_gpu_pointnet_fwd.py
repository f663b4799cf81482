"""The trunk kernels geoa3_pointnet_forward launches, ALONE (geoa3_debug_conv_chain / geoa3_debug_conv_cm_ex of
include/geoa3_hip_debug.h), against the float64 restatement tests/_pointnet_fwd_ref.py on the hand-made inputs of
tests/_pointnet_fwd_cases.py: the three chain kernels, the forward forms of the single-layer kernels in both arithmetic modes,
chain against layer by layer bit for bit, the large-launch forms, and the real forward stage by stage.

Bound: |got - ref| <= 4 sqrt(n) 2^-24 mag + 2^-22 |ref| per layer, carried through |W| along a chain (the restatement's
docstring).  A gate bit must be the float64 gate wherever |pre| exceeds the entry's bound (at most 0.5 % of a case's bits are
left open: tests/test_pointnet_fwd_ref.py asserts that on the CPU), and the bits of a stored activation must be Y > 0 exactly.
Bits of columns >= N are not compared.  Every output and mask buffer lies between two sentinel-filled guard regions and is
prefilled: nothing outside [B][Co][N] floats / [B][ceil(N/64)][Co] words may change, nothing inside may stay unwritten.
Every test prints its worst err / bound."""
import ctypes

import pytest
import torch

from tests import _pointnet_fwd_cases as C
from tests import _pointnet_fwd_ref as R

pytestmark = pytest.mark.gpu

GUARD = 1024                      # elements in front of and behind every output
F_FILL = 0x7FC5A5A5               # a NaN: a finite result must have replaced every one inside
W_FILL = 0x5A5A5A5A5A5A5A5A


def lib_stream():
    from geoa3_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


class Guarded:
    """an output buffer of n floats / 64-bit words between two guard regions, everything prefilled"""

    def __init__(self, n, words=False):
        self.n, self.words = n, words
        self.buf = torch.full((n + 2 * GUARD,), W_FILL if words else F_FILL, dtype=torch.int64 if words else torch.int32,
                              device="cuda")
        self.inner = self.buf[GUARD:GUARD + n]
        self.fill = W_FILL if words else F_FILL

    def ptr(self):
        return self.inner.data_ptr()

    def take(self, *shape):
        """the written contents; asserts the guards are untouched and nothing inside was left as prefilled"""
        assert bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.n:] == self.fill).all()), \
            "a write outside the buffer"
        assert not bool((self.inner == self.fill).any()), "an element inside the buffer was not written"
        out = self.inner if self.words else self.inner.view(torch.float32)
        return out.view(*shape).clone()


def dev(c):
    d = {k: (c[k].cuda() if c.get(k) is not None else None) for k in ("X", "x3", "T3", "w1", "b1")}
    d["stages"] = [(W.cuda(), b.cuda()) for (W, b) in c["stages"]]
    return d


def run_chain(c, d):
    """one launch of the chain kernel of the case's kind -> ([Y or None per stage], [bits per stage])"""
    _lib, lib, s = lib_stream()
    Bn, N, ns = c["B"], c["N"], len(c["stages"])
    stored = C.STORED[c["kind"]]
    cos = [W.shape[-2] for (W, _) in c["stages"]]
    Ys = [Guarded(Bn * co * N) if st else None for co, st in zip(cos, stored)]
    Ms = [Guarded(Bn * ((N + 63) // 64) * co, words=True) for co in cos]
    arr = lambda vals: (ctypes.c_void_p * ns)(*vals)
    strides = (ctypes.c_int64 * ns)(*[4096 if W.dim() == 3 else 0 for (W, _) in c["stages"]])
    _lib.check(lib.geoa3_debug_conv_chain(P(d["X"]), P(d["x3"]), P(d["T3"]), P(d["w1"]), P(d["b1"]), ns,
                                          arr([P(W) for (W, _) in d["stages"]]), strides,
                                          arr([P(b) for (_, b) in d["stages"]]), arr([y.ptr() if y else None for y in Ys]),
                                          arr([m.ptr() for m in Ms]), Bn, N, s), "geoa3_debug_conv_chain")
    torch.cuda.synchronize()
    Y = [y.take(Bn, co, N) if y else None for y, co in zip(Ys, cos)]
    bits = [R.unpack_gate_bits(m.take(Bn, (N + 63) // 64, co), N) for m, co in zip(Ms, cos)]
    return Y, bits


def run_layer(d_in, cloud, W, bias, Bn, N, split):
    """one launch of the single-layer kernel: d_in = X on the device, or None with cloud = (x3, T3, w1, b1)"""
    _lib, lib, s = lib_stream()
    co = W.shape[-2]
    Y, M = Guarded(Bn * co * N), Guarded(Bn * ((N + 63) // 64) * co, words=True)
    x3, T3, w1, b1 = cloud if d_in is None else (None, None, None, None)
    _lib.check(lib.geoa3_debug_conv_cm_ex(P(d_in), P(x3), P(T3), P(w1), P(b1), 64, co, P(W), 4096 if W.dim() == 3 else 0,
                                          P(bias), 1, Y.ptr(), M.ptr(), split, Bn, N, s), "geoa3_debug_conv_cm_ex")
    torch.cuda.synchronize()
    return Y.take(Bn, co, N), R.unpack_gate_bits(M.take(Bn, (N + 63) // 64, co), N)


def run_layers(c, d, split):
    """the launches a chain replaces: every stage one kernel, its activation written and read back by the next"""
    Y, bits, h = [], [], d["X"]
    for (W, bias) in d["stages"]:
        y, m = run_layer(h, (d["x3"], d["T3"], d["w1"], d["b1"]), W, bias, c["B"], c["N"], split)
        Y.append(y)
        bits.append(m)
        h = y
    return Y, bits


def check_stage(what, Y, bits, L, cap=C.OPEN_CAP):
    """values (when stored) and gate bits of one stage against its float64 layer L; -> worst err / bound.  cap: the share of
    open gate bits the case promises (None: inputs that promise none -- the share is printed)"""
    ratio = 0.0
    if Y is not None:
        Yc = Y.cpu()
        ratio = R.worst_ratio(Yc, L["y"], L["bound"])
        assert torch.equal(bits, Yc > 0), "%s: a gate bit is not Y > 0" % what
    wrong, open_share = R.gate_ratio(bits, L)
    print("worst err/bound %-44s %.4f   open gate bits %.2e" % (what, ratio, open_share))
    assert ratio <= 1.0, "%s: worst err / bound = %g" % (what, ratio)
    assert wrong == 0, "%s: %d gate bits differ from the float64 gate outside the bound" % (what, wrong)
    assert cap is None or open_share <= cap, what
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# conv_chain_kernel<1,true,128>, <3,true,128>, <2,false,128>
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", C.CHAIN_N)
@pytest.mark.parametrize("kind", C.KINDS)
def test_chain_kernel_against_float64(kind, N):
    """Each chain kernel alone: values of every stored stage, gate bits of every stage (the unstored c1 / h3 included).  Input
    rows ascending (the running scale shrinks at a later chunk and rescales its sums), descending, 1e-30 then 1e+10 (the
    sums are flushed); an all-zero instance, one scaled by 1e-12; per-instance weights 1e-3 / 1e3 / 1 apart (x2); a
    per-instance T3 and none, w1 / b1 rows over five decades (cloud-fed)."""
    for v in C.variants(kind):
        c, (layers, _) = C.case_and_reference(kind, N, v)
        Y, bits = run_chain(c, dev(c))
        for i, L in enumerate(layers):
            check_stage("chain %s %s N %d %s" % (kind, C.STAGE_NAMES[kind][i], N, "/".join(map(str, v))), Y[i], bits[i], L)
        if "X" in c:
            assert not bool(Y[1][2, :, :].ne(Y[1][2, :, :1]).any())      # the all-zero instance: relu(W relu(b0) + b1) in every column


# ---------------------------------------------------------------------------------------------------------------------
# conv_cm64_kernel / conv_cm64s_kernel: the forward forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("N", C.CHAIN_N)
@pytest.mark.parametrize("kind", C.KINDS)
def test_single_layer_forward_forms_against_float64(kind, N, split):
    """The same cases one layer per launch, both arithmetic modes, the same bound (n is the same): produce_first with T3
    and without into 64 (c3) and 128 (c1) channels, per-instance weights at K = Co = 64 (x2), the plain 64 -> 64 and
    64 -> 128 layers behind them; the gate words of every form."""
    for v in C.variants(kind):
        c, (layers, _) = C.case_and_reference(kind, N, v)
        Y, bits = run_layers(c, dev(c), split)
        for i, L in enumerate(layers):
            check_stage("%s %s %s N %d %s" % ("f16x2" if split else "f32", kind, C.STAGE_NAMES[kind][i], N,
                                              "/".join(map(str, v))), Y[i], bits[i], L)


@pytest.mark.parametrize("N", C.CHAIN_N)
@pytest.mark.parametrize("kind", C.KINDS)
def test_chain_same_bits_as_the_launches_it_replaces(kind, N):
    """The whole-network claim (tests/test_gpu_pointnet.py) on the hand-made magnitudes: a chain's stored outputs and all
    its gate bits (columns < N) are those of the split single-layer launches, bit for bit."""
    for v in C.variants(kind):
        c, _ = C.case_and_reference(kind, N, v)
        d = dev(c)
        Yc, bc = run_chain(c, d)
        Yl, bl = run_layers(c, d, 1)
        for i in range(len(bc)):
            assert torch.equal(bc[i], bl[i]), (kind, N, v, i)
            if Yc[i] is not None:
                assert torch.equal(Yc[i], Yl[i]), (kind, N, v, i)


# ---------------------------------------------------------------------------------------------------------------------
# large launches
# ---------------------------------------------------------------------------------------------------------------------
GROUPS = [[0, 1, 2], [128, 129, 130], [254, 255, 256]]


def test_chain_with_two_column_blocks_per_workgroup():
    """conv_chain_kernel<3,true,128> at N = 513, B = 257: 3 x 257 column blocks > 768, so two workgroups per instance and one of
    them walks two blocks.  Instances [0:3], [128:131], [254:257] give the bits of three-instance launches (one block per
    workgroup), and those nine hold the float64 bound."""
    c, (layers, _) = C.large_chain_case()
    assert ((c["N"] + 255) // 256) * c["B"] > 768
    Y, bits = run_chain(c, dev(c))
    for g, rows in enumerate(GROUPS):
        small = C.select(c, rows)
        Ys, bs = run_chain(small, dev(small))
        sl = slice(3 * g, 3 * g + 3)
        for i, L in enumerate(layers):
            assert torch.equal(bits[i][rows], bs[i]), (rows, i)
            if Y[i] is not None:
                assert torch.equal(Y[i][rows], Ys[i]), (rows, i)
            Lg = {k: t[sl] for k, t in L.items()}
            check_stage("large chain %s instances %d.." % (C.STAGE_NAMES["c3"][i], rows[0]), Ys[i], bs[i], Lg)


@pytest.mark.parametrize("split", [0, 1])
def test_single_layer_on_more_than_512_workgroups(split):
    """K = 64, Co = 128, N = 256, B = 257: the split kernel's 514 workgroups take the instantiation without the deep prefetch
    and the tile remap's 32 full groups and one partial one; both modes against three-instance launches and float64."""
    c, (layers, _) = C.large_conv_case()
    d = dev(c)
    W, bias = d["stages"][0]
    Y, bits = run_layer(d["X"], None, W, bias, c["B"], c["N"], split)
    for g, rows in enumerate(GROUPS):
        Ys, bs = run_layer(d["X"][rows].contiguous(), None, W, bias, 3, c["N"], split)
        assert torch.equal(Y[rows], Ys) and torch.equal(bits[rows], bs), rows
        Lg = {k: t[3 * g:3 * g + 3] for k, t in layers[0].items()}
        check_stage("large layer %s instances %d.." % ("f16x2" if split else "f32", rows[0]), Ys, bs, Lg)


# ---------------------------------------------------------------------------------------------------------------------
# the real forward, stage by stage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_chain", [0, 2])
@pytest.mark.parametrize("mode", ["f16x2", "f32"])
@pytest.mark.parametrize("Bn,N", [(3, 77), (2, 300)])
def test_real_forward_stage_by_stage(Bn, N, mode, no_chain, monkeypatch):
    """geoa3_pointnet_forward on the module's weights: a2, T3, h2, c2, T64, W3eff, h4 (c1 and h3 too when they are written: layer
    by layer) and the six gate masks read out of the workspace by name, each held to the float64 restatement of its stage
    on the DEVICE's own input to that stage -- the forward hands every launch the right operand: T3 to the trunk but not to
    the input T-Net, each layer its own bias, W3eff with its instance stride."""
    from oracle import geoa3_oracle as O
    from geoa3_amd import pointnet as PN
    _lib, lib, _ = lib_stream()
    monkeypatch.setattr(PN, "AB_FLAGS", no_chain)
    sd = O.make_pointnet_state_dict(40, seed=0)
    net = PN.PointNet(40)
    net.load_state_dict(sd)
    net.wide_mode = mode
    net = net.cuda().eval()
    pc, _ = O.make_synthetic_clouds(Bn, N, seed=11 * Bn + N)
    with torch.no_grad():
        net(pc.cuda())
    torch.cuda.synchronize()
    ws = net._ws_cache["ws"]
    names, offs = (ctypes.c_char_p * 64)(), (ctypes.c_int64 * 64)()
    n = lib.geoa3_debug_pointnet_workspace_layout(Bn, N, 40, names, offs, 64)
    at = {names[i].decode(): offs[i] for i in range(n)}
    T = (N + 63) // 64

    def read(name, *shape):
        count = 1
        for s in shape:
            count *= s
        return ws[at[name]:at[name] + 4 * count].view(torch.float32).view(*shape).cpu().double()

    def bits(name, co):
        return R.unpack_gate_bits(ws[at["m_" + name]:at["m_" + name] + 8 * Bn * T * co].view(torch.int64).view(Bn, T, co), N)

    pk = PN.pack_pointnet(sd)
    w = lambda p, k: p[k].double()
    t3, t64 = pk["t3"], pk["t64"]
    chained = mode == "f16x2" and not no_chain
    tag = "%s %s (%d, %d) " % (mode, "chain" if chained else "layers", Bn, N)
    x = pc.double()

    def walk(h, bound, stages):
        """stages: (name, W, bias, co, written); each held to the restatement on the device's own input where there is one"""
        for name, W, bias, co, written in stages:
            L = R.stage(h, W, bias, bound)
            Yd = read(name, Bn, co, N) if written else None
            check_stage(tag + name, None if Yd is None else Yd.float(), bits(name, co), L, cap=None)
            h, bound = (Yd, None) if written else (L["y"], L["bound"])

    # input T-Net: the cloud itself, no transform
    f = R.first_layer(x, w(t3, "w1"), w(t3, "b1"))
    walk(f["y"], f["bound"], [("a2", w(t3, "w2"), w(t3, "b2"), 128, True)])
    # trunk front and the feature T-Net's first layers: the cloud through the device's T3
    T3 = read("T3", Bn, 3, 3)
    f = R.first_layer(x, w(pk, "w1"), w(pk, "b1"), T3)
    walk(f["y"], f["bound"], [("h2", w(pk, "w2"), w(pk, "b2"), 64, True),
                              ("c1", w(t64, "w1"), w(t64, "b1"), 64, not chained),
                              ("c2", w(t64, "w2"), w(t64, "b2"), 128, True)])
    # W3eff = W3 T64^T per instance (the batched FC kernel: 64 fp32 terms)
    T64 = read("T64", Bn, 64, 64)
    ref = torch.einsum("oj,bij->boi", w(pk, "w3"), T64)
    mag = torch.einsum("oj,bij->boi", w(pk, "w3").abs(), T64.abs())
    ratio = R.worst_ratio(read("W3eff", Bn, 64, 64), ref, R.tolerance(ref, mag, 64))
    print("worst err/bound %-44s %.4f" % (tag + "W3eff", ratio))
    assert ratio <= 1.0
    # conv3 with the device's W3eff on the device's h2, conv4
    walk(read("h2", Bn, 64, N), None, [("h3", read("W3eff", Bn, 64, 64), w(pk, "b3"), 64, not chained),
                                       ("h4", w(pk, "w4"), w(pk, "b4"), 128, True)])
