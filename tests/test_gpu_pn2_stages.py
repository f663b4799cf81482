"""The native PointNet++ SSG forward and backward in their real launch sequence, checked STAGE BY STAGE: the workspace is
read after the forward and again after the backward through geoa3_debug_pn2ssg_workspace_layout (some buffers serve twice:
include/geoa3_hip_debug.h), and every stage is held to its restatement (tests/_pn2_native_ref.py; the sampler and the ball
queries to the oracle) fed with the GPU's OWN inputs of that stage, so errors do not compound.

Exact: xyz, idx1 (the pipelined sampler, centroid by centroid), nx1, gidx1, idx2, nx2, gidx2, bad.
Bounded (the bounds of tests/test_gpu_pn2_kernels.py; plain fp32 sums without the split term): out1 / arg1 (level 1's
forward, three chained split layers: R.sa1_fwd), shift, rt, out2 / arg2 / m0 / m1, h1, h2, p3 / arg3, q1, q2, logits; after the
backward g256, g512, g1024, dh2, dh1, dout2, dr, g1, the final dnx2 (level 3's coordinate gradient minus the centres' share),
the final dnx1 (W_x^T dr + dnx2 scattered by idx2 + gnx1) and dx (gxyz + dnx1 scattered by idx1, planar).
Level 1's BACKWARD recomputes its gates in the kernel: gnx1 and the level's own gxyz are held to R.sa1_bwd + its allowance for
the gates inside their bands (tests/test_gpu_pn2_sa1_bwd.py), computed from the GPU's own out1, arg1 and g1; where the
single-stream form accumulates the scatter of dnx1 into gxyz in place, the sum is held."""
import ctypes

import pytest
import torch

from tests import _pn2_native_cases as C
from tests import _pn2_native_ref as R

pytestmark = pytest.mark.gpu


def snapshot(net, B, N):
    """{name: uint8 CPU copy of the buffer up to the next one} of the module's workspace"""
    from geoa3_amd import _lib
    lib = _lib.load()
    names = (ctypes.c_char_p * 64)()
    offs = (ctypes.c_int64 * 64)()
    n = lib.geoa3_debug_pn2ssg_workspace_layout(B, N, names, offs, 64)
    assert 0 < n <= 64
    torch.cuda.synchronize()
    ws = net._ws_cache["ws"].cpu()
    assert offs[n - 1] <= ws.numel()
    return {names[i].decode(): ws[offs[i]:offs[i + 1]] for i in range(n - 1)}


def f32(buf, *shape):
    n = 1
    for s in shape:
        n *= s
    return buf[:4 * n].view(torch.float32).reshape(*shape).clone()


def i32(buf, *shape):
    n = 1
    for s in shape:
        n *= s
    return buf[:4 * n].view(torch.int32).reshape(*shape).clone()


def bound(got, ref, tol, what):
    ratio = R.worst_ratio(got, ref, tol)
    print("worst err/tol %-40s %.4f" % (what, ratio))
    assert ratio <= 1.0, "%s: worst err / tol = %g" % (what, ratio)


@pytest.mark.parametrize("B,N,side", [(3, 1024, "1"), (3, 1024, "0"), (3, 700, "1"), (2, 100, "1")])
def test_native_ssg_stage_by_stage(B, N, side, monkeypatch):
    from geoa3_amd import pointnet2 as pn2
    from oracle import geoa3_oracle as O
    from oracle import pointnet2_oracle as P2
    monkeypatch.setenv("GEOA3_PN2_SIDE", side)
    net = pn2.PointNet2ClassificationSSG(use_xyz=True, use_normal=False)
    net.load_state_dict(P2.make_pn2_state_dict(0))
    net = net.cuda().eval()
    for p in net.parameters():
        p.requires_grad_(False)
    pc, _ = O.make_synthetic_clouds(B, N, seed=70 + N)
    x = pc.cuda().requires_grad_()
    logits = net(x)
    packed = net.packed(x.device)
    assert (packed.struct.side is not None) == (side == "1")
    contract = bool(packed.struct.flags & 1)
    F_ = snapshot(net, B, N)
    w = torch.randn(B, 40, generator=torch.Generator().manual_seed(N)).cuda()
    (logits * w).sum().backward()
    K = snapshot(net, B, N)
    dx = x.grad.cpu()
    tag = "B %d N %d side %s" % (B, N, side)
    (w0, b0), (w1, b1), (w2, b2) = [(a.cpu(), b.cpu()) for a, b in pn2._fold_triples(net.SA_modules[1].mlps[0])]
    Wx, Wf = w0[:, :3].contiguous(), w0[:, 3:].contiguous()
    Wx3 = pn2._fold_triples(net.SA_modules[2].mlps[0])[0][0].cpu()[:, :3].contiguous()

    # ---- exact stages: layout, the pipelined sampler, gathers, ball queries
    xyz = f32(F_["xyz"], B, N, 3)
    assert torch.equal(xyz, R.planar_to_points(pc)), tag
    idx1 = i32(F_["idx1"], B, 512)
    assert torch.equal(idx1, P2.furthest_point_sampling(xyz, 512, contract)), tag
    nx1 = f32(F_["nx1"], B, 512, 3)
    assert torch.equal(nx1, R.gather_rows3(xyz, idx1)), tag
    gidx1 = i32(F_["gidx1"], B, 512, 64)
    assert torch.equal(gidx1, P2.ball_query(nx1, xyz, 0.2, 64, contract)), tag
    idx2 = i32(F_["idx2"], B, 128)
    assert torch.equal(idx2, P2.furthest_point_sampling(nx1, 128, contract)), tag
    nx2 = f32(F_["nx2"], B, 128, 3)
    assert torch.equal(nx2, R.gather_rows3(nx1, idx2)), tag
    gidx2 = i32(F_["gidx2"], B, 128, 64)
    assert torch.equal(gidx2, P2.ball_query(nx2, nx1, 0.4, 64, contract)), tag
    assert not i32(F_["bad"], B).any()
    for name in ("xyz", "idx1", "nx1", "gidx1", "idx2", "nx2", "gidx2", "out2", "arg2", "m0", "m1", "shift"):
        assert torch.equal(F_[name], K[name]), (tag, name)            # the backward leaves the forward's tables alone

    # ---- level 1's forward (with the side queue: four launches of 128 centroids each): out1 under the three-layer bound, arg1
    # a live sample whose y3 is maximal within 2 tol
    L1 = [(a.cpu().double(), b.cpu().double()) for a, b in pn2._fold_triples(net.SA_modules[0].mlps[0])]
    out1_, arg1 = f32(F_["out1"], B, 512, 128), F_["arg1"][:B * 512 * 128].reshape(B, 512, 128).long()
    worst = 0.0
    for b in range(B):
        r1 = R.sa1_fwd(xyz[b], nx1[b], gidx1[b], L1)
        worst = max(worst, R.worst_ratio(out1_[b], r1["out"], r1["tol_out"]))
        live1 = C._live_counts(gidx1[b])
        assert int(arg1[b].min()) >= 0 and bool((arg1[b] < live1.view(512, 1)).all()), "arg1 names a padded sample"
        at = torch.gather(r1["y3"], 1, arg1[b].unsqueeze(1)).squeeze(1)
        assert bool((at >= r1["y3"].max(1).values - 2 * r1["tol_out"]).all()), "arg1 is not a maximal sample"
    print("worst err/tol %-40s %.4f" % ("out1 " + tag, worst))
    assert worst <= 1.0, "out1: worst err / tol = %g" % worst
    assert torch.equal(F_["out1"], K["out1"]) and torch.equal(F_["arg1"], K["arg1"]), tag

    # ---- level 2's forward
    shift = f32(F_["shift"], B, 128, 128)
    ref, mag = R.affine3(Wx.double(), b0.double(), nx2.double(), -1.0)
    bound(shift, ref, R.tolerance(ref, mag, 4), "shift " + tag)
    out1 = f32(F_["out1"], B * 512, 128)
    rt = f32(F_["df1"], B, 512, 128)                                  # the forward keeps rT in the backward's df1
    ref, mag = R.sa2_pre(out1.double(), nx1.reshape(-1, 3).double(), Wf.double(), Wx.double())
    bound(rt.reshape(-1, 128), ref, R.tolerance(ref, mag, C.PRE_TERMS, extra=R.SPLIT), "rt " + tag)
    live = torch.stack([C._live_counts(gidx2[b]) for b in range(B)])
    c = dict(B=B, M=128, N1=512, live=live, tie=torch.full((B,), -1, dtype=torch.long))
    r = R.sa2_fwd(rt, gidx2, shift, w1, b1, w2, b2)
    r["tol_z1"], r["tol_y2"], r["tol_out"] = R.sa2_fwd_tolerances(r, w2)
    out2, arg2 = f32(F_["out2"], B, 256, 128), i32(F_["arg2"], B, 256, 128)
    m0, m1 = i32(F_["m0"], B * 128, 64, 4), i32(F_["m1"], B * 128, 64, 4)
    res = C.fwd_checks(c, r, out2, arg2, m0, m1)
    print("worst err/tol %-40s %.4f (band %.2e)" % ("out2 " + tag, res["out"], res["band"]))

    # ---- level 3 and the head, forward: h1 = relu(W_f out2 + W_x nx2 + b0), h2, the pooled layer, three FC layers
    (v0, c0), (v1, c1), (v2, c2) = [(a.cpu(), b.cpu()) for a, b in pn2._fold_triples(net.SA_modules[2].mlps[0])]
    Wf3 = v0[:, 3:].contiguous()
    fcl = net.fc_layer
    (f1, fb1), (f2, fb2), (f3, fb3) = [tuple(t.cpu() for t in pn2._fold_linear_bn(lin, bn))
                                       for lin, bn in ((fcl[0], fcl[1]), (fcl[3], fcl[4]), (fcl[7], None))]
    D = lambda t: t.double()
    h1 = f32(F_["h1"], B, 256, 128)
    ref, mag = R.conv(D(Wf3), D(out2), D(c0), relu=True, xyz=D(nx2), Wx=D(Wx3))
    bound(h1, ref, R.tolerance(ref, mag, 256 + 3 + 1, extra=R.SPLIT), "h1 " + tag)
    h2 = f32(F_["h2"], B, 512, 128)
    ref, mag = R.conv(D(v1), D(h1), D(c1), relu=True)
    bound(h2, ref, R.tolerance(ref, mag, 256 + 1, extra=R.SPLIT), "h2 " + tag)
    p3, arg3 = f32(F_["p3"], B, 1024), i32(F_["arg3"], B, 1024)
    ref, _, y3, mag = R.conv_pool(D(v2), D(h2), D(c2))
    tol3 = R.tolerance(y3, mag, 512 + 1, extra=R.SPLIT).max(-1).values          # relu and max are 1-Lipschitz
    bound(p3, ref, tol3, "p3 " + tag)
    assert int(arg3.min()) >= 0 and int(arg3.max()) < 128
    at = torch.gather(y3, 2, arg3.long().unsqueeze(-1)).squeeze(-1)
    assert bool((at >= y3.max(-1).values - 2 * tol3).all()), "arg3 is not a maximal point"
    q1, q2 = f32(F_["q1"], B, 512), f32(F_["q2"], B, 256)
    ref, mag = R.fc(D(p3), D(f1), D(fb1), relu=True)
    bound(q1, ref, R.tolerance(ref, mag, 1024 + 1), "q1 " + tag)
    ref, mag = R.fc(D(q1), D(f2), D(fb2), relu=True)
    bound(q2, ref, R.tolerance(ref, mag, 512 + 1), "q2 " + tag)
    ref, mag = R.fc(D(q2), D(f3), D(fb3))
    bound(logits.detach().cpu(), ref, R.tolerance(ref, mag, 256 + 1), "logits " + tag)

    # ---- the head and level 3, backward (d logits = w)
    g256, g512, g1024 = f32(K["g256"], B, 256), f32(K["g512"], B, 512), f32(K["g1024"], B, 1024)
    ref, mag = R.fc(D(w.cpu()), D(f3).t(), Zgate=q2 > 0)
    bound(g256, ref, R.tolerance(ref, mag, 40), "g256 " + tag)
    ref, mag = R.fc(D(g256), D(f2).t(), Zgate=q1 > 0)
    bound(g512, ref, R.tolerance(ref, mag, 256), "g512 " + tag)
    ref, mag = R.fc(D(g512), D(f1).t(), Zgate=p3 > 0)
    bound(g1024, ref, R.tolerance(ref, mag, 512), "g1024 " + tag)
    dh2 = f32(K["dh2"], B, 512, 128)
    terms = max(1, R.column_terms(g1024, arg3, 128, 1))
    for k0 in range(0, 512, 128):        # the sparse walk of the pooled layer, in four 128-row slices of h2
        ref, mag = R.wide_bwd(D(g1024), arg3, D(v2[:, k0:k0 + 128]), h2[:, k0:k0 + 128] > 0, 1)
        bound(dh2[:, k0:k0 + 128], ref, R.tolerance(ref, mag, terms), "dh2[%d:] %s" % (k0, tag))
    dh1_ = f32(K["dh1"], B, 256, 128)
    ref, mag = R.conv(D(v1).t(), D(dh2), gate=h1 > 0)
    bound(dh1_, ref, R.tolerance(ref, mag, 512, extra=R.SPLIT), "dh1 " + tag)
    ref, mag = R.conv(D(Wf3).t(), D(dh1_))
    bound(f32(K["dout2"], B, 256, 128), ref, R.tolerance(ref, mag, 256, extra=R.SPLIT), "dout2 " + tag)

    # ---- level 2's backward, from the GPU's own dout2 / gates / tables
    dout2, dh1 = f32(K["dout2"], B, 256, 128), f32(K["dh1"], B, 256, 128)
    dnx2_in, mag_in = R.affine3_grad(dh1.double(), Wx3.double())
    gate0 = R.unpack_gate_words(m0.reshape(B, 128, 64, 4))
    gate1 = R.unpack_gate_words(m1.reshape(B, 128, 64, 4))
    rb = R.sa2_bwd(dout2.double(), out2.double(), arg2, gidx2, gate0, gate1, w1.double(), w2.double(), Wx.double(), dnx2_in)
    tb = R.sa2_bwd_tolerances(rb)
    dr = f32(K["r"], B, 512, 128)                                     # the backward writes dr over r
    bound(dr, rb["dr"][0], tb["dr"], "dr " + tag)
    dnx2 = f32(K["dnx2"], B, 128, 3)
    bound(dnx2, rb["dnx2"][0], tb["dnx2"] + R.tolerance(dnx2_in, mag_in, 256), "dnx2 " + tag)
    g1 = f32(K["g1"], B * 512, 128)
    ref, mag = R.sa2_pre(dr.reshape(-1, 128).double(), None, Wf.t().contiguous().double(), None)
    bound(g1, ref, R.tolerance(ref, mag, 128, extra=R.SPLIT), "g1 " + tag)
    # the final dnx1 = W_x^T dr + dnx2 scattered by idx2 + level 1's share gnx1
    gnx1 = f32(K["gnx1"], B, 512, 3)
    base, bmag = dr.double() @ Wx.double(), dr.double().abs() @ Wx.double().abs()
    sc, smag, most = R.scatter_rows3(dnx2.double(), idx2, 512, into=base)
    dnx1 = f32(K["dnx1"], B, 512, 3)
    bound(dnx1, sc + gnx1.double(), R.tolerance(sc + gnx1.double(), smag - base.abs() + bmag + gnx1.double().abs(), 128 + most + 1),
          "dnx1 " + tag)
    # ---- level 1's backward, from the GPU's own out1 / arg1 / g1: gnx1 = dnew, gxyz = dxyz (+ the scatter of dnx1 by idx1 where
    # that went into gxyz in place), under bound + allowance
    gxyz = f32(K["gxyz"], B, N, 3)
    sc, smag, most = R.scatter_rows3(dnx1.double(), idx1, N)
    worst = {"gnx1": 0.0, "gxyz": 0.0}
    for b in range(B):
        rb1 = R.sa1_bwd(xyz[b], nx1[b], gidx1[b], L1, out1_[b], arg1[b], g1.reshape(B, 512, 128)[b])
        ref, _, tol, allow = rb1["dnew"]
        worst["gnx1"] = max(worst["gnx1"], R.worst_ratio(gnx1[b], ref, tol + allow))
        ref, mag, tol, allow = rb1["dxyz"]
        if side != "1":
            tol = tol + R.tolerance(ref + sc[b], mag + smag[b], most + 1)
            ref = ref + sc[b]
        worst["gxyz"] = max(worst["gxyz"], R.worst_ratio(gxyz[b], ref, tol + allow))
    for name, ratio in worst.items():
        print("worst err/tol %-40s %.4f" % (name + " " + tag, ratio))
        assert ratio <= 1.0, "%s: worst err / tol = %g" % (name, ratio)
    # dx = planar(gxyz + dnx1 scattered by idx1)
    if side == "1":      # the scatter went into a buffer of its own (the forward's f1), added on the way out
        gx2 = f32(K["f1"], B, N, 3)
        bound(gx2, sc, R.tolerance(sc, smag, most), "gx2 " + tag)
        ref, mag = gxyz.double() + gx2.double(), gxyz.double().abs() + gx2.double().abs()
        bound(R.planar_to_points(dx), ref, R.tolerance(ref, mag, 2), "dx " + tag)
    else:
        # One stream: the scatter of dnx1 by idx1 accumulated into gxyz IN PLACE, so level 1's own gxyz no longer exists and
        # the workspace holds only the sum.  This assertion therefore checks points_to_planar_kernel alone, NOT dx: the
        # accumulating scatter_rows3_kernel is checked above through idx2 (accumulate = 1) and, with the side queue, through
        # idx1 (accumulate = 0); dx itself is held to the side-queue run bit for bit by
        # test_native_ssg_side_queue_same_bits_and_module_copies.
        assert torch.equal(R.planar_to_points(dx), gxyz), tag
