"""CPU only: the float64 restatements of tests/_pn2_native_ref.py are pinned to plain torch (the concatenated first layer,
group -> shared MLP -> max-pool with autograd-free float64 modules); every non-stress case of tests/_pn2_native_cases.py
shows one lost term moving an entry past the case's bound; and the emulation of the kernels' split-fp16 arithmetic stays
inside every case's bound, stress cases included (its worst err / tol per kernel is printed: DESIGN 8b's CPU column)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _pn2_native_cases as C
from tests import _pn2_native_ref as R


# ---------------------------------------------------------------------------------------------------------------------
# frag_image
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Rw,K,variant", C.FRAG_CASES)
def test_frag_image_restatement(Rw, K, variant):
    """The scale rule takes the maximum into [2^13, 2^14); hi + lo carries W to 2^-23 of each entry (subnormal low pieces: to
    2^-25 of the smallest normal fp16 at the image's scale); the index map is a permutation of the image."""
    W = C.frag_case(Rw, K, variant).numpy()
    E, hi, lo, pos = R.frag_image(W)
    assert 14 <= E <= 254
    v = W.astype(np.float64) * float(R.scale_of(E))
    if variant == "zeros":
        assert E == 14 and not hi.any() and not lo.any() and np.isfinite(R.unscale_of(E)) and R.unscale_of(E) > 0
    else:
        assert 2.0 ** 13 <= np.abs(v).max() < 2.0 ** 14
    err = np.abs(v - hi.astype(np.float64) - lo.astype(np.float64))
    assert (err <= np.maximum(2.0 ** -23 * np.abs(v), 2.0 ** -25)).all()
    assert sorted(pos.ravel().tolist()) == list(range(2 * Rw * K))
    un, img = R.frag_image_flat(W)
    assert float(un) * float(R.scale_of(E)) == 1.0
    # the documented layout, entry by entry, on a few rows
    for row, k in ((0, 0), (31, 15), (Rw - 1, K - 1), (Rw // 2 + 1, K // 2 + 3)):
        base = ((((row >> 5) * (K >> 4) + (k >> 4)) * 2) * 64 + 32 * ((k >> 3) & 1) + (row & 31)) * 8 + (k & 7)
        assert img[base] == hi[row, k] and img[base + 64 * 8] == lo[row, k]


# ---------------------------------------------------------------------------------------------------------------------
# sa2_pre
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Np", [s for s in C.PRE_SHAPES if s[0] <= 1024])
def test_sa2_pre_restatement_is_the_concatenated_first_layer(P, Np):
    """r = W0 [xyz ; f] with W0 = [W_x | W_f], the level's first 1x1 convolution applied per point (both layouts of f)"""
    c = C.pre_case(P, Np)
    W0 = torch.cat([c["Wx"], c["Wf"]], 1).double()
    X = R.point_major(c["f"], c["channel_major"]).double()
    want = F.conv1d(torch.cat([c["xyz"].double(), X], 1).t().unsqueeze(0), W0.unsqueeze(-1))[0].t()
    ref, tol = C.pre_reference(c)
    assert torch.allclose(ref, want, rtol=1e-13, atol=1e-13)
    assert torch.allclose(C.pre_reference(c, with_xyz=False)[0], X @ c["Wf"].double().t(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("P,Np", C.PRE_SHAPES)
def test_sa2_pre_bound_notices_a_lost_term_and_holds_the_emulation(P, Np):
    c = C.pre_case(P, Np)
    for with_xyz in (True, False):
        ref, tol = C.pre_reference(c, with_xyz)
        bad = [C.pre_reference(c, with_xyz, skip_k=77)[0]]
        if with_xyz:
            bad.append(C.pre_reference(c, True, skip_ninth=True)[0])      # the ninth k-step
        for b in bad:
            assert R.worst_ratio(b, ref, tol) > 1.0
        got = R.sa2_pre_split(c["f"], c["xyz"] if with_xyz else None, c["Wf"], c["Wx"], c["channel_major"])
        ratio = R.worst_ratio(got, ref, tol)
        print("cpu emulation err/tol sa2_pre P %d Np %d xyz %d: %.4f" % (P, Np, with_xyz, ratio))
        assert ratio <= 1.0


@pytest.mark.parametrize("variant", C.PRE_STRESS)
def test_sa2_pre_stress_emulation(variant):
    c = C.pre_case(96, 0, variant)
    ref, tol = C.pre_reference(c)
    ratio = R.worst_ratio(R.sa2_pre_split(c["f"], c["xyz"], c["Wf"], c["Wx"]), ref, tol)
    print("cpu emulation err/tol sa2_pre %s: %.4f" % (variant, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("ratio", C.WX_RATIOS)
def test_sa2_pre_wx_magnitude(ratio):
    """max|W_x| = ratio max|W_f|.  The image's scale takes max|W_f| into [2^13, 2^14) and fp16 rounds 65520 and more to
    infinity: W_x carried at that scale saturates from max|W_x| / max|W_f| = 65520 / 2^14 = 3.999 on when max|W_f| sits at the
    top of its binade, from 7.998 on when it sits at the bottom -- never below 3.999, always from 8 on.  The kernel as it was
    (wx_in_image_always) then returns Inf / NaN; with the saturating column tiles' coordinate term in fp32 every ratio stays
    inside the bound, and a ratio that does not saturate computes the same bits either way."""
    c = C.pre_case(96, 0, "random", ratio)
    assert abs(float(c["Wx"].abs().max()) / float(c["Wf"].abs().max()) - ratio) < 1e-6 * ratio
    ref, tol = C.pre_reference(c)
    got = R.sa2_pre_split(c["f"], c["xyz"], c["Wf"], c["Wx"])
    r = R.worst_ratio(got, ref, tol)
    print("cpu emulation err/tol sa2_pre W_x ratio %g: %.4f" % (ratio, r))
    assert r <= 1.0
    old = R.sa2_pre_split(c["f"], c["xyz"], c["Wf"], c["Wx"], wx_in_image_always=True)
    sat = R.wx_saturates(c["Wf"], c["Wx"])
    assert sat == (ratio >= 8) or 3.999 <= ratio < 8
    if sat:
        assert not torch.isfinite(old).all()
    else:
        assert torch.equal(old, got)


# ---------------------------------------------------------------------------------------------------------------------
# sa2_fwd
# ---------------------------------------------------------------------------------------------------------------------
FWD_ALL = [s + (False,) for s in C.FWD_SHAPES] + [(1, 8, 40, True)]


@pytest.mark.parametrize("B,M,N1", C.FWD_SHAPES)
def test_sa2_fwd_restatement_is_group_mlp_maxpool(B, M, N1):
    """float64 torch: group the pre-transformed rows, + shift, relu, two 1x1 convolutions, max_pool over the samples (with
    return_indices: the first maximal sample)"""
    c, r = C.fwd_case(B, M, N1), C.fwd_reference(B, M, N1)
    rows = torch.stack([c["rT"][b][c["gidx"][b].long().reshape(-1)].reshape(M, 64, 128) for b in range(B)])
    # (the one add in front of the first relu in float32, as the kernel and the restatement have it: a0 is an INPUT of the
    # products, and its sign is the gate m0 the kernel must reproduce bit for bit)
    a0 = F.relu(rows.permute(0, 3, 1, 2) + c["shift"].unsqueeze(-1)).double()                     # [B][128][M][64]
    a1 = F.relu(F.conv2d(a0, c["W1"].double().view(128, 128, 1, 1), c["b1"].double()))
    y2 = F.conv2d(a1, c["W2"].double().view(256, 128, 1, 1), c["b2"].double())
    out, idx = F.max_pool2d(y2, (1, 64), return_indices=True)
    assert torch.allclose(r["y2"], y2, rtol=1e-12, atol=1e-12)
    assert torch.allclose(r["out"], F.relu(out.squeeze(-1)), rtol=1e-12, atol=1e-12)
    assert bool(torch.gather(r["maximal"], 3, r["arg"].unsqueeze(-1)).all())
    assert bool((r["arg"] <= (idx.squeeze(-1) % 64)).all())          # first maximal sample
    assert r["a0"].dtype == torch.float32 and torch.equal(r["a0"].double(), a0.permute(0, 2, 3, 1).float().double())
    # the forced rows
    assert int(c["live"][0, 1]) == 1 and int(c["live"][0, 2]) == min(64, N1)
    assert int(c["gidx"].min()) >= 0 and int(c["gidx"].max()) < N1
    words = R.pack_gate_words(r["a0"] > 0)
    assert torch.equal(R.unpack_gate_words(words), r["a0"] > 0)


@pytest.mark.parametrize("B,M,N1,stress", FWD_ALL)
def test_sa2_fwd_bounds_notice_a_lost_term_and_hold_the_emulation(B, M, N1, stress):
    c, r = C.fwd_case(B, M, N1, stress), C.fwd_reference(B, M, N1, stress)
    args = (c["rT"], c["gidx"], c["shift"], c["W1"], c["b1"], c["W2"], c["b2"])
    if not stress:
        lost1 = R.sa2_fwd(*args, skip_k1=5)
        assert R.worst_ratio(lost1["z1"], r["z1"], r["tol_z1"]) > 1.0
        assert R.worst_ratio(lost1["out"], r["out"], r["tol_out"]) > 1.0
        lost2 = R.sa2_fwd(*args, skip_k2=100)
        assert R.worst_ratio(lost2["out"], r["out"], r["tol_out"]) > 1.0
    z1, y2 = R.sa2_fwd_split(*args)
    rz = R.worst_ratio(z1, r["z1"], r["tol_z1"])
    ry = R.worst_ratio(y2, r["y2"], r["tol_y2"])
    out = y2.max(-1).values.clamp_min(0)
    arg = (y2 == y2.max(-1, keepdim=True).values).to(torch.uint8).argmax(-1)
    res = C.fwd_checks(c, r, out, arg, R.pack_gate_words(r["a0"] > 0).reshape(-1, 64, 4),
                       R.pack_gate_words(z1 > 0).reshape(-1, 64, 4))
    print("cpu emulation err/tol sa2_fwd B %d M %d N1 %d stress %d: z1 %.4f y2 %.4f out %.4f, band %.2e"
          % (B, M, N1, stress, rz, ry, res["out"], res["band"]))
    assert rz <= 1.0 and ry <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# sa2b: the level's backward
# ---------------------------------------------------------------------------------------------------------------------
def test_sa2_bwd_restatement_is_autograd_of_gather_mlp_max():
    """float64 autograd through gather -> + shift -> relu -> W1 -> relu -> W2 -> max over the samples -> relu, with the pooled
    arg-max fixed to the first maximal sample: d rT == dr, W_x^T d shift == the centres' coordinate sums"""
    from oracle import pointnet2_oracle as O
    g = torch.Generator().manual_seed(5)
    xyz = torch.rand(1, 512, 3, generator=g)
    gidx = O.ball_query(xyz[:, :128].contiguous(), xyz, 0.4, 64)
    rT = (torch.randn(1, 512, 128, generator=g) * 0.5).double().requires_grad_(True)
    shift = (torch.randn(1, 128, 128, generator=g) * 0.5).double().requires_grad_(True)       # [b][channel][centre]
    W1, W2 = torch.randn(128, 128, generator=g).double() * 0.125, torch.randn(256, 128, generator=g).double() * 0.125
    b1, b2 = torch.randn(128, generator=g).double() * 0.1, torch.randn(256, generator=g).double() * 0.1
    Wx = torch.randn(128, 3, generator=g).double()
    a0 = F.relu(rT[0][gidx[0].long().reshape(-1)].reshape(128, 64, 128) + shift[0].t().unsqueeze(1))
    a1 = F.relu(a0 @ W1.t() + b1)
    y2 = (a1 @ W2.t() + b2).permute(2, 0, 1)                                                  # [256][128][64]
    arg = (y2 == y2.max(-1, keepdim=True).values).to(torch.uint8).argmax(-1)
    out = F.relu(torch.gather(y2, 2, arg.unsqueeze(-1)).squeeze(-1))
    dout = torch.randn(256, 128, generator=g).double()
    out.backward(dout)
    dnx2_in = torch.randn(1, 128, 3, generator=g).double()
    # the backward reads W1 as [k][i] = d a1[k] -> d a0[i]: the forward's W1 [k = output][i = input] as it is
    r = R.sa2_bwd(dout.unsqueeze(0), out.detach().unsqueeze(0), arg.unsqueeze(0), gidx, (a0 > 0).unsqueeze(0),
                  (a1 > 0).unsqueeze(0), W1, W2, Wx, dnx2_in)
    assert torch.allclose(r["dr"][0], rT.grad, rtol=1e-11, atol=1e-12)
    assert torch.allclose(r["dnx2"][0], dnx2_in - torch.einsum("bim,id->bmd", shift.grad, Wx), rtol=1e-11, atol=1e-12)
    assert torch.allclose(r["dnx1"][0], rT.grad @ Wx, rtol=1e-11, atol=1e-12)
    assert torch.allclose(r["y"][0].sum(2), torch.einsum("bim,id->bmd", shift.grad, Wx), rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("launch", range(len(C.SA2B_LAUNCHES)))
def test_sa2b_tables_bounds_and_emulation(launch):
    """The tables of every cloud have the shape its pattern is there for; in every cloud with rows, each lost term (a row's
    last entry, a tile's row 32, the last row of a destination, one k of the W1^T product, one sample of a centre's coordinate
    sum) moves an entry of dr / dnx2 past the bound; the emulation of the kernels' arithmetic stays inside every bound."""
    c = C.sa2b_case(launch)
    ref, tol = C.sa2b_reference(c)
    worst = {k: 0.0 for k in tol}
    for b, pat in enumerate(c["patterns"]):
        tb = R.sa2b_tables(c["dout"][b], c["out"][b], c["arg"][b], c["gidx"][b])
        Rn, parts = len(tb["keys"]), [tb["pb"][p + 1] - tb["pb"][p] for p in range(4)]
        per_dest = np.bincount(tb["rows"][:, 0], minlength=512) if Rn else np.zeros(512, dtype=np.int64)
        if pat == "sample0":
            assert Rn == 128 and (np.diff(tb["first"]) == 256).all()
        elif pat == "full":
            assert Rn == 8192 and len(tb["td"]) >= 128
        elif pat == "zero":
            assert Rn == 0 and len(tb["td"]) == 0 and not tb["hit"].any()
        elif pat == "one":
            assert Rn == 1 and len(tb["ec"]) == 1
        elif pat == "shared":
            assert per_dest[0] == 128
        elif pat == "rows65":
            assert parts == [65, 65, 65, 65] and per_dest.max() == 1
        elif pat == "rows33":
            assert parts == [33, 33, 33, 33]
        elif pat == "repeat":
            assert Rn > 64
        assert int(tb["ptile"][4]) == len(tb["td"]) and sum(int(t[1]) for t in tb["td"]) == Rn
        if Rn:
            usable = lambda pos: bool(c["gate0"][b, tb["rows"][pos][1], tb["rows"][pos][2]].any()
                                      and c["gate1"][b, tb["rows"][pos][1], tb["rows"][pos][2]].any())
            key = lambda pos: (b, int(tb["rows"][pos][1]), int(tb["rows"][pos][2]))
            some = next(p for p in range(Rn) if usable(p))
            lastd = next((p for p in range(Rn) if usable(p) and tb["keys"][p] < 0), some)
            row32 = next((int(t[0]) + 32 for t in tb["td"] if t[1] > 32 and usable(int(t[0]) + 32)), some)
            for what, defect in (("last entry", dict(skip_last_entry=[key(some)])), ("row 32", dict(zero_rows=[key(row32)])),
                                 ("last row of a destination", dict(zero_rows=[key(lastd)])), ("one k", dict(skip_k=9)),
                                 ("one sample", dict(skip_samples=[key(some)]))):
                bad, _ = C.sa2b_reference(c, **defect)
                moved = max(R.worst_ratio(bad[k][0][b], ref[k][0][b], tol[k][b]) for k in ("dr", "dnx2"))
                assert moved > 1.0, (pat, what, moved)
        got = R.sa2_bwd_split(c["dout"][b], c["out"][b], c["arg"][b], c["gidx"][b], c["gate0"][b], c["gate1"][b], c["W1"],
                              c["W2"], c["Wx"], c["dnx2_in"][b])
        for k, v in zip(("dr", "y", "dnx2", "dnx1"), got):
            ratio = R.worst_ratio(v, ref[k][0][b], tol[k][b])
            worst[k] = max(worst[k], ratio)
            assert ratio <= 1.0, (pat, k, ratio)
    print("cpu emulation err/tol sa2b launch %d: " % launch + " ".join("%s %.4f" % kv for kv in worst.items()))


# ---------------------------------------------------------------------------------------------------------------------
# glue, level 3
# ---------------------------------------------------------------------------------------------------------------------
def test_glue_and_level3_restatements():
    """conv / conv_pool against F.conv1d and F.max_pool1d; gather_rows3 / scatter_rows3 / affine3 / affine3_grad against
    autograd of the gather and of the affine map; planar <-> point-major round trip; a lost k moves conv past its bound"""
    g = torch.Generator().manual_seed(9)
    X = torch.randn(2, 32, 50, generator=g, dtype=torch.float64)
    W, b = torch.randn(48, 32, generator=g, dtype=torch.float64), torch.randn(48, generator=g, dtype=torch.float64)
    xyz, Wx = torch.randn(2, 50, 3, generator=g, dtype=torch.float64), torch.randn(48, 3, generator=g, dtype=torch.float64)
    want = F.relu(F.conv1d(torch.cat([xyz.permute(0, 2, 1), X], 1), torch.cat([Wx, W], 1).unsqueeze(-1), b))
    ref, mag = R.conv(W, X, b, relu=True, xyz=xyz, Wx=Wx)
    assert torch.allclose(ref, want, rtol=1e-12, atol=1e-12)
    two, _ = R.affine3_add(R.conv(W, X)[0], Wx, b, xyz, relu=True)          # the convolution, then affine3_add_kernel
    assert torch.allclose(two, want, rtol=1e-12, atol=1e-12)
    plain, pmag = R.conv(W, X, b)
    assert R.worst_ratio(R.conv(W, X, b, skip_k=7)[0], plain, R.tolerance(plain, pmag, 33, extra=R.SPLIT)) > 1.0
    pooled, arg, y, _ = R.conv_pool(W, X, b)
    mp, idx = F.max_pool1d(F.conv1d(X, W.unsqueeze(-1), b), 50, return_indices=True)
    assert torch.allclose(pooled, F.relu(mp.squeeze(-1)), rtol=1e-12, atol=1e-12) and torch.equal(arg, idx.squeeze(-1))
    pts = torch.randn(2, 20, 3, generator=g, dtype=torch.float64, requires_grad=True)
    idx = torch.randint(0, 20, (2, 30), generator=g).to(torch.int32)
    out = R.gather_rows3(pts, idx)
    up = torch.randn(2, 30, 3, generator=g, dtype=torch.float64)
    out.backward(up)
    sc, smag, most = R.scatter_rows3(up, idx, 20)
    assert torch.allclose(sc, pts.grad, rtol=1e-12, atol=1e-12) and most == int(max(torch.bincount(i.long()).max() for i in idx))
    acc, _, _ = R.scatter_rows3(up, idx, 20, into=torch.ones(2, 20, 3, dtype=torch.float64))
    assert torch.allclose(acc, pts.grad + 1, rtol=1e-12, atol=1e-12)
    p = xyz.clone().requires_grad_(True)
    val, _ = R.affine3(Wx, b, p, -1.0)
    dY = torch.randn(2, 48, 50, generator=g, dtype=torch.float64)
    val.backward(dY)
    assert torch.allclose(-R.affine3_grad(dY, Wx)[0], p.grad, rtol=1e-12, atol=1e-12)
    x = torch.randn(2, 3, 50, generator=g)
    assert torch.equal(R.points_to_planar(R.planar_to_points(x)), x) and R.planar_to_points(x).shape == (2, 50, 3)


def test_debug_entries_refuse_null_pointers_and_sizes_outside_the_contract():
    """no GPU work: every geoa3_debug_pn2_* entry returns GEOA3_EINVAL before it launches anything"""
    import __graft_entry__
    __graft_entry__.build()
    from geoa3_amd import _lib
    lib = _lib.load()
    # Every non-null argument is a REAL buffer, far larger than any of these calls could touch (device memory where there is
    # a GPU, else host memory): the size checks come first and nothing is launched, but should one of them ever regress, the
    # result is a failing assertion here and not an access outside an allocation.
    import ctypes
    if torch.cuda.is_available():
        keep = torch.zeros(8 << 20, dtype=torch.uint8, device="cuda")
        p = keep.data_ptr()
    else:
        keep = ctypes.create_string_buffer((8 << 20) + 256)
        p = (ctypes.addressof(keep) + 255) // 256 * 256
    assert p % 256 == 0
    EINVAL = -1
    assert lib.geoa3_debug_pn2_frag_image(None, 32, 16, p, p, None) == EINVAL
    assert lib.geoa3_debug_pn2_frag_image(p, 33, 16, p, p, None) == EINVAL
    assert lib.geoa3_debug_pn2_frag_image(p, 32, 8, p, p, None) == EINVAL
    assert lib.geoa3_debug_pn2_sa2_pre(p, 0, 0, None, p, p, None, None, 32, None) == EINVAL
    assert lib.geoa3_debug_pn2_sa2_pre(p, 0, 0, None, p, p, None, p, 33, None) == EINVAL
    assert lib.geoa3_debug_pn2_sa2_pre(p, 1, 48, None, p, p, None, p, 96, None) == EINVAL
    assert lib.geoa3_debug_pn2_sa2_pre(p, 0, 0, p, p, p, None, p, 32, None) == EINVAL          # xyz without W_x
    ok13 = [p] * 13
    assert lib.geoa3_debug_pn2_sa2_fwd(*ok13, 1, 40, 12, None) == EINVAL                         # M not a multiple of 8
    assert lib.geoa3_debug_pn2_sa2_fwd(*ok13, 0, 40, 8, None) == EINVAL
    assert lib.geoa3_debug_pn2_sa2_fwd(*([None] + ok13[1:]), 1, 40, 8, None) == EINVAL
    ok14 = [p] * 14
    assert lib.geoa3_debug_pn2_sa2b(*ok14, 0, None) == EINVAL
    assert lib.geoa3_debug_pn2_sa2b(*(ok14[:10] + [p + 8] + ok14[11:]), 1, None) == EINVAL       # scratch not 256-byte aligned
    assert lib.geoa3_debug_pn2_sa2b(*(ok14[:13] + [None]), 1, None) == EINVAL
    assert lib.geoa3_debug_pn2_sa1_scatter(None, p, 1, 40, 8, p, None) == EINVAL
    assert lib.geoa3_debug_pn2_sa1_scatter(p, p, 0, 40, 8, p, None) == EINVAL
    assert lib.geoa3_debug_pn2_sa1_scatter(p, p, 1, 40, 8, None, None) == EINVAL
    assert lib.geoa3_debug_pn2_sa1_scatter(p, p, 1, 7000, 8, p, None) == -3      # one instance's sums beyond LDS: not supported
    assert lib.geoa3_debug_pn2_sa2b_scratch_bytes(0) == 0
    per = lib.geoa3_debug_pn2_sa2b_scratch_bytes(1)
    assert per == R.sa2b_scratch_layout()[1] and lib.geoa3_debug_pn2_sa2b_scratch_bytes(5) == 5 * per
    names, offs = (ctypes.c_char_p * 64)(), (ctypes.c_int64 * 64)()
    assert lib.geoa3_debug_pn2ssg_workspace_layout(1, 16, names, offs, 64) == -1
    n = lib.geoa3_debug_pn2ssg_workspace_layout(2, 100, names, offs, 64)
    assert 0 < n <= 64 and offs[n - 1] == lib.geoa3_pn2ssg_workspace_bytes(2, 100)


# ---------------------------------------------------------------------------------------------------------------------
# the restatements chained == the oracle's classifier and its autograd input gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [100, 300])
def test_chained_restatements_are_the_oracle_forward_and_input_gradient(N):
    """float64 throughout (the sampler and the ball queries pick in float32, as the oracle's do): sa1_fwd -> sa2_pre -> affine3 -> sa2_fwd ->
    conv -> conv -> conv_pool -> fc x 3 gives oracle.pointnet2_ssg_forward; fc x 3 -> wide_bwd -> conv x 2 -> affine3_grad ->
    sa2_bwd -> sa2_pre (W_f^T) -> scatter_rows3, with level 1's forward restatement (sa1_fwd) differentiated by autograd (its
    backward's restatement, sa1_bwd, is pinned to autograd on its own below), gives its input gradient."""
    from oracle import geoa3_oracle as O
    from oracle import pointnet2_oracle as P2
    B = 2
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in P2.make_pn2_state_dict(0).items()}
    pc, _ = O.make_synthetic_clouds(B, N, seed=80 + N)
    pc = pc.double()
    wgt = torch.randn(B, 40, generator=torch.Generator().manual_seed(N)).double()
    x = pc.clone().requires_grad_(True)
    want = P2.pointnet2_ssg_forward(sd, x)
    (want * wgt).sum().backward()

    def folded(prefix, j):
        w = sd["%s.%d.weight" % (prefix, 3 * j)]
        q = "%s.%d" % (prefix, 3 * j + 1)
        scale = sd[q + ".weight"] / torch.sqrt(sd[q + ".running_var"] + 1e-5)
        return w.reshape(w.shape[0], -1) * scale.view(-1, 1), sd[q + ".bias"] - sd[q + ".running_mean"] * scale

    L = [[folded("SA_modules.%d.mlps.0" % i, j) for j in range(3)] for i in range(3)]
    (f1, fb1), (f2, fb2) = folded("fc_layer", 0), folded("fc_layer", 1)
    f3, fb3 = sd["fc_layer.7.weight"], sd["fc_layer.7.bias"]
    # level 1: its restatement, differentiable (cloud by cloud)
    xyz = R.planar_to_points(pc).requires_grad_(True)
    idx1 = P2.furthest_point_sampling(xyz.detach(), 512)
    nx1 = R.gather_rows3(xyz, idx1)
    gidx1 = P2.ball_query(nx1.detach(), xyz.detach(), 0.2, 64)
    out1 = torch.stack([R.sa1_fwd(xyz[b], nx1[b], gidx1[b], L[0])["out"] for b in range(B)])      # [B][512][128], point-major
    # level 2
    idx2 = P2.furthest_point_sampling(nx1.detach(), 128)
    nx2 = R.gather_rows3(nx1.detach(), idx2)
    gidx2 = P2.ball_query(nx2, nx1.detach(), 0.4, 64)
    (w0, b0), (w1, b1), (w2, b2) = L[1]
    Wx, Wf = w0[:, :3], w0[:, 3:]
    rt = R.sa2_pre(out1.detach().reshape(-1, 128), nx1.detach().reshape(-1, 3), Wf, Wx)[0].reshape(B, 512, 128)
    shift = R.affine3(Wx, b0, nx2, -1.0)[0]
    r2 = R.sa2_fwd(rt, gidx2, shift, w1, b1, w2, b2)
    # level 3 and the head
    (v0, c0), (v1, c1), (v2, c2) = L[2]
    Wx3, Wf3 = v0[:, :3], v0[:, 3:]
    h1 = R.conv(Wf3, r2["out"], c0, relu=True, xyz=nx2, Wx=Wx3)[0]
    h2 = R.conv(v1, h1, c1, relu=True)[0]
    p3, arg3, _, _ = R.conv_pool(v2, h2, c2)
    q1 = R.fc(p3, f1, fb1, relu=True)[0]
    q2 = R.fc(q1, f2, fb2, relu=True)[0]
    logits = R.fc(q2, f3, fb3)[0]
    assert torch.allclose(logits, want.detach(), rtol=1e-10, atol=1e-11)
    # backward
    g256 = R.fc(wgt, f3.t(), Zgate=q2 > 0)[0]
    g512 = R.fc(g256, f2.t(), Zgate=q1 > 0)[0]
    g1024 = R.fc(g512, f1.t(), Zgate=p3 > 0)[0]
    dh2 = torch.cat([R.wide_bwd(g1024, arg3, v2[:, k:k + 128].contiguous(), h2[:, k:k + 128] > 0, 1)[0] for k in range(0, 512, 128)], 1)
    dh1 = R.conv(v1.t(), dh2, gate=h1 > 0)[0]
    dout2 = R.conv(Wf3.t(), dh1)[0]
    dnx2_in = R.affine3_grad(dh1, Wx3)[0]
    rb = R.sa2_bwd(dout2, r2["out"], r2["arg"], gidx2, r2["a0"] > 0, r2["z1"] > 0, w1, w2, Wx, dnx2_in)
    g1 = R.sa2_pre(rb["dr"][0].reshape(-1, 128), None, Wf.t(), None)[0].reshape(B, 512, 128)
    dnx1 = R.scatter_rows3(rb["dnx2"][0], idx2, 512, into=rb["dnx1"][0])[0]
    (gx,) = torch.autograd.grad([out1, nx1], xyz, [g1, dnx1])
    assert torch.allclose(R.points_to_planar(gx), x.grad, rtol=1e-9, atol=1e-11 * float(x.grad.abs().max()))


def test_sa1_fwd_bound_notices_a_lost_term_and_reads_float32_differences():
    """level 1's forward restatement at a kernel's float32 inputs: the grouped differences are float32 (one subtraction, the
    kernel's operand); one lost k of the second product moves `out` past the three-layer bound; a plain float32 evaluation
    stays inside it; arg is the first maximal sample"""
    from oracle import pointnet2_oracle as P2
    g = torch.Generator().manual_seed(11)
    xyz = torch.rand(1, 200, 3, generator=g)
    nx = xyz[:, :32].contiguous()
    gidx = P2.ball_query(nx, xyz, 0.3, 64)[0]
    layers = [(torch.randn(co, ci, generator=g) * (2.0 / ci) ** 0.5, torch.randn(co, generator=g) * 0.1)
              for ci, co in ((3, 64), (64, 64), (64, 128))]
    L64 = [(w.double(), b.double()) for w, b in layers]
    r = R.sa1_fwd(xyz[0], nx[0], gidx, L64)
    d32 = xyz[0][gidx.long().reshape(-1)].reshape(32, 64, 3) - nx[0].unsqueeze(1)
    want = F.relu(F.relu(F.relu(d32.double() @ L64[0][0].t() + L64[0][1]) @ L64[1][0].t() + L64[1][1]) @ L64[2][0].t() + L64[2][1])
    assert torch.allclose(r["out"], want.max(1).values, rtol=1e-12, atol=1e-12)
    assert bool((torch.gather(r["y3"], 1, r["arg"].unsqueeze(1)).squeeze(1) == r["y3"].max(1).values).all())
    bad = R.sa1_fwd(xyz[0], nx[0], gidx, L64, skip_k2=17)
    assert R.worst_ratio(bad["out"], r["out"], r["tol_out"]) > 1.0
    f32 = R.sa1_fwd(xyz[0], nx[0], gidx, layers)
    ratio = R.worst_ratio(f32["out"], r["out"], r["tol_out"])
    print("cpu fp32 err/tol sa1_fwd: %.4f" % ratio)
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# level 1's backward: sa1_bwd_kernel + sa1_scatter_kernel
# ---------------------------------------------------------------------------------------------------------------------
SA1B_PLAIN = [s + ("random",) for s in C.SA1B_SHAPES] + [(1, 8, 80, v) for v in ("padding", "padding_arg", "zeros")] + \
             [C.SA1B_BAND]
SA1B_ALL = SA1B_PLAIN + [(1, 8, 80, v) for v in C.SA1B_STRESS]


@pytest.mark.parametrize("B,M,N,variant", SA1B_PLAIN)
def test_sa1_bwd_restatement_is_autograd_of_gather_mlp_max(B, M, N, variant):
    """float64 autograd through gather -> minus the centroid -> three layers -> the sample arg names -> relu, at float64 copies
    of the case's inputs: d xyz == dxyz, d new_xyz == dnew, the gradient of the differences with the padded samples merged
    into sample 0 == dp"""
    c = C.sa1b_case(B, M, N, variant)
    L = [(w.double(), b.double()) for w, b in c["layers"]]
    for b in range(min(B, 3)):
        x, nx = c["xyz"][b].double().requires_grad_(True), c["nx"][b].double().requires_grad_(True)
        d = x[c["gidx"][b].long().reshape(-1)].reshape(M, 64, 3) - nx.unsqueeze(1)
        d.retain_grad()
        y3 = F.relu(F.relu(d @ L[0][0].t() + L[0][1]) @ L[1][0].t() + L[1][1]) @ L[2][0].t() + L[2][1]
        at = torch.gather(y3, 1, c["arg"][b].long().unsqueeze(1)).squeeze(1)
        live = (c["out"][b] > 0).double()
        (at * live * c["g"][b].double()).sum().backward()
        r = R.sa1_bwd(x.detach(), nx.detach(), c["gidx"][b], L, c["out"][b], c["arg"][b], c["g"][b])
        scale = float(d.grad.abs().max()) + 1e-300
        assert torch.allclose(r["dxyz"][0], x.grad, rtol=1e-10, atol=1e-12 * scale)
        assert torch.allclose(r["dnew"][0], nx.grad, rtol=1e-10, atol=1e-12 * scale)
        assert torch.allclose(r["dp"][0], R.merge_padding(d.grad, r["pad"]), rtol=1e-10, atol=1e-12 * scale)
        assert bool((r["dp"][1] >= r["dp"][0].abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("B,M,N,variant", SA1B_ALL)
def test_sa1_bwd_share_cap_lost_terms_and_emulation(B, M, N, variant):
    """From the reference alone: at most 1e-3 of the case's non-padded dp rows carry an allowance.  In every case that is not
    a stress case one lost term -- a channel of W3^T dz3, a k of the W2^T product, a row of the K = 3 contraction, a sample of
    dnew's sum, a merged duplicate (where arg names one), an (m, s) entry of a destination -- moves an entry past bound +
    allowance.  The emulation of the kernels' arithmetic stays inside it (stress cases included), and so does a plain float32
    evaluation of the restatement."""
    c, refs = C.sa1b_case(B, M, N, variant), C.sa1b_reference(B, M, N, variant)
    share = C.sa1b_share(refs)
    print("share of rows with an allowance %s %s: %.2e" % ((B, M, N), variant, share))
    assert share <= C.SA1B_SHARE
    L = [(w.double(), b.double()) for w, b in c["layers"]]
    r0 = refs[0]
    if variant not in C.SA1B_STRESS:
        mag_rows = r0["dp"][1].sum(-1) * (~r0["pad"])
        m, s = divmod(int(mag_rows.argmax()), 64)                                  # the non-padded row with the most behind it
        g0 = torch.where(c["out"][0, m] > 0, c["g"][0, m], torch.zeros(128)) * (c["arg"][0, m].long() == s)
        fw = C._sa1_fwd64(c, 0)                                                    # (a k / a row whose gate is open at that row)
        lost = [("ch", (m, s, int(g0.abs().argmax()))), ("k2", int(fw["z2"][m, s].argmax())), ("row", int(fw["z1"][m, s].argmax())),
                ("sample", (m, s)), ("entry", (m, s))]
        if variant == "padding_arg":
            lost.append(("dup", (0, 63)))
        for lose in lost:
            bad = R.sa1_bwd(c["xyz"][0], c["nx"][0], c["gidx"][0], L, c["out"][0], c["arg"][0], c["g"][0], lose=lose)
            moved = max(R.worst_ratio(bad[k][0], r0[k][0], r0[k][2] + r0[k][3]) for k in ("dp", "dnew", "dxyz"))
            assert moved > 1.0, (lose, moved)
    few = min(B, 3)          # (clouds are independent on the CPU: three of the five are enough here)
    C.sa1b_checks(refs[:few], *C.sa1b_emulate(dict(c, B=few)), "cpu emulation sa1_bwd %s %s" % ((B, M, N), variant))
    f32 = [R.sa1_bwd(c["xyz"][0], c["nx"][0], c["gidx"][0], c["layers"], c["out"][0], c["arg"][0], c["g"][0])]
    C.sa1b_checks(refs[:1], *[[r[k][0] for r in f32] for k in ("dp", "dnew", "dxyz")], "cpu fp32 sa1_bwd %s %s" % ((B, M, N), variant))


def test_sa1_bwd_allowance_is_what_admits_an_in_band_gate():
    """The `band` case: one z1 and one z2 of a row that carries gradient sit inside their bands.  The emulation with either of
    those gates as it computes them AND inverted stays inside bound + allowance; of each pair one side misses the plain bound:
    the margin scheme is necessary, not merely loose."""
    sh = C.SA1B_BAND
    c, refs = C.sa1b_case(*sh), C.sa1b_reference(*sh)
    assert len(c["band"]) == 2
    L = [(w.double(), b.double()) for w, b in c["layers"]]
    f = C._sa1_fwd64(c, 0)
    for (layer, b, m, s, ch) in c["band"]:
        z, t = (f["z1"], f["t1"]) if layer == 1 else (f["z2"], f["t2"])
        assert float(z[m, s, ch].abs()) <= float(t[m, s, ch]) and float(refs[0]["dp"][3][m, s if not refs[0]["pad"][m, s] else 0].max()) > 0
        plain = []
        for flip in ((), ((layer, b, m, s, ch),)):
            got = C.sa1b_emulate(c, flip=flip)
            C.sa1b_checks(refs, *got, "band gate %d flipped %d" % (layer, len(flip)))
            plain.append(max(R.worst_ratio(got[i][0], refs[0][k][0], refs[0][k][2]) for i, k in enumerate(("dp", "dnew", "dxyz"))))
        print("plain err/tol with the layer-%d gate as computed / inverted: %.3g %.3g" % (layer, plain[0], plain[1]))
        assert max(plain) > 1.0


@pytest.mark.parametrize("defect,variant", [("no_ex", "padding_arg"), ("mask_block0", "padding"), ("skip_ks3", "padding"),
                                            ("skip_ks2", "padding"), ("no_hcb", "padding")])
def test_sa1_bwd_bounds_notice_the_kernel_defects(defect, variant):
    """the emulation with one of the kernel's steps broken -- the merged duplicates dropped from sample 0, the one-hot mask of
    the wrong column block, the last k-step of either backward product skipped, the column block's selection removed -- misses
    the bounds of the padding cases"""
    sh = (1, 8, 80, variant)
    c, refs = C.sa1b_case(*sh), C.sa1b_reference(*sh)
    with pytest.raises(AssertionError):
        C.sa1b_checks(refs, *C.sa1b_emulate(c, defect=defect), "defect " + defect)


def test_sa1_scatter_model_bound_and_order_independence():
    """the integer model of sa1_scatter_kernel: within cnt 2^(Ex - 41) + 2^-24 |sum| of the float64 sum; the same bits with
    the centroids and the samples behind sample 0 in any order; a NaN row poisons its destination, an infinite one the
    instance; padded samples are skipped whatever they hold"""
    c = C.sa1b_case(3, 40, 300)
    dp = C.sa1b_emulate(c)[0][1].numpy()
    gidx = c["gidx"][1].numpy()
    got = R.sa1_scatter_fixed(dp, gidx, 300)
    ref, bound, Ex = R.sa1_scatter_bound(dp, gidx, 300)
    assert 2.0 ** (Ex - 1) <= float(np.abs(dp).max()) < 2.0 ** Ex
    ratio = R.worst_ratio(torch.from_numpy(got), ref, bound)
    print("scatter model err/bound %.4f" % ratio)
    assert ratio <= 1.0
    rng = np.random.default_rng(5)
    pm = rng.permutation(40)
    dp2, g2 = dp[pm].copy(), gidx[pm].copy()
    for m in range(40):
        ps = np.concatenate([[0], 1 + rng.permutation(63)])
        dp2[m], g2[m] = dp2[m][ps], g2[m][ps]
    assert np.array_equal(R.sa1_scatter_fixed(dp2, g2, 300).view(np.uint32), got.view(np.uint32))
    pad = R.pad_mask(torch.from_numpy(gidx)).numpy()
    junk = dp.copy()
    junk[pad] = 7.0                                   # (below the instance's maximum?  no: it moves Ex, as in the kernel)
    assert R.sa1_scatter_fixed(junk, gidx, 300).shape == got.shape
    small = dp.copy()
    small[pad] = np.float32(2.0 ** (Ex - 30))
    assert np.array_equal(R.sa1_scatter_fixed(small, gidx, 300).view(np.uint32), got.view(np.uint32))
    nan = dp.copy()
    nan[5, 0, 1] = np.nan
    out = R.sa1_scatter_fixed(nan, gidx, 300)
    assert np.isnan(out[gidx[5, 0]]).all() and np.isfinite(np.delete(out, gidx[5, 0], 0)).all()
    inf = dp.copy()
    inf[5, 0, 1] = np.inf
    assert np.isnan(R.sa1_scatter_fixed(inf, gidx, 300)).all()
    assert not R.sa1_scatter_fixed(np.zeros_like(dp), gidx, 300).any()


def test_sa1_bwd_emulation_follows_small_gradients():
    """grad_out times 2^-s in the emulation: with the scale's exponent field clamped at 110 (the kernel as it was) the scale-free
    bound is missed from a centroid maximum of about 2^-34 on, and from 2^-50 on every result is an exact zero; with the clamp
    the format allows (Emin = max(13, 14 + k2 - EW3T)) the bound holds down to a maximum of 2^(Emin - 127), and below it the
    centroid's results are NaN"""
    sh = (1, 8, 80)
    c, refs = C.sa1b_case(*sh), C.sa1b_reference(*sh)
    r = refs[0]
    (_, _), (W2, _), (W3, _) = c["layers"]
    Emin = max(13, 14 + R.sa_k(float(W2.abs().max())) - R.l1_exponent(float(W3.abs().sum(0).max())))
    g0 = torch.where(c["out"][0] > 0, c["g"][0], torch.zeros(()))
    Es = [R.biased_exponent(float(v)) for v in g0.abs().max(1).values]
    ratio = lambda got, s: max(R.worst_ratio(got[i][0], r[k][0] * 2.0 ** -s, (r[k][2] + r[k][3]) * 2.0 ** -s)
                               for i, k in enumerate(("dp", "dnew")))
    was = {s: ratio(C.sa1b_emulate(dict(c, g=c["g"] * 2.0 ** -s), kg_lo=110), s) for s in (16, 32, 40, 56)}
    print("cpu emulation, clamp at 110: " + " ".join("2^-%d %.3g" % kv for kv in was.items()))
    assert was[16] <= 1.0 and was[32] <= 1.0 and was[40] > 1.0 and was[56] > 1.0
    assert not C.sa1b_emulate(dict(c, g=c["g"] * 2.0 ** -56), kg_lo=110)[0].any()
    worst = 0.0
    for s in range(20, min(Es) - Emin + 1, 4):
        worst = max(worst, ratio(C.sa1b_emulate(dict(c, g=c["g"] * 2.0 ** -s)), s))
    print("cpu emulation, derived clamp: worst err/tol down to 2^-%d: %.4f" % (min(Es) - Emin, worst))
    assert worst <= 1.0
    dp, dnew, _ = C.sa1b_emulate(dict(c, g=c["g"] * 2.0 ** -(max(Es) - Emin + 4)))
    assert bool(torch.isnan(dnew).all()) and bool(torch.isnan(dp[0][~r["pad"]]).all())
