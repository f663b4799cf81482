"""Every entry point of csrc/geom_reg.hip alone, through geoa3_amd.ops with the table handed in (knn=) and the outputs
pre-filled with NaN, against the float64 restatement that takes the table as given (tests/_reg_table_ref.py).

Bounds (from the header of geom_reg.hip and the float32 format, not from what the kernels return):
  gradients, per element   n_i 2^(ex - 41) + 2^-24 |ref_i|: n_i pair terms, each rounded to the instance's fixed-point unit
                           2^(ex - 40), ex = ilogb of the instance's largest |term|, then one float32 rounding
                           (displacement_loss: the first part times 2 |adv_c - ori_c|, the sum being d theta)
  kNN_smoothing_loss       mask exact; loss within 2^-23 |ref| (s_i and the loss are float32, everything between double)
  repulsion_loss, per point (1/k) sum_m (2 u_m + c) 2^-24 |term_m| + 2^-24 |ref|, u = d^2 / h^2: d * d and the division
                           each move u by 2^-24 u.  c is in units of 2^-24 relative: an ulp of a float32 result is at
                           most 2 of them, so expf's measured EXPF_ULPS ulps are at most 2 * EXPF_ULPS units (1.71; the
                           largest relative error seen was 1.41), and c = 2 * EXPF_ULPS + 2 adds the two roundings
                           around it (the quotient's sign flip is exact; the product d * expf).  Nothing is doubled
                           beyond that change of units
  displacement_loss, per term 2 |t| D + D^2 + 2^-24 t^2, D = 4 * 2^-24 (theta_i + theta_j), and 2^-24 |ref| per point
EXPF_ULPS: no document of the ROCm installation states expf's error, so it was measured once on the MI355X: expf(-u) alone
against exp in double over every float u in [0, 87] (the range of u the cases keep to, asserted): at most 0.8567 ulp of the
float32 result (1.41 * 2^-24 relative), near u = 5.285.

Tables, ld = k + 3: column 0 holds index N + 5 and distance NaN, the columns beyond k hold -7 and NaN -- no kernel may read
either.  Distances are the float32 un-fused squared distance of the listed pair (geoa3_sqdist).
  search  the device's own geoa3_knn_self table, wider than k + 1 (finite, in range): the bits of the entry point's own search
  random  uniform indices; rows 0..9 hold one index twice and another three times in columns 1..5 (as many of the five as k
          allows), rows 10..19 the point itself in columns 1..k
  hub     every entry one index: it receives N k terms, every other point k
  oob     the random table with one entry N and one -1 in instance 1
Instance 1 is the cloud scaled by 2^-10 and instance 2 by 2^10: each has its own ex, and with h = 0.03 every repulsion term
of instance 2 underflows (largest term 0: gradient exactly +0.0).

Largest err / bound on the MI355X (printed per case; a float32 result half an ulp off a reference just above a power of
two reaches 1 by itself): gradients -- smoothing 0.997, repulsion 1.000, displacement 0.998, normal 0.995; forwards --
smoothing loss 0.426, repulsion 0.746, displacement 0.747; geoa3_reg_fold 0.950."""
import numpy as np
import pytest
import torch

from geoa3_amd import _lib
from tests import _reg_table_ref as TR

pytestmark = pytest.mark.gpu
EXPF_ULPS = 0.8567   # measured on the MI355X, see the module docstring
C_EXP = 2 * EXPF_ULPS + 2
U24 = 2.0 ** -24
H = 0.03
H2 = float(np.float32(H * H))          # what the kernels take: float32 of the double product
COEF = 0.3
LDS, WORKSPACE = 0, 1
SMOOTH, REPULSE, DISPLACE, NORMAL = range(4)
NAMES = ("smoothing", "repulsion", "displacement", "normal")
SCALES = (1.0, 2.0 ** -10, 2.0 ** 10)
RATIOS = {}


# ------------------------------------------------------------------------------------------------ inputs (host)
def clouds(B, N, seed):
    """x, ori, nrm [B,3,N] float32; instance b scaled by SCALES[b] (exact).  ori = x + a small displacement."""
    rng = np.random.default_rng(seed)
    x = (rng.random((B, 3, N)) * 0.3 - 0.15).astype(np.float32)
    ori = (x + 0.01 * rng.standard_normal((B, 3, N))).astype(np.float32)
    nrm = rng.standard_normal((B, 3, N))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    s = np.asarray(SCALES[:B], np.float32).reshape(B, 1, 1)
    return x * s, ori * s, nrm


def sqdist32(x, idx):
    """float32 un-fused squared distance (geoa3_sqdist) of every listed pair; indices outside the cloud give NaN"""
    B, _, N = x.shape
    inside = (idx >= 0) & (idx < N)
    j = np.where(inside, idx, 0)
    d = []
    for c in range(3):
        t = x[:, c, :, None] - np.take_along_axis(x[:, c, None, :], j.reshape(B, 1, -1), 2).reshape(idx.shape)
        d.append(t * t)
    out = (d[0] + d[1]) + d[2]
    assert out.dtype == np.float32
    return np.where(inside, out, np.float32("nan"))


def poison(idx, d, k):
    idx, d = idx.copy(), d.copy()
    idx[:, :, 0], d[:, :, 0] = idx.shape[1] + 5, np.nan
    idx[:, :, k + 1:], d[:, :, k + 1:] = -7, np.nan
    return idx.astype(np.int32), d.astype(np.float32)


def table(kind, x, k, seed):
    B, _, N = x.shape
    ld = k + 3
    rng = np.random.default_rng(seed)
    if kind == "hub":
        idx = np.full((B, N, ld), N // 3)
    else:
        idx = rng.integers(0, N, (B, N, ld))
        if N >= 20:
            a, b = rng.integers(0, N, (2, B, 10))
            pat = [a, a, b, b, b][:k]
            for m, v in enumerate(pat):
                idx[:, :10, 1 + m] = v
            idx[:, 10:20, 1:k + 1] = np.arange(10, 20)[None, :, None]
    idx, d = poison(idx, sqdist32(x, idx), k)
    return idx, d, smoothing_dists(x, k, ld, rng)


def smoothing_dists(x, k, ld, rng, coef=COEF):
    """kNN_smoothing_loss reads nothing but the table's distances, so they are free: random ones at the instance's scale,
    then every row whose s_i lies within 2e-4 thr of the threshold is moved 1 % away from it, until none does"""
    B, _, N = x.shape
    scale = np.abs(x).max((1, 2), keepdims=True).astype(np.float64) ** 2
    d = (scale * (0.05 + rng.random((B, N, ld)))).astype(np.float32)
    for _ in range(50):
        s = d[:, :, 1:k + 1].astype(np.float64).sum(2) / k
        thr = s.mean(1) + coef * s.std(1, ddof=1)
        near = np.abs(s - thr[:, None]) <= 2e-4 * thr[:, None]
        if not near.any():
            break
        d = np.where(near[:, :, None], d * np.where(s > thr[:, None], 1.01, 0.99)[:, :, None], d).astype(np.float32)
    return poison(np.zeros((B, N, ld), np.int64), d, k)[1]


def upstream(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    gp = torch.rand(B, N, generator=g) - 0.3
    gp.view(-1)[torch.randperm(B * N, generator=g)[:min(10, B * N // 4)]] = 0.0
    return gp, torch.rand(B, generator=g) - 0.3


def reference(x, ori, nrm, idx, d, ds, k, gp, gb, coef=COEF):
    """the four restatements (ds: the distances kNN_smoothing_loss is given); asserts what the bounds and the exact mask rest on"""
    r = [TR.smoothing(x, ds, idx, k, coef, gb), TR.repulsion(x, d, idx, k, H2, gp), TR.displacement(x, ori, idx, k, gp),
         TR.normal_grad(x, nrm, idx, k, gp)]
    s, thr = r[0]["s"], r[0]["thr"]
    ok = np.isfinite(thr)
    assert (np.abs(s - thr[:, None])[ok] > 1e-4 * np.abs(thr)[ok, None]).all(), "a point within 1e-4 thr of the threshold"
    # repulsion: every term either vanishes in float64 too or stays in float32's normal range with u in the measured range
    u, t = r[1]["u"], np.abs(r[1]["term"])
    live = np.isfinite(t) & (t != 0)
    assert (u[live] <= 87.0).all() and (t[live] >= 2.0 ** -126).all(), "a repulsion term in float32's subnormal range"
    return r


def fwd_bounds(r, k):
    rep, dis = r[REPULSE], r[DISPLACE]
    b_rep = ((2 * rep["u"] + C_EXP) * U24 * np.abs(rep["term"])).sum(2) / k + U24 * np.abs(rep["out"])
    th, t = dis["theta"], dis["t"]
    D = 4 * U24 * (th[:, :, None] + t + th[:, :, None])        # theta_j = t + theta_i
    b_dis = (2 * np.abs(t) * D + D * D + U24 * t * t).sum(2) / k + U24 * np.abs(dis["out"])
    return np.nan_to_num(b_rep), b_dis


# ------------------------------------------------------------------------------------------------ device
def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return (t.to(dtype) if dtype is not None else t).cuda().contiguous()


def nan_out(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


def run_all(x, ori, nrm, knn, k, gp, gb, coef=COEF, knn_s=None):
    """[loss, cond, dsmooth, rep, drep, dis, ddis, dnormal], every float output pre-filled with NaN; knn_s: the table
    kNN_smoothing_loss is given (None: knn)"""
    from geoa3_amd import ops
    B, _, N = x.shape
    knn_s = knn if knn_s is None else knn_s
    loss, cond = ops.knn_smoothing_loss(x, k, coef, knn=knn_s, out=nan_out(B), want_cond=True)
    return [loss, cond,
            ops.knn_smoothing_loss_grad(x, k, coef, g=gb, knn=knn_s, out=nan_out(B, 3, N)),
            ops.repulsion_loss(x, k, H, knn=knn, out=nan_out(B, N)),
            ops.repulsion_loss_grad(x, k, H, g=gp, knn=knn, out=nan_out(B, 3, N)),
            ops.displacement_loss(x, ori, k, knn=knn, out=nan_out(B, N)),
            ops.displacement_loss_grad(x, ori, k, g=gp, knn=knn, out=nan_out(B, 3, N)),
            ops.corr_normal_loss_grad(x, nrm, k, g=gp, knn=knn, out=nan_out(B, 3, N))]


def ratio(tag, got, ref, bound):
    got, ref = got.detach().cpu().double().numpy(), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and np.isfinite(ref).all()
    err = np.abs(got - ref)
    assert not np.isnan(err).any(), tag
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    worst = float(q.max())
    RATIOS[tag] = worst
    print("%-58s err/bound %.3f" % (tag, worst))
    assert worst <= 1.0, (tag, worst, float(err.max()))


def compare(tag, got, r, k, x, ori, rows=None):
    """got = run_all's list against the restatements r, instance by instance (rows: the instances to look at)"""
    B = x.shape[0]
    rows = list(range(B)) if rows is None else rows
    b_rep, b_dis = fwd_bounds(r, k)
    sel = lambda a: a[rows]
    assert np.array_equal(sel(got[1].cpu().numpy().astype(bool)), sel(r[SMOOTH]["mask"])), tag + " mask"
    ratio(tag + " smoothing loss", got[0][rows], sel(r[SMOOTH]["loss"]), 2 * U24 * np.abs(sel(r[SMOOTH]["loss"])))
    ratio(tag + " repulsion", got[3][rows], sel(r[REPULSE]["out"]), sel(b_rep))
    ratio(tag + " displacement", got[5][rows], sel(r[DISPLACE]["out"]), sel(b_dis))
    scale = 2 * np.abs(x.astype(np.float64) - ori.astype(np.float64))
    for mode, gi in ((SMOOTH, 2), (REPULSE, 4), (DISPLACE, 6), (NORMAL, 7)):
        bound = TR.grad_bound(r[mode], scale if mode == DISPLACE else None)
        ratio("%s d%s" % (tag, NAMES[mode]), got[gi][rows], sel(r[mode]["grad"]), sel(bound))


def equal_bits(a, b, what):
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p.view(torch.uint8 if p.dtype == torch.uint8 else torch.int32),
                           q.view(torch.uint8 if q.dtype == torch.uint8 else torch.int32)), (what, i)


def check_tables(B, N, k, seed, kinds=("random", "hub"), alone=1):
    x, ori, nrm = clouds(B, N, seed)
    gp, gb = upstream(B, N, seed + 1)
    xd, od, nd, gpd, gbd = dev(x), dev(ori), dev(nrm), dev(gp), dev(gb)
    for kind in kinds:
        idx, d, ds = table(kind, x, k, seed + 2)
        tag = "B%d N%d k%d %s" % (B, N, k, kind)
        r = reference(x, ori, nrm, idx, d, ds, k, gp, gb)
        # displacement_loss reads ori's table: the same hand-made indices serve
        dd, dsd, idd = dev(d), dev(ds), dev(idx)

        def call(lo, hi, gp_, gb_):
            c = lambda t: None if t is None else t[lo:hi].contiguous()
            return run_all(c(xd), c(od), c(nd), (c(dd), c(idd)), k, c(gp_), c(gb_), knn_s=(c(dsd), c(idd)))
        got = call(0, B, gpd, gbd)
        compare(tag, got, r, k, x, ori)
        if B == 3:      # every repulsion term of the 2^10 instance underflows: the gradient is +0.0, not NaN
            assert r[REPULSE]["tmax"][2] == 0.0
            assert torch.equal(got[4][2].view(torch.int32), torch.zeros_like(got[4][2]).view(torch.int32)), tag
        equal_bits(got, call(0, B, gpd, gbd), tag + " repeat")
        a = alone % B
        equal_bits([t[a:a + 1] for t in got], call(a, a + 1, gpd, gbd), tag + " row alone")
        # g = None equals ones, bit for bit
        equal_bits(call(0, B, torch.ones_like(gpd), torch.ones_like(gbd)), call(0, B, None, None), tag + " g None")


# ------------------------------------------------------------------------------------------------ tests
SHAPES = [(3, 2, 1), (3, 64, 63), (3, 511, 4), (3, 512, 4), (3, 513, 4), (3, 1400, 5)]


@pytest.mark.parametrize("B,N,k", SHAPES)
def test_hand_made_tables(B, N, k):
    check_tables(B, N, k, seed=1000 + N)


@pytest.mark.parametrize("N,routes", [(4262, (LDS, LDS, LDS, LDS)), (4263, (WORKSPACE, LDS, LDS, LDS)),
                                      (4380, (WORKSPACE, LDS, LDS, LDS)), (4381, (WORKSPACE, WORKSPACE, LDS, WORKSPACE))])
def test_both_sides_of_the_lds_boundary(N, routes):
    """both sides of each mode's boundary (routes: smoothing, repulsion, displacement, normal); repeats and a row alone too"""
    assert tuple(_lib.load().geoa3_debug_reg_route(m, N, 4) for m in range(4)) == routes
    check_tables(2, N, 4, seed=2000 + N)


def test_displacement_at_the_largest_cloud():
    assert _lib.load().geoa3_debug_reg_route(DISPLACE, 8192, 16) == LDS
    check_tables(1, 8192, 16, seed=3000, alone=0)


# (N = 2 is left to the hand-made tables: a search gives both points the same s_i, which IS the threshold.  The seeds of the
# two large clouds are the first of 4000 + N + 100 j that keep every s_i 2e-4 thr away from the threshold.)
@pytest.mark.parametrize("B,N,k,seed", [(B, N, k, 4000 + N) for B, N, k in SHAPES[1:]] + [(2, 4263, 4, 11963), (2, 4381, 4, 10381)])
def test_search_table(B, N, k, seed):
    """A wider table of the device's own search: the bits of the entry point's own search, and the restatement's values."""
    from geoa3_amd import ops
    x, ori, nrm = clouds(B, N, seed)
    gp, gb = upstream(B, N, seed + 1)
    xd, od, nd, gpd, gbd = dev(x), dev(ori), dev(nrm), dev(gp), dev(gb)
    K = min(k + 3, N, 64)
    wx, wo = ops.knn_self_planar(xd, K), ops.knn_self_planar(od, K)
    for w in (wx, wo):
        assert torch.isfinite(w[0]).all() and int(w[1].min()) >= 0 and int(w[1].max()) < N
    own = run_all(xd, od, nd, None, k, gpd, gbd)
    got = run_all(xd, od, nd, wx, k, gpd, gbd)
    got[5] = ops.displacement_loss(xd, od, k, knn=wo, out=nan_out(B, N))
    got[6] = ops.displacement_loss_grad(xd, od, k, g=gpd, knn=wo, out=nan_out(B, 3, N))
    equal_bits(got, own, "search table N%d" % N)
    tag = "B%d N%d k%d search" % (B, N, k)
    ix, dx, io = wx[1].cpu().numpy(), wx[0].cpu().numpy(), wo[1].cpu().numpy()
    r = reference(x, ori, nrm, ix, dx, dx, k, gp, gb)
    r[DISPLACE] = TR.displacement(x, ori, io, k, gp)
    compare(tag, got, r, k, x, ori)


def test_out_of_range_index():
    """One entry N and one -1 in instance 1: its gradients are NaN, instances 0 and 2 keep the bits of the run without them;
    displacement_loss's forward is NaN on exactly the two points."""
    B, N, k = 3, 513, 4
    x, ori, nrm = clouds(B, N, 5000)
    gp, gb = upstream(B, N, 5001)
    xd, od, nd, gpd, gbd = dev(x), dev(ori), dev(nrm), dev(gp), dev(gb)
    idx, d, _ = table("random", x, k, 5002)
    bad = idx.copy()
    bad[1, 100, 2], bad[1, 400, k] = N, -1
    clean = run_all(xd, od, nd, (dev(d), dev(idx)), k, gpd, gbd)
    got = run_all(xd, od, nd, (dev(d), dev(bad)), k, gpd, gbd)
    for gi in (2, 4, 6, 7):
        assert torch.isnan(got[gi][1]).all(), gi
        equal_bits([got[gi][[0, 2]]], [clean[gi][[0, 2]]], "oob grad %d" % gi)
    where = torch.zeros(B, N, dtype=torch.bool, device="cuda")
    where[1, 100] = where[1, 400] = True
    assert torch.isnan(got[5][where]).all()
    equal_bits([got[5][~where]], [clean[5][~where]], "oob displacement forward")
    equal_bits([got[0], got[1], got[3]], [clean[0], clean[1], clean[3]], "oob: the forwards that read distances only")


@pytest.mark.parametrize("N,route", [(513, LDS), (4263, WORKSPACE)])
def test_non_finite_distance_over_a_finite_cloud_is_loud(N, route):
    """The header's rule: the instance's smoothing loss is NaN, its mask 0 and its gradient NaN; the others keep their bits."""
    from geoa3_amd import ops
    assert _lib.load().geoa3_debug_reg_route(SMOOTH, N, 4) == route
    B, k = 3, 4
    x, _, _ = clouds(B, N, 6000 + N)
    xd = dev(x)
    gb = dev(upstream(B, N, 6001)[1])
    idx, _, d = table("random", x, k, 6002)
    knn = (dev(d), dev(idx))
    loss0, cond0 = ops.knn_smoothing_loss(xd, k, COEF, knn=knn, want_cond=True)
    grad0 = ops.knn_smoothing_loss_grad(xd, k, COEF, g=gb, knn=knn)
    assert torch.isfinite(loss0).all() and torch.isfinite(grad0).all() and cond0[1].any()
    for v in (float("nan"), float("inf"), float("-inf")):
        dn = d.copy()
        dn[1, 7, 2] = v
        knn = (dev(dn), dev(idx))
        loss, cond = ops.knn_smoothing_loss(xd, k, COEF, knn=knn, out=nan_out(B), want_cond=True)
        grad = ops.knn_smoothing_loss_grad(xd, k, COEF, g=gb, knn=knn, out=torch.zeros(B, 3, N, device="cuda"))
        assert torch.isnan(loss[1]) and not cond[1].any() and torch.isnan(grad[1]).all(), v
        equal_bits([loss[[0, 2]], cond[[0, 2]], grad[[0, 2]]], [loss0[[0, 2]], cond0[[0, 2]], grad0[[0, 2]]], "clean instances")
        r = TR.smoothing(x, dn, idx, k, COEF)
        assert np.isnan(r["loss"][1]) and not r["mask"][1].any() and np.isnan(r["grad"][1]).all()


def test_empty_mask_gives_zero_loss_and_positive_zero_gradient():
    from geoa3_amd import ops
    B, N, k = 3, 513, 4
    x, _, _ = clouds(B, N, 7000)
    idx, _, d = table("random", x, k, 7001)
    r = TR.smoothing(x, d, idx, k, 1e6)
    assert not r["mask"].any() and np.isfinite(r["thr"]).all()
    knn = (dev(d), dev(idx))
    loss, cond = ops.knn_smoothing_loss(dev(x), k, 1e6, knn=knn, out=nan_out(B), want_cond=True)
    grad = ops.knn_smoothing_loss_grad(dev(x), k, 1e6, knn=knn, out=nan_out(B, 3, N))
    zero = torch.zeros(1, device="cuda").view(torch.int32)
    assert not cond.any() and (loss.view(torch.int32) == zero).all() and (grad.view(torch.int32) == zero).all()


# ------------------------------------------------------------------------------------------------ geoa3_reg_fold alone
@pytest.mark.parametrize("B,N", [(1, 1), (3, 1), (300, 1), (1, 513), (3, 513), (300, 513), (3, 60000)])
def test_reg_fold_alone(B, N):
    """constrain (+)= w loss, g (+)= w grad: one float32 multiply and one add, 2^-23 (|old| + |w v|); a NULL output is
    honoured and nothing beside the outputs is written (B = 3, N = 60000: the grid-stride loop, 2048 blocks)."""
    from geoa3_amd import ops
    gen = torch.Generator().manual_seed(B * 7 + N)
    w, PAD = -0.37, 64
    loss, grad = (torch.rand(B, generator=gen) - 0.4).cuda(), (torch.randn(B * 3 * N, generator=gen)).cuda()
    old_c, old_g = torch.randn(B, generator=gen).cuda(), torch.randn(B * 3 * N, generator=gen).cuda()
    for add in (False, True):
        for use_c, use_g in ((True, True), (True, False), (False, True)):
            cbuf, gbuf = torch.full((B + 2 * PAD,), 7.5, device="cuda"), torch.full((B * 3 * N + 2 * PAD,), 7.5, device="cuda")
            c, g = cbuf[PAD:PAD + B], gbuf[PAD:PAD + B * 3 * N]
            c.copy_(old_c if add else torch.full_like(old_c, float("nan")))
            g.copy_(old_g if add else torch.full_like(old_g, float("nan")))
            before_c, before_g = cbuf.clone(), gbuf.clone()
            ops.reg_fold(loss if use_c else None, grad if use_g else None, w, B, N, constrain=c if use_c else None,
                         constrain_add=add, g=g if use_g else None, g_add=add)
            for what, used, buf, before, n, old, v in (("constrain", use_c, cbuf, before_c, B, old_c, loss),
                                                       ("g", use_g, gbuf, before_g, B * 3 * N, old_g, grad)):
                assert torch.equal(buf[:PAD], before[:PAD]) and torch.equal(buf[PAD + n:], before[PAD + n:])
                if not used:
                    assert torch.equal(buf.view(torch.int32), before.view(torch.int32))
                    continue
                o = old.double() if add else torch.zeros_like(old, dtype=torch.float64)
                wv = float(np.float32(w)) * v.double()
                ref = o + wv
                ratio("reg_fold B%d N%d add%d c%d g%d %s" % (B, N, add, use_c, use_g, what),
                      buf[PAD:PAD + n], ref.cpu().numpy(), (2 * U24 * (o.abs() + wv.abs())).cpu().numpy())


def test_zz_print_ratios():
    """the largest err / bound per family (what the module docstring records)"""
    fam = {}
    for tag, v in RATIOS.items():
        key = tag.split(" ", 4)[-1] if tag.startswith("B") else "reg_fold"
        fam[key] = max(fam.get(key, 0.0), v)
    for key in sorted(fam):
        print("max err/bound  %-28s %.3f" % (key, fam[key]))
