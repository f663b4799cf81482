"""Non-finite points in every neighbour search: geoa3_nn1_pair, geoa3_grid_nn1_pair under every policy and size class of its
dispatcher, geoa3_knn, and every route of geoa3_knn_self -- held bit for bit to tests/_nonfinite_ref.py (the rule in float32
numpy) and to the all-pairs kernels.

Every case is a batch of three instances with the poisoned one in the middle: instances 0 and 2 must come out with the bits
of the same call on the clean batch (an instance that diverges in the attack loop may not touch its neighbours), instance 1
with the reference's.  Part two runs the consumers of the K-NN table -- every route of geoa3_geo_loss_grad and geoa3_kappa --
on the tables of a poisoned cloud, rows of -1 included ("NaN rule of the searches").
Runs on the GPU box: python -m pytest tests/test_gpu_nonfinite.py -m gpu"""
import numpy as np
import pytest
import torch

from oracle import geoa3_oracle as O
from tests import _nonfinite_ref as R

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ops():
    from geoa3_amd import ops as _ops
    assert torch.cuda.is_available(), "needs the MI355X"
    return _ops


def dev(x):
    return x.contiguous().cuda()


# ---- the poisons: x is ONE instance [3, n], changed in place; j = an index that is some query's own seed
def _nan_coord(x, n, j):
    x[1, n // 3] = NAN


def _nan_point(x, n, j):
    x[:, n // 3] = NAN


def _inf_coord(x, n, j):
    x[0, n // 3] = INF


def _inf_both_signs(x, n, j):          # +inf and -inf on one axis: the extent is +inf, their difference too
    x[2, n // 3] = INF
    x[2, (2 * n) // 3] = -INF


def _nan_and_inf(x, n, j):
    x[:, n // 3] = NAN
    x[:, (2 * n) // 3] = INF


def _at_index_0(x, n, j):              # index 0 is the answer of a query that finds nothing
    x[:, 0] = NAN


def _at_last_index(x, n, j):
    x[0, n - 1] = INF


def _at_a_seed(x, n, j):               # without a prior, query j is seeded with searched point j
    x[:, j] = NAN


def _all_nan(x, n, j):
    x[:] = NAN


def _all_inf(x, n, j):                 # the box's extent is inf - inf: the grid's cell size itself is NaN
    x[:] = INF


POISONS = {"nan_coord": _nan_coord, "nan_point": _nan_point, "inf_coord": _inf_coord, "inf_both_signs": _inf_both_signs,
           "nan_and_inf": _nan_and_inf, "at_index_0": _at_index_0, "at_last_index": _at_last_index, "at_a_seed": _at_a_seed,
           "all_nan": _all_nan, "all_inf": _all_inf}


def clean_pair(na, nr, noise, cad, seed):
    """-> (queries [3,3,na], searched [3,3,nr]) on the CPU: the clean cloud plus noise against the clean cloud."""
    m = max(na, nr)
    if cad:
        from geoa3_amd.data import synthetic_cad_clouds
        ori, _ = synthetic_cad_clouds(3, m, seed=seed)
    else:
        ori, _ = O.make_synthetic_clouds(3, m, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    a = ori[:, :, :na] + noise * torch.randn(3, 3, na, generator=g)
    return a.contiguous(), ori[:, :, :nr].contiguous()


def bits_equal(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def middle_matches_ref(got_d, got_i, ref_d, ref_i):
    return (np.array_equal(got_i[1].cpu().numpy(), ref_i) and R.same_bits(got_d[1].cpu().numpy(), ref_d))


def outer_keep_their_bits(got, clean):
    return all(bits_equal(g[[0, 2]], c[[0, 2]]) for g, c in zip(got, clean))


# ------------------------------------------------------------------------------------------------------------------
# 1-NN.  One size for every class of geoa3_launch_grid_nn1_policy (M = max(Na, Nr)).  Which search a policy (brute_frac,
# filter) forces, by the code (geom_grid.hip; no route query exists, so it cannot be observed):
#   M < 32:        the filter is off (it needs 32 points a side): grid_nn1_kernel<1>, walk or in-kernel sweep
#   32..1024:      filter policies -> geoa3_launch_nn1_filter (nf::search, no grid); (0, 0) -> the sweep of grid_nn1_kernel<1>;
#                  (1e9, 0) -> its walk
#   1025..4096:    grid_nn1_kernel<2> / <4>.  brute_frac = 0 makes `all > brute_frac * Nq * M` true for any workgroup whose
#                  boxes hold a point: (0, 1) -> the dense-box branch with the filter, grid_filter_sorted -- or, where a point
#                  or a query is not finite, grid_filter_search's exact sweep; (0, 0) -> the dense-box branch's in-kernel sweep;
#                  (1e9, 0) -> the balanced walk.  Shipped (0.03, filter): the walk at noise 0.03 on clean workgroups; a
#                  poisoned query's radius is infinite, its box holds the whole cloud, and with noise 0.3 the workgroup
#                  passes brute_frac and takes the dense-box branch (the "far" sizes below)
#   > 4096:        filter policies -> geoa3_launch_nn1_filter in chunks of 1024 candidates; no grid fits: filter = 0 is refused
# ------------------------------------------------------------------------------------------------------------------
NN1_SIZES = {   # name: (Na, Nr, noise, CAD-like clouds, policies run)
    "lt32": (20, 27, 0.03, False, "all"),
    "300v777": (300, 777, 0.03, True, "all"),
    "1024": (1024, 1024, 0.03, False, "all"),
    "ppt2_1025": (1025, 1025, 0.03, True, "all"),          # the last lanes have no second query
    "ppt2_1025_far": (1025, 1025, 0.3, True, "shipped"),
    "ppt4_2500v2049": (2500, 2049, 0.03, True, "all"),
    "ppt4_2500v2049_far": (2500, 2049, 0.3, True, "shipped"),
    "ppt4_4096": (4096, 4096, 0.03, False, "all"),
    "gt4096": (4100, 4100, 0.03, False, "all"),
}
NN1_POLICIES = (("filter", (0.0, 1), None), ("filter+prior", (0.0, 1), "exact"), ("filter+junk prior", (0.0, 1), "junk"),
                ("sweep", (0.0, 0), None), ("walk", (1e9, 0), "exact"), ("shipped", None, "exact"),
                ("shipped, no prior", None, None))
_nn1_clean = {}


def nn1_policies(size):
    na, nr, _, _, which = NN1_SIZES[size]
    for label, policy, prior in NN1_POLICIES:
        if which == "shipped" and policy is not None:
            continue
        if max(na, nr) > 4096 and policy is not None and policy[1] == 0:     # (walk and sweep need the grid)
            continue
        yield label, policy, prior


def nn1_run(ops, A, Rr, want, policy, prior, both=True):
    pr = None
    if prior == "exact":
        pr = (want[1].clone(), want[3].clone() if both else None)
    elif prior == "junk":
        pr = (torch.full_like(want[1], 10 ** 6), torch.full_like(want[3], -5))
    return ops.nn1_pair(A, Rr, both=both, method="grid", prior=pr, policy=policy)


def nn1_clean(ops, size):
    """The clean batch of a size through the all-pairs kernel and every policy, once per module."""
    if size not in _nn1_clean:
        na, nr, noise, cad, _ = NN1_SIZES[size]
        a, r = clean_pair(na, nr, noise, cad, seed=na + nr)
        A, Rr = dev(a), dev(r)
        want = ops.nn1_pair(A, Rr)
        runs = {label: nn1_run(ops, A, Rr, want, policy, prior) for label, policy, prior in nn1_policies(size)}
        _nn1_clean[size] = (a, r, want, runs)
    return _nn1_clean[size]


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("place", ["queries", "searched"])
@pytest.mark.parametrize("size", list(NN1_SIZES))
def test_nn1_poisoned_instance_follows_the_rule_and_its_neighbours_keep_their_bits(ops, size, place, poison):
    na, nr = NN1_SIZES[size][:2]
    a0, r0, clean_want, clean_runs = nn1_clean(ops, size)
    a, r = a0.clone(), r0.clone()
    if place == "queries":
        POISONS[poison](a[1], na, min(na, nr) // 2)
    else:
        POISONS[poison](r[1], nr, min(na, nr) // 2)
    ref = R.nn1(a[1].numpy(), r[1].numpy()) + R.nn1(r[1].numpy(), a[1].numpy())
    A, Rr = dev(a), dev(r)
    want = ops.nn1_pair(A, Rr)
    wrong = []
    if not (middle_matches_ref(want[0], want[1], ref[0], ref[1]) and middle_matches_ref(want[2], want[3], ref[2], ref[3])):
        wrong.append("all pairs: instance 1 differs from the reference")
    if not outer_keep_their_bits(want, clean_want):
        wrong.append("all pairs: instances 0 / 2 differ from the clean batch")
    for label, policy, prior in nn1_policies(size):
        got = nn1_run(ops, A, Rr, want, policy, prior)
        if not all(bits_equal(w, x) for w, x in zip(want, got)):
            nd = [(w.view(torch.int32) != x.view(torch.int32)).sum().item() for w, x in zip(want, got)]
            wrong.append("%s: differs from the all-pairs kernel in %s entries (d_ar, i_ar, d_ra, i_ra)" % (label, nd))
        if not outer_keep_their_bits(got, clean_runs[label]):
            wrong.append("%s: instances 0 / 2 differ from the clean batch" % label)
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("size", [s for s in NN1_SIZES if not s.endswith("_far")])
def test_nn1_one_direction_only(ops, size):
    """both = False (pseudo_chamfer_loss): once per size class, a NaN point and an inf point among the queries AND in the
    searched cloud."""
    na, nr = NN1_SIZES[size][:2]
    a0, r0, clean_want, _ = nn1_clean(ops, size)
    a, r = a0.clone(), r0.clone()
    _nan_and_inf(a[1], na, 0)
    _inf_coord(r[1], nr, 0)
    ref = R.nn1(a[1].numpy(), r[1].numpy())
    A, Rr = dev(a), dev(r)
    want = ops.nn1_pair(A, Rr, both=False)
    assert want[2] is None and want[3] is None
    assert middle_matches_ref(want[0], want[1], ref[0], ref[1])
    assert outer_keep_their_bits(want[:2], clean_want[:2])
    for label, prior in (("shipped", (want[1].clone(), None)), ("shipped, no prior", None)):
        got = ops.nn1_pair(A, Rr, both=False, method="grid", prior=prior)
        assert bits_equal(got[0], want[0]) and torch.equal(got[1], want[1]), label
    for label, policy, _ in nn1_policies(size):               # the forced branches with d_ra == NULL
        if policy is not None:
            got = ops.nn1_pair(A, Rr, both=False, method="grid", policy=policy)
            assert bits_equal(got[0], want[0]) and torch.equal(got[1], want[1]), label


# ------------------------------------------------------------------------------------------------------------------
# K-NN.  A query with a NaN coordinate collects nothing: K times (+inf, -1) -- the opposite of geoa3_knn_nd, which reports
# a NaN distance as +inf and keeps every index in range.  Three priors: none; the CLEAN cloud's table (the attack loop's
# situation: last iteration was finite); the poisoned cloud's OWN table, whose rows hold -1.
# ------------------------------------------------------------------------------------------------------------------
KNN_SIZES = {"300v777_k8": (300, 777, 8), "700v1100_k33": (700, 1100, 33), "100v150_k41": (100, 150, 41)}   # lists of 40 / 72 / 96
_knn_clean = {}


def knn_clean(ops, size):
    if size not in _knn_clean:
        nq, nr, K = KNN_SIZES[size]
        q, r = clean_pair(nq, nr, 0.03, True, seed=nq + K)
        _knn_clean[size] = (q, r, ops.knn_planar(dev(q), dev(r), K))
    return _knn_clean[size]


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("place", ["queries", "searched"])
@pytest.mark.parametrize("size", list(KNN_SIZES))
def test_knn_poisoned_instance_follows_the_rule_and_its_neighbours_keep_their_bits(ops, size, place, poison):
    nq, nr, K = KNN_SIZES[size]
    q0, r0, clean = knn_clean(ops, size)
    q, r = q0.clone(), r0.clone()
    if place == "queries":
        POISONS[poison](q[1], nq, min(nq, nr) // 2)
    else:
        POISONS[poison](r[1], nr, min(nq, nr) // 2)
    ref_d, ref_i = R.knn(q[1].numpy(), r[1].numpy(), K)
    Q, Rr = dev(q), dev(r)
    own = ops.knn_planar(Q, Rr, K)
    wrong = []
    for label, prior in (("no prior", None), ("clean prior", clean[1]), ("own prior", own[1].clone())):
        d, i = ops.knn_planar(Q, Rr, K, prior=prior)
        if not middle_matches_ref(d, i, ref_d, ref_i):
            wrong.append("%s: instance 1 differs from the reference" % label)
        if not outer_keep_their_bits((d, i), clean):
            wrong.append("%s: instances 0 / 2 differ from the clean batch" % label)
    assert not wrong, "\n".join(wrong)


# GEOA3_KNN_ROUTE_* of include/geoa3_hip_debug.h
ALLPAIRS, CELLGRID, SLAB40, SLAB72, SLAB96, SLABP32, SLABP56 = range(7)
SELF_ROUTES = {   # name: (B, N, K, method, scratch given, route)
    "slab40": (3, 300, 8, 3, True, SLAB40),
    "slab72": (3, 300, 33, 3, True, SLAB72),
    "slab96": (3, 300, 41, 3, True, SLAB96),
    "slab40_two_chunks": (3, 1100, 8, 3, True, SLAB40),        # more than one staging chunk of 1024
    "slabp32": (3, 300, 8, 4, True, SLABP32),
    "slabp56": (3, 300, 33, 4, True, SLABP56),
    "cellgrid_1001": (3, 1001, 8, 2, True, CELLGRID),
    "cellgrid_2049": (3, 2049, 8, 0, True, CELLGRID),
    "cellgrid_4096_b1": (1, 4096, 8, 0, True, CELLGRID),       # the poisoned instance alone
    "allpairs": (3, 300, 8, 0, False, ALLPAIRS),
}
_self_clean = {}


def self_clean(ops, name):
    if name not in _self_clean:
        B, N, K, method, has_scratch, _ = SELF_ROUTES[name]
        ori, _ = O.make_synthetic_clouds(3, N, seed=N + K)
        pc = (ori + 0.03 * torch.randn(3, 3, N, generator=torch.Generator().manual_seed(N))).contiguous()
        pc[:, :, 5] = pc[:, :, 4]                              # a duplicate: exact ties, the lower index first
        P = dev(pc)
        table = ops.knn_planar(P, P, K)
        scratch = ops.knn_self_scratch(3, N, "cuda") if has_scratch else None
        runs = {"clean prior": ops.knn_self_planar(P, K, prior=table[1], scratch=scratch, method=method)}
        runs["own prior"] = runs["clean prior"]
        _self_clean[name] = (pc, table, scratch, runs)
    return _self_clean[name]


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("name", list(SELF_ROUTES))
def test_knn_self_every_route(ops, name, poison):
    from geoa3_amd import _lib
    B, N, K, method, has_scratch, route = SELF_ROUTES[name]
    assert _lib.load().geoa3_debug_knn_self_route(B, N, K, method, 1, int(has_scratch)) == route
    pc0, clean, scratch, clean_runs = self_clean(ops, name)
    pc = pc0.clone()
    POISONS[poison](pc[1], N, N // 2)
    ref_d, ref_i = R.knn(pc[1].numpy(), pc[1].numpy(), K)
    lo, hi = (1, 2) if B == 1 else (0, 3)                      # B = 1: the poisoned instance alone
    P = dev(pc[lo:hi])
    mid = 1 - lo
    want = ops.knn_planar(P, P, K)                             # the all-pairs kernel
    wrong = []
    if not (np.array_equal(want[1][mid].cpu().numpy(), ref_i) and R.same_bits(want[0][mid].cpu().numpy(), ref_d)):
        wrong.append("all pairs: the poisoned instance differs from the reference")
    if B == 3 and not outer_keep_their_bits(want, clean):
        wrong.append("all pairs: instances 0 / 2 differ from the clean batch")
    for label, prior in (("clean prior", clean[1][lo:hi].contiguous()), ("own prior", want[1].clone())):
        d, i = ops.knn_self_planar(P, K, prior=prior, scratch=scratch, method=method)
        if not (bits_equal(d, want[0]) and torch.equal(i, want[1])):
            nd = ((d.view(torch.int32) != want[0].view(torch.int32)).sum().item(), (i != want[1]).sum().item())
            wrong.append("%s: differs from the all-pairs kernel in %s entries (distances, indices)" % (label, nd))
        if B == 3 and not outer_keep_their_bits((d, i), clean_runs[label]):
            wrong.append("%s: instances 0 / 2 differ from the clean batch" % label)
    # without a prior every route is the all-pairs kernel (nothing to prune with): the same bits again
    assert _lib.load().geoa3_debug_knn_self_route(B, N, K, method, 0, int(has_scratch)) == ALLPAIRS
    d, i = ops.knn_self_planar(P, K, prior=None, scratch=scratch, method=method)
    if not (bits_equal(d, want[0]) and torch.equal(i, want[1])):
        wrong.append("no prior: differs from the all-pairs kernel")
    assert not wrong, "\n".join(wrong)


# ------------------------------------------------------------------------------------------------------------------
# The consumers of the tables.  geoa3_knn / geoa3_knn_self write -1 into the row of a point with a NaN coordinate, and the
# attack loop hands that table to geoa3_geo_loss_grad as it is.  Rule (geom_loss_fix.h, geo_tab_idx): every entry of a
# table -- knn_adv and i_oa against [0, N), i_ao against [0, Nr) -- is compared with its range before it forms an address;
# an entry outside is not followed and its term counts as NaN.  Hausdorff point of an instance whose d_ao holds +inf: the
# LOWEST index among the +inf entries (the arg-max takes the larger value, then the lower index; the 1-NN search never
# writes a NaN distance) -- on every route.
# Reference: tests/_geo_table_ref.objective in float64 on the same tables, a -1 replaced by the row's own index (that row's
# own point is NaN, so the row is NaN anyway).  Tolerances: those of test_pair_parallel_objective_special_paths.
# ------------------------------------------------------------------------------------------------------------------
from tests import _geo_table_ref as G   # noqa: E402

FUSED, BIG, LISTS, ATOMICS, WIDE = 0, 1, 2, 3, 4     # GEOA3_GEO_ROUTE_* of include/geoa3_hip_debug.h
# name: (N, deterministic, scratch (None = the wrapper's own choice, False = none), wide_ranges, route, batch).
# batch: 3 = the three instances; 129 = the three repeated 43 times; 1 = the poisoned instance alone.  geo_fused_kernel has two
# forms, chosen by geo_plan from the batch size alone (S doubles while S < 4, 2 B S <= 256 and ceil(N / 2S) >= 64): at
# N = 300, B = 3 and B = 1 give S = 4 owner-range workgroups per instance (the pair-parallel form of small batches), B = 129
# gives S = 1, one workgroup per instance with rows for the whole cloud -- the form the 250-instance batch runs.
GEO_ROUTES = {
    "fused_s4": (300, True, None, None, FUSED, 3),
    "fused_s4_alone": (300, True, None, None, FUSED, 1),
    "fused_s1": (300, True, None, None, FUSED, 129),
    "atomics": (300, False, False, None, ATOMICS, 3),
    "lists": (1100, True, False, None, LISTS, 3),
    "big": (1100, True, None, None, BIG, 3),
    "wide": (300, True, None, 0, WIDE, 3),
}
GEO_K = 8


def _poison_adv_nan(adv, ori, N):
    adv[1, :, N // 3] = NAN


def _poison_adv_inf(adv, ori, N):
    adv[1, 0, N // 3] = INF


def _poison_ori_nan(adv, ori, N):      # i_oa / d_oa of that clean point: (index 0, +inf)
    ori[1, :, N // 3] = NAN


GEO_POISONS = {"adv_nan_point": _poison_adv_nan, "adv_inf_point": _poison_adv_inf, "ori_nan_point": _poison_ori_nan}
GEO_FORMS = ("curvature", "distance_only", "dkappa")
_geo_clean = {}


def geo_inputs(ops, adv, ori, nrm, kappa_ori, form, N):
    A, Oo = dev(adv), dev(ori)
    d_ao, i_ao, d_oa, i_oa = ops.nn1_pair(A, Oo)
    kw = dict(d_ao=d_ao, i_ao=i_ao, d_oa=d_oa, i_oa=i_oa, dis_type=1, w_dis=1.0, w_hd=0.1)
    if form != "distance_only":
        _, knn_adv = ops.knn_planar(A, A, GEO_K + 1)
        kw.update(normal_ori=nrm, kappa_ori=kappa_ori, knn_adv=knn_adv, k=GEO_K)
        if form == "dkappa":
            kw.update(dkappa=dev(torch.randn(3, N, generator=torch.Generator().manual_seed(N))), w_curv=0.0)
        else:
            kw.update(w_curv=1.0)
    return A, Oo, kw


def geo_run(ops, A, Oo, kw, name):
    """-> the outputs of instances 0, 1, 2 (batch 1: of the poisoned instance at position 1, the others NaN)."""
    N, det, scratch, wide, route, batch = GEO_ROUTES[name]
    if wide is None:    # the route, before the call (as tests/test_geo_route.py: only sizes, flags and WHICH pointers count)
        from geoa3_amd import _lib
        import ctypes
        PTR = 0x1000
        has_tab = "knn_adv" in kw
        # BIG needs the curvature term; without a table the wrapper gives no scratch and the call is FUSED / LISTS / ATOMICS
        a = _lib.GeoArgs(adv=PTR, ori=PTR, d_ao=PTR, i_ao=PTR, d_oa=PTR, i_oa=PTR, B=batch, N=N, k=GEO_K if has_tab else 0,
                         Nr=N, dis_type=1, single_side=0, w_dis=1.0, w_hd=0.1, w_curv=float(kw.get("w_curv", 0.0)),
                         constrain=PTR, grad=PTR, deterministic=int(det),
                         scratch=PTR if (scratch is None and has_tab and N > 1024) else None)
        if has_tab:
            a.normal_ori = a.kappa_ori = a.knn_adv = PTR
            if "dkappa" in kw:
                a.dkappa = PTR
        want = route if (has_tab or route != BIG) else LISTS
        assert _lib.load().geoa3_debug_geo_route(ctypes.byref(a)) == want, name

    def shape(x):
        if not torch.is_tensor(x):
            return x
        if batch == 1:
            return x[1:2].contiguous()
        return x.repeat(batch // 3, *([1] * (x.dim() - 1))).contiguous() if batch > 3 else x
    out = ops.geo_loss_grad(shape(A), shape(Oo), deterministic=det, scratch=scratch, wide_ranges=wide,
                            want_kappa="knn_adv" in kw, **{n: shape(v) for n, v in kw.items()})
    res = {}
    for n, v in out.items():
        if batch == 1:
            full = torch.full((3,) + tuple(v.shape[1:]), NAN, device=v.device, dtype=v.dtype)
            full[1] = v[0]
            res[n] = full
        else:
            if batch > 3 and det:     # every copy of the three instances: the same bits, wherever it stands in the batch
                assert bits_equal(v, v[:3].repeat(batch // 3, *([1] * (v.dim() - 1)))), n
            res[n] = v[:3].clone()
    return res


def geo_clean(ops, name, form):
    N = GEO_ROUTES[name][0]
    if N not in _geo_clean:
        ori, nrm = O.make_synthetic_clouds(3, N, seed=N + 1)
        adv = (ori + 0.02 * torch.randn(3, 3, N, generator=torch.Generator().manual_seed(N))).contiguous()
        _, knn_ori = ops.knn_planar(dev(ori), dev(ori), GEO_K + 1)
        _geo_clean[N] = (adv, ori, dev(nrm), ops.kappa(dev(ori), dev(nrm), knn_ori), {})
    adv0, ori0, nrm, kappa_ori, clean_runs = _geo_clean[N]
    if (name, form) not in clean_runs:
        clean_runs[(name, form)] = geo_run(ops, *geo_inputs(ops, adv0, ori0, nrm, kappa_ori, form, N), name)
    return adv0, ori0, nrm, kappa_ori, clean_runs[(name, form)]


def neighbours_keep_their_bits(name, got, clean):
    if GEO_ROUTES[name][5] == 1:
        return
    for n in got:
        if name == "atomics" and n == "grad":                   # (LDS float atomics: the order of a sum is free, bits are not promised)
            x, c = got[n][[0, 2]].cpu().numpy(), clean[n][[0, 2]].cpu().numpy()
            np.testing.assert_allclose(x, c, rtol=2e-4, atol=2e-6 * max(float(np.abs(c).max()), 1.0))
        else:
            assert bits_equal(got[n][[0, 2]], clean[n][[0, 2]]), n


@pytest.mark.parametrize("form", GEO_FORMS)
@pytest.mark.parametrize("poison", list(GEO_POISONS))
@pytest.mark.parametrize("name", list(GEO_ROUTES))
def test_objective_on_the_tables_of_a_poisoned_cloud(ops, name, poison, form):
    N = GEO_ROUTES[name][0]
    adv0, ori0, nrm, kappa_ori, clean = geo_clean(ops, name, form)
    adv, ori = adv0.clone(), ori0.clone()
    GEO_POISONS[poison](adv, ori, N)
    A, Oo, kw = geo_inputs(ops, adv, ori, nrm, kappa_ori, form, N)
    if poison == "adv_nan_point" and form != "distance_only":
        assert (kw["knn_adv"][1, N // 3] == -1).all()          # the table does hold -1
    got = geo_run(ops, A, Oo, kw, name)
    neighbours_keep_their_bits(name, got, clean)
    # the poisoned instance against float64 on the same tables
    ref_kw = {n: (v[1:2] if torch.is_tensor(v) else v) for n, v in kw.items() if n not in ("d_ao", "d_oa", "k")}
    if "knn_adv" in ref_kw:
        t = ref_kw["knn_adv"].clone()
        rows = torch.arange(N, device=t.device).view(1, N, 1).expand_as(t)
        ref_kw["knn_adv"] = torch.where(t < 0, rows.to(t.dtype), t)
    hd_arg = torch.from_numpy(np.array([int(np.argmax(kw["d_ao"][1].cpu().numpy()))]))     # (the first of equal maxima)
    with np.errstate(all="ignore"):
        ref = G.objective(adv[1:2], ori[1:2], hd_arg=hd_arg, **ref_kw)
    wrong = []
    # (under a given dkappa the kernels still report curvature_loss, which is no part of that objective: not compared)
    for n in ("dis_loss", "hd_loss", "constrain") + (() if form == "dkappa" else ("curv_loss",)):
        r, x = ref[n][0].item(), got[n][1].item()
        print(name, poison, form, n, "reference", r, "kernel", x)
        if not np.isfinite(r):
            if np.isfinite(x):
                wrong.append("%s: reference %r, kernel finite %r" % (n, r, x))
        elif not np.isclose(x, r, rtol=5e-5, atol=1e-7):
            wrong.append("%s: reference %r, kernel %r" % (n, r, x))
    rg, xg = ref["grad"][0].numpy(), got["grad"][1].cpu().numpy().astype(np.float64)
    hidden = ~np.isfinite(rg) & np.isfinite(xg)
    print(name, poison, form, "gradient entries: reference non-finite", int((~np.isfinite(rg)).sum()), "kernel non-finite",
          int((~np.isfinite(xg)).sum()), "finite in the kernel where the reference is not", int(hidden.sum()))
    if hidden.any():
        wrong.append("gradient: %d entries finite where the reference is not, first at %s" % (hidden.sum(), np.argwhere(hidden)[0]))
    both = np.isfinite(rg) & np.isfinite(xg)
    more = np.isfinite(rg) & ~np.isfinite(xg)
    # the fixed-point routes poison a whole DESTINATION (its sticky bit: all three components) where one of its terms is not
    # representable -- only points of which the reference has a non-finite component too; the other routes poison exactly
    # the reference's entries
    if name in ("big", "wide"):
        more = more & ~(~np.isfinite(rg)).any(axis=0, keepdims=True)
    if more.any():
        wrong.append("gradient: %d entries non-finite where the reference is finite, first at %s" % (more.sum(), np.argwhere(more)[0]))
    scale = float(np.abs(rg[both]).max()) if both.any() else 0.0
    if both.any() and not np.allclose(xg[both], rg[both], rtol=2e-4, atol=2e-6 * max(scale, 1.0)):
        wrong.append("gradient: finite entries differ, max abs error %g at scale %g" % (np.abs(xg[both] - rg[both]).max(), scale))
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("form", GEO_FORMS)
@pytest.mark.parametrize("name", list(GEO_ROUTES))
def test_objective_does_not_follow_a_table_entry_outside_the_cloud(ops, name, form):
    """Entries written by hand into the rows of FINITE points of the clean cloud's tables, where only the guard makes the
    term NaN (a point that is NaN itself is NaN with or without it): knn_adv[1, r, 3] = -1 and [1, r, 5] = N + 5, i_ao[1, r2]
    = Nr + 7, i_ao[1, r2 + 1] = -1, i_oa[1, r3] = -1.  Expected: kappa_adv of r and r2 NaN (with the curvature table), the
    gradient of r (table), r2, r2 + 1 NaN, dis_loss and constrain NaN (the clean point r3 names no point); every point that is
    neither one of these, nor named by their rows (their NaN coefficient pulls on it), nor the point r3 named before, keeps
    the clean run's gradient; the neighbours keep their bits.  The poisoned instance stands in the middle of the batch."""
    N = GEO_ROUTES[name][0]
    adv0, ori0, nrm, kappa_ori, clean = geo_clean(ops, name, form)
    A, Oo, kw = geo_inputs(ops, adv0, ori0, nrm, kappa_ori, form, N)
    r, r2, r3 = N // 4, N // 2, (3 * N) // 4
    kw["i_ao"] = kw["i_ao"].clone()
    kw["i_oa"] = kw["i_oa"].clone()
    named_before = int(kw["i_oa"][1, r3])
    kw["i_ao"][1, r2] = N + 7
    kw["i_ao"][1, r2 + 1] = -1
    kw["i_oa"][1, r3] = -1
    touched = {r2, r2 + 1, named_before}
    if "knn_adv" in kw:
        kw["knn_adv"] = kw["knn_adv"].clone()
        for c in (r, r2, r2 + 1):
            touched |= set(kw["knn_adv"][1, c, 1:].tolist())
        kw["knn_adv"][1, r, 3] = -1
        kw["knn_adv"][1, r, 5] = N + 5
        touched.add(r)
    got = geo_run(ops, A, Oo, kw, name)
    neighbours_keep_their_bits(name, got, clean)
    g = got["grad"][1].cpu().numpy()
    bad_pts = [r2, r2 + 1] + ([r] if "knn_adv" in kw else [])
    assert np.isnan(g[:, bad_pts]).all(), g[:, bad_pts]
    assert np.isnan(got["dis_loss"][1].item()) and np.isnan(got["constrain"][1].item())
    if "knn_adv" in kw:
        ka = got["kappa_adv"][1].cpu().numpy()
        assert np.isnan(ka[[r, r2, r2 + 1]]).all()
        keep = np.ones(N, dtype=bool)
        keep[[r, r2, r2 + 1]] = False
        assert R.same_bits(ka[keep], clean["kappa_adv"][1].cpu().numpy()[keep])
    keep = np.ones(N, dtype=bool)
    keep[sorted(touched)] = False
    c = clean["grad"][1].cpu().numpy()
    np.testing.assert_allclose(g[:, keep], c[:, keep], rtol=2e-4, atol=2e-6 * max(float(np.abs(c).max()), 1.0))


def test_kappa_does_not_follow_an_index_outside_the_cloud(ops):
    """geoa3_kappa (both forms of kappa_kernel: the cloud in LDS from 2048 points on) against itself on the table brought
    into range by hand: (1) the search's own table of a cloud with a NaN point -- that row is -1 and NaN either way, every
    other row has the same bits; (2) -1 and N + 3 written into the rows of two FINITE points, and nn_idx[1, r3] = -1: only
    the guard makes those three values NaN, the rest keeps its bits; (3) ops.corresponding_normal_loss, which hands the
    table over as it is, gives what it gave with the table clamped first."""
    for N in (300, 2100):
        ori, nrm = O.make_synthetic_clouds(3, N, seed=N)
        pc = ori.clone()
        pc[1, :, N // 3] = NAN
        P, Nm = dev(pc), dev(nrm)
        _, tab = ops.knn_planar(P, P, GEO_K + 1)
        assert (tab[1, N // 3] == -1).all()
        clamped = tab.clamp(0, N - 1)
        assert not torch.equal(clamped, tab)
        want, out = ops.kappa(P, Nm, clamped), ops.kappa(P, Nm, tab)
        assert torch.isnan(out[1, N // 3]) and torch.isnan(want[1, N // 3])
        keep = torch.ones(3, N, dtype=torch.bool, device="cuda")
        keep[1, N // 3] = False
        assert bits_equal(out[keep], want[keep])
        # (3)
        got = ops.corresponding_normal_loss(P, Nm, k=GEO_K)
        bad = torch.isnan(P).any(dim=1).any(dim=1).view(3, 1)
        assert R.same_bits(got.cpu().numpy(), torch.where(bad, torch.full_like(want, NAN), want).cpu().numpy())
        # (2) on the clean cloud
        Pc = dev(ori)
        _, tab = ops.knn_planar(Pc, Pc, GEO_K + 1)
        nn = torch.arange(N, dtype=torch.int32, device="cuda").repeat(3, 1).contiguous()
        want = ops.kappa(Pc, Nm, tab, nn_idx=nn)
        r, r2, r3 = N // 4, N // 2, (3 * N) // 4
        hand, nn_hand = tab.clone(), nn.clone()
        hand[1, r, 2] = -1
        hand[1, r2, GEO_K] = N + 3
        nn_hand[1, r3] = -1
        out = ops.kappa(Pc, Nm, hand, nn_idx=nn_hand)
        assert torch.isnan(out[1, [r, r2, r3]]).all() and not torch.isnan(want).any()
        keep = torch.ones(3, N, dtype=torch.bool, device="cuda")
        keep[1, [r, r2, r3]] = False
        assert bits_equal(out[keep], want[keep])
