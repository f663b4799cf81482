"""CPU: the numpy restatements of tests/_aux_ref.py pinned to oracle/aux_oracle.py on inputs without ties or NaN (at the
oracle's own tolerance where the two do not state the same float32 operations), the float32 forms pinned to the float64
ones within the bounds the module derives, and the selection's total order on ties, +inf and NaN."""
import numpy as np
import pytest
import torch

from oracle import aux_oracle as A
from oracle import geoa3_oracle as O
from tests import _aux_ref as R
from tests import _normal_ref as NR

F = np.float32
U32 = R.U32


def _clouds(b, n, seed, noise=0.0):
    pc, nrm = O.make_synthetic_clouds(b, n, seed)
    if noise:
        pc = pc + torch.randn(b, 3, n, generator=torch.Generator().manual_seed(seed + 1)) * noise
    return pc, nrm


# ------------------------------------------------------------------ farthest point sampling
@pytest.mark.parametrize("n,m", [(37, 20), (300, 300), (1100, 64)])
def test_fps_is_the_oracle_bit_for_bit(n, m):
    pc, _ = _clouds(3, n, 400 + n)
    start = torch.tensor([0, n - 1, n // 3])
    want_pts, want_idx = A.farthest_points_sample(pc, m, start)
    for j in range(3):
        idx, pts = R.fps_sample(pc[j].numpy(), m, int(start[j]))
        assert np.array_equal(idx, want_idx[j].numpy())
        assert np.array_equal(pts.view(np.int32), want_pts[j].numpy().view(np.int32))
        # float64 picks the same points on a cloud without near-ties (no bound: an index is right or wrong) ...
        idx64, _ = R.fps_sample(pc[j].numpy(), m, int(start[j]), np.float64)
        assert np.array_equal(idx64, idx)
        # ... and a shorter run is a prefix of a longer one
        assert np.array_equal(R.fps_sample(pc[j].numpy(), 5, int(start[j]))[0], idx[:5])


def test_fps_clamps_the_start_and_repeats_index_zero_once_exhausted():
    pc = _clouds(1, 6, 7)[0][0].numpy()
    assert R.fps_sample(pc, 3, -4)[0][0] == 0 and R.fps_sample(pc, 3, 6)[0][0] == 5
    idx, pts = R.fps_sample(pc, 9, 2)
    assert sorted(idx[:6].tolist()) == list(range(6)) and idx[6:].tolist() == [0, 0, 0]
    assert np.array_equal(pts, pc[:, idx])


# ------------------------------------------------------------------ statistical outlier removal
@pytest.mark.parametrize("n,k", [(65, 1), (257, 5), (600, 64)])
def test_sor_statistic(n, k):
    """The oracle sums the K roots with torch.mean, in an order of its own: rtol 2e-6, the tolerance tests/test_gpu_aux.py
    holds the kernel to against the same oracle.  float32 against float64: |d32 - d64| <= (K + 6) u d64
    (R.sor_statistic_tol) -- per distance the difference and the added 1e-10 (2u on dx, so 4u + u on its square), two
    additions (2u): 7u on d, 3.5u + u after the root; K - 1 additions and the quotient: K u; 4.5 + K rounded up, and one
    spare u for the second order.  The k-th smallest of perturbed values moves by no more than the largest perturbation,
    so the choice of neighbours needs no term."""
    pc, _ = _clouds(2, n, 410 + n, noise=0.01)
    want = A.sor_statistic(pc, k).numpy()
    for j in range(2):
        d32 = R.sor_statistic(pc[j].numpy(), k)
        d64 = R.sor_statistic(pc[j].numpy(), k, np.float64)
        assert d32.dtype == F and d64.dtype == np.float64
        np.testing.assert_allclose(d32, want[j], rtol=2e-6, atol=0)
        err, tol = np.abs(d32.astype(np.float64) - d64), R.sor_statistic_tol(d64, k)
        print("sor_statistic n=%d k=%d: max err/tol %.3f" % (n, k, (err / tol).max()))
        assert (err <= tol).all()


def test_sor_statistic_coincident_points_and_a_lost_point():
    pc = _clouds(1, 40, 3)[0][0].numpy()
    pc[:, 10:20] = pc[:, 10:11]                                       # 10 coincident points, K = 4
    d = R.sor_statistic(pc, 4)
    root = np.sqrt((F(1e-10) * F(1e-10) + F(1e-10) * F(1e-10)) + F(1e-10) * F(1e-10))
    want = (((root + root) + root) + root) / F(4)                     # the dropped column is a genuine neighbour
    assert (d[10:20].view(np.int32) == want.view(np.int32)).all() and abs(float(want) - np.sqrt(3e-20)) < 1e-16
    bad = pc.copy()
    bad[1, 5] = np.nan
    got = R.sor_statistic(bad, 4)
    rest = np.delete(np.arange(40), 5)
    assert np.isnan(got[5]) and np.array_equal(got[rest].view(np.int32), R.sor_statistic(pc[:, rest], 4).view(np.int32))


@pytest.mark.parametrize("kind,drop,alpha,knn", [("outliers_fixNum", 128, 1.1, 2), ("outliers_fixNum", 1, 1.1, 16),
                                                 ("outliers_variance", 0, 1.1, 2), ("outliers_variance", 0, 0.3, 8),
                                                 ("outliers_variance", 0, -0.5, 8)])
def test_selection_is_the_oracle_without_ties(kind, drop, alpha, knn):
    pc, _ = _clouds(3, 700, 420, noise=0.01)
    for j in range(3):
        dis = A.sor_statistic(pc[j:j + 1], knn)[0].numpy()
        assert np.unique(dis).size == dis.size
        _, num, want = A.outlier_removal(pc[j:j + 1], kind, drop, alpha, knn)
        if kind == "outliers_fixNum":
            got = R.select_fixnum(dis, drop)
        else:
            mean, std = R.variance_stats(dis)
            got = R.select_variance(dis, F(mean), F(std), alpha)
            # the oracle's float32 statistics lie within an ulp or two of the float64 ones
            assert abs(float(torch.from_numpy(dis).mean()) - mean) <= 2 * R.ulp32(mean)
            assert abs(float(torch.from_numpy(dis).std()) - std) <= 2 * R.ulp32(std)
        assert got.tolist() == want.tolist() and len(got) == 700 - num


def test_selection_total_order():
    """finite < +inf < NaN, ties to the lower index, exactly N - drop_num kept (torch.topk promises no order among ties)."""
    inf, nan = np.inf, np.nan
    d = np.array([2.0, nan, 1.0, inf, 1.0, -0.0, 0.0, nan, inf, 1.0, -inf, -nan, -3.0, -inf], F)
    assert np.signbit(d[11]) and np.isnan(d[11])
    order = [10, 13, 12, 5, 6, 2, 4, 9, 0, 3, 8, 1, 7, 11]            # -inf, finite, +inf, NaN of either sign
    for drop in range(15):
        assert R.select_fixnum(d, drop).tolist() == sorted(order[:14 - drop])
    g = np.random.default_rng(5)
    ties = (g.integers(0, 2, 320)).astype(F)
    zeros, ones = np.nonzero(ties == 0)[0], np.nonzero(ties == 1)[0]
    assert 100 < len(zeros) < 200                                    # every 0, then the lowest-index 1s
    want = np.sort(np.concatenate([zeros, ones[:200 - len(zeros)]]))
    assert np.array_equal(R.select_fixnum(ties, 120), want)


def test_variance_selection_edges():
    d = np.full(50, 0.37, F)
    mean, std = R.variance_stats(d)
    assert mean == float(F(0.37)) and std == 0.0
    for alpha in (1.1, 0.3, -0.5):
        assert R.select_variance(d, F(mean), F(std), alpha).size == 0
    d[7] = np.nan
    mean, std = R.variance_stats(d)
    assert np.isnan(mean) and np.isnan(std) and R.select_variance(d, F(mean), F(std), 1.1).size == 0


# ------------------------------------------------------------------ smoothness
@pytest.mark.parametrize("k", [4, 16])
def test_smoothness(k):
    """The oracle (float32 normals of np.cov / eigh, torch sums) against the float64 restatement on the float64 normals of
    tests/_normal_ref.py: rtol 5e-5, the tolerance tests/test_gpu_aux.py uses for the same pair.  float32 against
    float64: C u mag with C = R.smoothness_c(k)."""
    pc, _ = _clouds(2, 300, 430, noise=0.005)
    for j in range(2):
        p = pc[j].numpy()
        table = NR.knn_table(p, k + 1)
        nrm, _ = NR.estimate_normal(p, table)
        evecs = np.zeros((3, 3, 300))
        evecs[0] = nrm
        s64, mag = R.smoothness(p, table, evecs)
        np.testing.assert_allclose(s64.max(), float(A.smoothness(pc[j].t().contiguous(), k, k)), rtol=5e-5)
        e32 = evecs.astype(F)
        s32, _ = R.smoothness(p, table, e32, F)
        s64, mag = R.smoothness(p, table, e32)                       # the same float32 normals on both sides
        err, tol = np.abs(s32.astype(np.float64) - s64), R.smoothness_c(k) * U32 * mag
        print("smoothness k=%d: max err/tol %.3f" % (k, (err / tol).max()))
        assert s32.dtype == F and (err <= tol).all() and (mag >= s64 * (1 - 1e-12)).all()


# ------------------------------------------------------------------ tangent-plane jitter
def test_perp_jitter():
    """The oracle's last line on the oracle's own eigenvectors: the same float32 operations, the same bits."""
    pc, _ = _clouds(2, 200, 440)
    g = torch.Generator().manual_seed(9)
    a1, a2 = torch.randn(2, 200, generator=g) * 0.04, torch.randn(2, 200, generator=g) * 0.04
    want, _, v = A.estimate_perpendicular(pc, 12, a1, a2, clip=0.05)
    assert (want.abs() == 0.05).any() or (want.abs() > 0.05).any()   # some product clamps
    for j in range(2):
        evecs = v[j].permute(2, 1, 0).contiguous().numpy()           # [n,xyz,e] -> [e,xyz,n]
        got = R.perp_jitter(evecs, a1[j].numpy(), a2[j].numpy(), 0.05)
        assert got.dtype == F and np.array_equal(got.view(np.int32), want[j].numpy().view(np.int32))
        # float64: a product (u) and the sum (u) of two clamped terms
        g64 = R.perp_jitter(evecs, a1[j].numpy(), a2[j].numpy(), float(F(0.05)), np.float64)
        t = np.abs(evecs[2] * a1[j].numpy()[None]) + np.abs(evecs[1] * a2[j].numpy()[None])
        assert (np.abs(got - g64) <= 2 * U32 * np.minimum(t, 0.1) + 1e-45).all()
    e = np.ones((3, 3, 4), F)
    e[2, 1, 2] = np.nan
    out = R.perp_jitter(e, np.array([0.01, 9.0, 0.01, -0.0], F), np.array([-9.0, 0.0, 0.01, np.nan], F), 0.05)
    assert np.array_equal(np.isnan(out), [[0, 0, 0, 1], [0, 0, 1, 1], [0, 0, 0, 1]])
    assert out[0, 0] == F(0.01) - F(0.05) and out[0, 1] == F(0.05)


# ------------------------------------------------------------------ normals of moved points
@pytest.mark.parametrize("k", [1, 3, 16])
def test_knn_normal(k):
    """rtol 2e-6 / atol 2e-7: the tolerance tests/test_gpu_aux.py holds the kernel to against the same oracle."""
    ori, nrm = _clouds(2, 400, 450)
    adv = ori[:, :, :150] + torch.randn(2, 3, 150, generator=torch.Generator().manual_seed(2)) * 0.02
    adv[:, :, :20] = ori[:, :, :20]
    for j in range(2):
        want = A.estimate_normal_via_ori_normal(adv[j:j + 1], ori[j:j + 1], nrm[j:j + 1], k)[0].numpy()
        d, i = O.knn_points(adv[j:j + 1].permute(0, 2, 1), ori[j:j + 1].permute(0, 2, 1), k)
        d, i = d[0].numpy(), i[0].numpy()
        o64, tol, moved = R.knn_normal(d, i, nrm[j].numpy())
        o32, _, _ = R.knn_normal(d, i, nrm[j].numpy(), F)
        assert not moved[:20].any() and moved[20:].all()
        np.testing.assert_allclose(o64, want, rtol=2e-6, atol=2e-7)
        assert np.array_equal(o32[:, :20].view(np.int32), nrm[j].numpy()[:, i[:20, 0]].view(np.int32))
        err = np.abs(o32.astype(np.float64) - o64)
        print("knn_normal k=%d: max err/tol %.3f" % (k, (err[:, moved] / tol[:, moved]).max()))
        assert (err <= tol).all() and (tol[:, ~moved] == 0).all()
