"""GPU: every kernel of geoa3_amd/csrc/geom_aux.hip that tests/test_gpu_normal.py does not hold alone -- fps_sample,
sor_statistic, sor_select, smoothness, perp_jitter, knn_normal -- called through the C ABI on inputs the test builds itself
(tables, eigenvectors and `dis` arrays included), against the numpy restatements of tests/_aux_ref.py: bit for bit where
the kernel's chain is reproducible, within a bound counted from its operations where a product may fuse into a sum.
Then the file's two rules ("NaN rule"): a NaN stays a NaN, and a table entry outside [0,N) is never read.
B = 3 with a different cloud per instance unless a case says otherwise."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _aux_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
U32 = R.U32
NAN = float("nan")
OK, EINVAL, ENOSUPPORT = 0, -1, -3
POISON_I = -77


@pytest.fixture(scope="module")
def lib():
    from geoa3_amd import _lib
    assert torch.cuda.is_available(), "needs the MI355X"
    return _lib.load()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda().contiguous()


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(got, want):
    """the same bits, a NaN for a NaN (its payload is not compared)"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and np.array_equal(
        np.where(gn, F(0), got).view(np.int32), np.where(wn, F(0), want).view(np.int32))


def _poisoned_f(t):
    return bool(torch.isnan(t).all())


def _poisoned_i(t):
    return bool((t == POISON_I).all())


# ====================================================================================== geoa3_fps_sample
FPS_N = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384]


def _fps(lib, pc, m, start, with_pts=True):
    b, _, n = pc.shape
    idx = torch.full((b, m), POISON_I, dtype=torch.int32, device="cuda")
    pts = torch.full((b, 3, m), NAN, device="cuda") if with_pts else None
    rc = lib.geoa3_fps_sample(_p(pc), b, n, m, _p(start), _p(idx), _p(pts), _stream())
    return rc, idx, pts


@pytest.mark.parametrize("n", FPS_N)
def test_fps_sample_bit_for_bit(lib, n):
    """2 points per thread up to 1024, 4 to 2048, 8 to 4096, 16 to 8192 in LDS; the register form from 8193 to 16384.
    m = 1 (no round), 2, 40; for n <= 65 also m = n and n + 3: the exhausted cloud has every distance 0 and picks 0."""
    g = np.random.default_rng(1000 + n)
    pc = g.standard_normal((3, 3, n)).astype(F)
    start = g.integers(0, n, 3).astype(np.int32)
    ms = [1, 2, 40] + ([n, n + 3] if n <= 65 else [])
    ref = [R.fps_sample(pc[j], max(ms), int(start[j])) for j in range(3)]
    want_idx, want_pts = np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])
    if n <= 65:
        assert (want_idx[:, n:] == 0).all() and (np.sort(want_idx[:, :n], axis=1) == np.arange(n)).all()
    dpc, dstart = _dev(pc), _dev(start)
    for m in ms:
        rc, idx, pts = _fps(lib, dpc, m, dstart)
        assert rc == OK
        assert np.array_equal(_np(idx), want_idx[:, :m]), (n, m)
        assert np.array_equal(_np(pts).view(np.int32), want_pts[:, :, :m].view(np.int32)), (n, m)
    rc, idx, _ = _fps(lib, dpc, 40, dstart, with_pts=False)          # pts == NULL
    assert rc == OK and np.array_equal(_np(idx), want_idx[:, :40])


@pytest.mark.parametrize("n", [65, 8193])
def test_fps_sample_clamps_the_start(lib, n):
    g = np.random.default_rng(n)
    pc = g.standard_normal((3, 3, n)).astype(F)
    start = np.array([-5, n, 2 ** 31 - 1], np.int32)
    rc, idx, pts = _fps(lib, _dev(pc), 6, _dev(start))
    assert rc == OK
    for j, first in enumerate([0, n - 1, n - 1]):
        want_idx, want_pts = R.fps_sample(pc[j], 6, int(start[j]))
        assert want_idx[0] == first
        assert np.array_equal(_np(idx)[j], want_idx) and np.array_equal(_np(pts)[j].view(np.int32), want_pts.view(np.int32))


def test_fps_sample_refuses_more_than_16384_points(lib):
    pc = torch.zeros(1, 3, 16385, device="cuda")
    rc, idx, pts = _fps(lib, pc, 4, torch.zeros(1, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert rc == ENOSUPPORT and _poisoned_i(idx) and _poisoned_f(pts)


@pytest.mark.parametrize("n,copies,want", [(2048, (511, 512, 1024), 511), (2048, (63, 64), 63), (2048, (1535, 1536), 1535),
                                           (8193, (1023, 1024, 8192), 1023)])
def test_fps_sample_ties_go_to_the_lowest_index(lib, n, copies, want):
    """A cloud of copies of two locations A and B, started at an A copy: every B copy is at the same distance, the lowest
    index has to win round 1, and after it every distance is 0, so round 2 returns to index 0.  n = 2048 runs 512 threads
    with 4 points each (point i in thread i % 512, slot i / 512): 511 is the last lane of the last wavefront in slot 0
    against lane 0 in slots 1 and 2; 63 | 64 is the last lane of wavefront 0 against the first of wavefront 1; 1535 | 1536
    slot 2's last lane against slot 3's first.  n = 8193 is the register form (1024 threads, 16 slots)."""
    a = np.array([[0.25, -0.5, 0.125], [1.5, 0.75, -2.0], [-0.375, 0.0, 3.0]], F)
    b = np.array([[1.0, 2.0, -1.0], [-0.5, 0.25, 0.5], [0.0, -1.25, 0.75]], F)
    pc = np.repeat(a[:, :, None], n, axis=2)
    pc[:, :, list(copies)] = b[:, :, None]
    rc, idx, pts = _fps(lib, _dev(pc), 3, torch.zeros(3, dtype=torch.int32, device="cuda"))
    assert rc == OK
    assert _np(idx).tolist() == [[0, want, 0]] * 3
    for j in range(3):
        ref_idx, ref_pts = R.fps_sample(pc[j], 3, 0)
        assert ref_idx.tolist() == [0, want, 0] and np.array_equal(_np(pts)[j].view(np.int32), ref_pts.view(np.int32))


# ====================================================================================== geoa3_sor_statistic
def _sor_stat(lib, pc, k):
    b, _, n = pc.shape
    dis = torch.full((b, n), NAN, device="cuda")
    rc = lib.geoa3_sor_statistic(_p(pc), b, n, k, _p(dis), _stream())
    return rc, dis


@pytest.mark.parametrize("n,k", [(2, 1), (65, 1), (65, 64), (255, 5), (256, 5), (257, 5), (600, 64)])
def test_sor_statistic_bit_for_bit(lib, n, k):
    """((p_j - p_i) + 1e-10)^2 summed (x + y) + z under contract(off), the K+1 smallest ascending, the first dropped,
    sqrtf of each, a sequential sum, / (float)K: no product feeds a sum that could fuse, roots and the quotient are
    correctly rounded.  256 rows per workgroup: one, one and a row, two; K = 64 at n = 600 is the opt-in LDS size."""
    g = np.random.default_rng(2000 + 7 * n + k)
    pc = (g.standard_normal((3, 3, n)) * np.array([0.3, 1.0, 4.0])[:, None, None]).astype(F)
    rc, dis = _sor_stat(lib, _dev(pc), k)
    assert rc == OK
    got = _np(dis)
    for j in range(3):
        want = R.sor_statistic(pc[j], k)
        assert np.isfinite(want).all() and _same(got[j], want), (n, k, j, np.abs(got[j] - want).max())


def test_sor_statistic_coincident_points(lib):
    """10 coincident points, K = 4: the dropped column is one of the copies, the four kept are genuine neighbours at
    sqrt(3e-20), as the reference's [:, :, 1:] leaves them."""
    g = np.random.default_rng(3)
    pc = g.standard_normal((3, 3, 40)).astype(F)
    pc[:, :, 10:20] = pc[:, :, 10:11]
    rc, dis = _sor_stat(lib, _dev(pc), 4)
    assert rc == OK
    got = _np(dis)
    for j in range(3):
        want = R.sor_statistic(pc[j], 4)
        assert abs(float(want[10]) - np.sqrt(3e-20)) < 1e-16 and _same(got[j], want)


def test_sor_statistic_nonfinite_point(lib):
    """The point itself is NaN; every other row keeps the bits it has on the cloud without that point."""
    g = np.random.default_rng(4)
    pc = g.standard_normal((3, 3, 257)).astype(F)
    bad = pc.copy()
    bad[1, 1, 100] = np.nan
    bad[2, 2, 7] = np.inf
    rc, dis = _sor_stat(lib, _dev(bad), 5)
    assert rc == OK
    got = _np(dis)
    assert _same(got[0], R.sor_statistic(pc[0], 5))
    for j, lost in ((1, 100), (2, 7)):
        rest = np.delete(np.arange(257), lost)
        assert np.isnan(got[j, lost])
        assert _same(got[j, rest], R.sor_statistic(pc[j][:, rest], 5))
        assert _same(got[j], R.sor_statistic(bad[j], 5))


@pytest.mark.parametrize("n,k", [(40, 40), (100, 65), (40, 0)])
def test_sor_statistic_refuses(lib, n, k):
    rc, dis = _sor_stat(lib, torch.zeros(3, 3, n, device="cuda"), k)
    torch.cuda.synchronize()
    assert rc == EINVAL and _poisoned_f(dis)


# ====================================================================================== geoa3_sor_select
SEL_N = [2, 63, 64, 65, 1023, 1024, 1025, 2049, 3000]


def _select(lib, dis, mode, drop, alpha, with_stats=True):
    b, n = dis.shape
    idx = torch.full((b, n), POISON_I, dtype=torch.int32, device="cuda")
    cnt = torch.full((b,), POISON_I, dtype=torch.int32, device="cuda")
    stats = torch.full((b, 2), NAN, device="cuda") if with_stats else None
    rc = lib.geoa3_sor_select(_p(dis), b, n, mode, drop, ctypes.c_float(alpha), _p(idx), _p(cnt), _p(stats), _stream())
    return rc, idx, cnt, stats


def _check_kept(idx, cnt, j, kept):
    n = idx.shape[1]
    assert int(cnt[j]) == len(kept)
    assert np.array_equal(idx[j, :len(kept)], kept) and (idx[j, len(kept):] == -1).all(), (j, n)


def _dis_cases(n, seed):
    g = np.random.default_rng(seed)
    rand = (np.abs(g.standard_normal((3, n))) + 0.1).astype(F)
    levels = np.array([0.0, -0.0, 0.25, 1.0, 3.0, -2.0], F)          # five values, zero under both signs
    ties = levels[g.integers(0, 6, (3, n))]
    wild = rand.copy()
    wild[g.random((3, n)) < 0.2] = np.inf
    wild[g.random((3, n)) < 0.2] = np.nan
    wild[0, 0], wild[1, n - 1], wild[2, n // 2] = np.nan, np.nan, np.inf   # at least one of each, whatever n
    wild[0, n - 1], wild[1, 0] = np.inf, 0.5
    if n > 2:                                                        # -inf is the lowest key; a NaN with its sign set is a NaN
        wild[:, 1] = [-np.inf, np.array([0xffc00001], np.uint32).view(F)[0], -np.inf]
        wild[2, 2] = np.array([0xff800001], np.uint32).view(F)[0]    # ... a signalling one too
    return {"random": rand, "ties": ties, "inf_nan": wild}


@pytest.mark.parametrize("n", SEL_N)
def test_sor_select_fixnum_exact(lib, n):
    """Mode 0 against the stable sort of tests/_aux_ref.py (finite, +inf, NaN; ties to the lower index): always
    count == n - drop_num, ascending indices, a tail of -1.  1024 elements per pass of the compaction loop: one pass,
    one and an element, three."""
    for kind, dis in _dis_cases(n, 3000 + n).items():
        ddis = _dev(dis)
        for drop in sorted({0, 1, n // 3, n - 1, n}):
            rc, idx, cnt, _ = _select(lib, ddis, 0, drop, 1.1)
            assert rc == OK
            idx, cnt = _np(idx), _np(cnt)
            for j in range(3):
                kept = R.select_fixnum(dis[j], drop)
                assert len(kept) == n - drop and (np.diff(kept) > 0).all()
                _check_kept(idx, cnt, j, kept)


def _check_variance(lib, dis, alpha):
    b, n = dis.shape
    rc, idx, cnt, stats = _select(lib, _dev(dis), 1, 0, alpha)
    assert rc == OK
    idx, cnt, stats = _np(idx), _np(cnt), _np(stats)
    for j in range(b):
        mean, std = R.variance_stats(dis[j])
        print("n=%d alpha=%g: mean %.9g (float64 %.17g), std %.9g (float64 %.17g)" % (
            n, alpha, stats[j, 0], mean, stats[j, 1], std))
        # the statistics are held to float64 (1 ulp of float32 around the rounded value) ...
        assert abs(float(stats[j, 0]) - float(F(mean))) <= R.ulp32(mean)
        assert abs(float(stats[j, 1]) - float(F(std))) <= R.ulp32(std)
        # ... and the selection to the statistics the kernel itself reports: exactly, whatever lies near the threshold
        _check_kept(idx, cnt, j, R.select_variance(dis[j], stats[j, 0], stats[j, 1], alpha))
    return idx, cnt


@pytest.mark.parametrize("n", SEL_N)
def test_sor_select_variance(lib, n):
    dis = _dis_cases(n, 4000 + n)["random"]
    for alpha in (1.1, 0.3, -0.5):
        idx, cnt = _check_variance(lib, dis, alpha)
    rc, idx2, cnt2, _ = _select(lib, _dev(dis), 1, 0, -0.5, with_stats=False)        # stats == NULL
    assert rc == OK and np.array_equal(_np(idx2), idx) and np.array_equal(_np(cnt2), cnt)


def test_sor_select_variance_opt_in_lds_size(lib):
    g = np.random.default_rng(5)
    dis = (np.abs(g.standard_normal((1, 38400))) + 0.1).astype(F)
    _, cnt = _check_variance(lib, dis, 1.1)
    assert 0 < int(cnt[0]) < 38400


def test_sor_select_variance_keeps_nothing_of_a_flat_or_nan_dis(lib):
    dis = np.stack([np.full(1025, 0.37, F), np.full(1025, 3.0, F), np.full(1025, 1e-3, F)])
    for alpha in (1.1, 0.3, -0.5):
        rc, idx, cnt, stats = _select(lib, _dev(dis), 1, 0, alpha)
        assert rc == OK and (_np(cnt) == 0).all() and (_np(idx) == -1).all()
        assert np.array_equal(_np(stats), np.stack([dis[:, 0], np.zeros(3, F)], axis=1))   # std is exactly 0
    g = np.random.default_rng(6)
    dis = (np.abs(g.standard_normal((3, 1025))) + 0.1).astype(F)
    dis[1, 300] = np.nan
    rc, idx, cnt, stats = _select(lib, _dev(dis), 1, 0, 1.1)
    idx, cnt, stats = _np(idx), _np(cnt), _np(stats)
    assert rc == OK and cnt[1] == 0 and (idx[1] == -1).all() and np.isnan(stats[1]).all()
    for j in (0, 2):
        _check_kept(idx, cnt, j, R.select_variance(dis[j], stats[j, 0], stats[j, 1], 1.1))
        assert 0 < cnt[j] < 1025


@pytest.mark.parametrize("n,mode,drop,want", [(38401, 1, 0, ENOSUPPORT), (38401, 0, 5, ENOSUPPORT), (1, 0, 0, EINVAL),
                                              (1, 1, 0, EINVAL), (64, 0, 65, EINVAL), (64, 0, -1, EINVAL),
                                              (64, 2, 0, EINVAL)])
def test_sor_select_refuses(lib, n, mode, drop, want):
    rc, idx, cnt, stats = _select(lib, torch.ones(1, n, device="cuda"), mode, drop, 1.1)
    torch.cuda.synchronize()
    assert rc == want and _poisoned_i(idx) and _poisoned_i(cnt) and _poisoned_f(stats)


# ====================================================================================== geoa3_smoothness
def _smooth(lib, pc, table, evecs, with_pp=True):
    b, _, n = pc.shape
    pp = torch.full((b, n), NAN, device="cuda") if with_pp else None
    out = torch.full((b,), NAN, device="cuda")
    rc = lib.geoa3_smoothness(_p(pc), _p(table), _p(evecs), b, n, table.shape[2], _p(pp), _p(out), _stream())
    return rc, pp, out


def _smooth_inputs(n, k, seed):
    g = np.random.default_rng(seed)
    pc = g.standard_normal((3, 3, n)).astype(F)
    table = g.integers(0, n, (3, n, k + 1)).astype(np.int32)
    table[:, :, 0] = np.arange(n)
    ev = g.standard_normal((3, 3, 3, n))
    evecs = (ev / np.linalg.norm(ev, axis=2, keepdims=True)).astype(F)
    return pc, table, evecs


@pytest.mark.parametrize("n,k", [(1, 1)] + [(n, k) for n in (63, 64, 65, 255, 256, 257, 1000) for k in (1, 16)])
def test_smoothness_per_point_and_its_maximum(lib, n, k):
    """per_point against float64: |got - want| <= C u (1/k) sum_m sum_c |d_c n_c| with C = k + 5 -- per term the three
    differences (u each), three products (u each; fewer when fused) and two additions (u each) are 4u on sum_c |d_c n_c|;
    k - 1 additions of the terms; the quotient; one spare u for the second order (tests/_aux_ref.smoothness_c).
    out[b] is the maximum of the per_point the kernel wrote, bit for bit: a maximum rounds nothing.  256 rows per
    workgroup.  n = 1: the only neighbour there is is the point itself, s = 0 exactly."""
    pc, table, evecs = _smooth_inputs(n, k, 5000 + 31 * n + k)
    dpc, dtab, dev = _dev(pc), _dev(table), _dev(evecs)
    rc, pp, out = _smooth(lib, dpc, dtab, dev)
    assert rc == OK
    pp, out = _np(pp), _np(out)
    for j in range(3):
        want, mag = R.smoothness(pc[j], table[j], evecs[j])
        err, tol = np.abs(pp[j].astype(np.float64) - want), R.smoothness_c(k) * U32 * mag
        print("smoothness n=%d k=%d cloud %d: max err %.3e, max err/bound %.3f" % (
            n, k, j, err.max(), (err / np.where(tol > 0, tol, 1.0)).max()))
        assert (err <= tol).all()
    assert np.array_equal(out.view(np.int32), pp.max(axis=1).view(np.int32))
    rc, _, out2 = _smooth(lib, dpc, dtab, dev, with_pp=False)        # per_point == NULL
    assert rc == OK and np.array_equal(_np(out2).view(np.int32), out.view(np.int32))


@pytest.mark.parametrize("n", [257, 1000])
def test_smoothness_finds_a_planted_maximum(lib, n):
    """Normal (0,0,1), every point in the plane z = 0 but one, raised by h: that row is h exactly (16 terms of h, / 16),
    the rows that do not list it are 0.  The raised point sits in the first and last lane of a wavefront, of a workgroup
    and of the cloud."""
    k = 16
    g = np.random.default_rng(n)
    h = np.array([0.375, 1.5, 0.046875], F)
    evecs = np.zeros((3, 3, 3, n), F)
    evecs[:, 0, 2] = 1.0
    for star in (0, 63, 64, 255, 256, n - 1):
        pc = g.standard_normal((3, 3, n)).astype(F)
        pc[:, 2] = 0.0
        pc[:, 2, star] = h
        table = ((np.arange(n)[:, None] + np.arange(k + 1)[None, :]) % n).astype(np.int32)
        table[:, 1:][table[:, 1:] == star] = (star + n // 2) % n     # no other row lists the raised point
        table = np.repeat(table[None], 3, axis=0)
        rc, pp, out = _smooth(lib, _dev(pc), _dev(table), _dev(evecs))
        assert rc == OK
        pp, out = _np(pp), _np(out)
        want = np.zeros((3, n), F)
        want[:, star] = h
        assert np.array_equal(pp.view(np.int32), want.view(np.int32)), star
        assert np.array_equal(out.view(np.int32), h.view(np.int32)), star


def test_smoothness_keeps_nan(lib):
    """A NaN coordinate: per_point is NaN in exactly the rows that list the point (its own row lists it in column 0), out
    is NaN for that cloud and keeps its bits for the others."""
    pc, table, evecs = _smooth_inputs(257, 16, 77)
    rc, pp0, out0 = _smooth(lib, _dev(pc), _dev(table), _dev(evecs))
    bad = pc.copy()
    bad[1, 0, 130] = np.nan
    rc1, pp, out = _smooth(lib, _dev(bad), _dev(table), _dev(evecs))
    assert rc == OK and rc1 == OK
    pp0, out0, pp, out = _np(pp0), _np(out0), _np(pp), _np(out)
    lists = (table[1] == 130).any(axis=1)
    assert lists[130] and 2 <= lists.sum() < 257 and np.isfinite(pp0).all()
    assert np.array_equal(np.isnan(pp[1]), lists) and np.isnan(out[1])
    want = pp0.copy()
    want[1, lists] = np.nan
    assert _same(pp, want) and _same(out, np.array([out0[0], np.nan, out0[2]], F))
    rc, _, out2 = _smooth(lib, _dev(bad), _dev(table), _dev(evecs), with_pp=False)
    assert rc == OK and _same(_np(out2), out)
    # ... and a NaN normal poisons its own row alone
    ebad = evecs.copy()
    ebad[2, 0, 1, 64] = np.nan
    rc, pp, out = _smooth(lib, _dev(pc), _dev(table), _dev(ebad))
    want = pp0.copy()
    want[2, 64] = np.nan
    assert rc == OK and _same(_np(pp), want) and _same(_np(out), np.array([out0[0], out0[1], np.nan], F))


# ====================================================================================== geoa3_perp_jitter
def _jitter(lib, evecs, a1, a2, clip):
    b, n = a1.shape
    out = torch.full((b, 3, n), NAN, device="cuda")
    rc = lib.geoa3_perp_jitter(_p(evecs), _p(a1), _p(a2), b, n, ctypes.c_float(clip), _p(out), _stream())
    return rc, out


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_perp_jitter_bit_for_bit(lib, n):
    """clamp(E[2] a1) + clamp(E[1] a2): each product feeds a clamp, not the sum, so nothing can fuse.  Planted per
    instance (element 0, so n = 1 has them too): a product exactly at +clip and one at -clip (0.5 * fl(0.1) is fl(0.05)),
    aux = +0 and -0, aux far beyond the clamp; NaN eigenvector components and NaN aux from element 200 on."""
    g = np.random.default_rng(6000 + n)
    ev = g.standard_normal((3, 3, 3, n))
    evecs = (ev / np.linalg.norm(ev, axis=2, keepdims=True)).astype(F)
    a1, a2 = (g.standard_normal((3, n)) * 0.04).astype(F), (g.standard_normal((3, n)) * 0.04).astype(F)
    clip = 0.05
    evecs[0, 2, :, 0], a1[0, 0] = [0.5, -0.5, 0.25], 0.1             # +clip, -clip, inside
    evecs[0, 1, :, 0], a2[0, 0] = [-0.5, 0.5, 1.0], 0.1              # -clip, +clip, beyond
    a1[1, 0], a2[1, 0] = 0.0, -0.0
    a1[2, 0], a2[2, 0] = 9.0, -1e30
    if n > 200:
        evecs[0, 2, 1, 200] = np.nan                                 # one component of the first term
        evecs[1, 1, 0, 201] = np.nan                                 # ... of the second
        a1[2, 202] = np.nan                                          # a whole point
        a2[0, 203] = np.nan
        evecs[1, 0, :, 204] = np.nan                                 # the eigenvector the kernel does not read
    rc, out = _jitter(lib, _dev(evecs), _dev(a1), _dev(a2), clip)
    assert rc == OK
    got = _np(out)
    want = np.stack([R.perp_jitter(evecs[j], a1[j], a2[j], clip) for j in range(3)])
    assert np.array_equal(want[0, :, 0], np.array([0.0, 0.0, F(0.25) * F(0.1) + F(0.05)], F))
    assert (want[1, :, 0] == 0).all() and (np.abs(want[2, :, 0]) <= 2 * F(clip)).all()
    if n > 200:
        nan = np.zeros((3, 3, n), bool)
        nan[0, 1, 200] = nan[1, 0, 201] = True
        nan[2, :, 202] = nan[0, :, 203] = True
        assert np.array_equal(np.isnan(want), nan)
    else:
        assert np.isfinite(want).all()
    assert _same(got, want), np.argwhere(got.view(np.int32) != want.view(np.int32))[:5]


@pytest.mark.parametrize("clip", [0.0, -0.05, NAN])
def test_perp_jitter_refuses(lib, clip):
    z = torch.zeros(3, 64, device="cuda")
    rc, out = _jitter(lib, torch.zeros(3, 3, 3, 64, device="cuda"), z, z, clip)
    torch.cuda.synchronize()
    assert rc == EINVAL and _poisoned_f(out)


# ====================================================================================== geoa3_knn_normal
def _knn_normal(lib, knn_d, knn_i, normals):
    b, nq, k = knn_i.shape
    out = torch.full((b, 3, nq), NAN, device="cuda")
    rc = lib.geoa3_knn_normal(_p(knn_d), _p(knn_i), _p(normals), b, nq, normals.shape[2], k, _p(out), _stream())
    return rc, out


def _knn_normal_inputs(nq, k, seed):
    """Random tables and unit normals over nr = nq + 40 points, with planted rows.  The last three normals are v, -v and 0,
    so a row that alternates between the first two (and ends on the third when k is odd) cancels exactly."""
    g = np.random.default_rng(seed)
    nr = nq + 40
    nm = g.standard_normal((3, 3, nr))
    nm = (nm / np.linalg.norm(nm, axis=1, keepdims=True)).astype(F)
    nm[:, :, nr - 2] = -nm[:, :, nr - 3]
    nm[:, :, nr - 1] = 0.0
    knn_i = g.integers(0, nr - 3, (3, nq, k)).astype(np.int32)
    knn_d = (np.sort(g.random((3, nq, k)), axis=2) + 1e-3).astype(F)
    cancel = np.array([nr - 3, nr - 2] * (k // 2) + [nr - 1] * (k % 2), np.int32)
    below = np.nextafter(R.MOVED, F(0))
    plant = {}                                                       # (instance, row) -> kind
    if nq == 1:
        plant = {(0, 0): "at", (1, 0): "below", (2, 0): "cancel"}
    else:
        for j in range(3):
            plant.update({(j, 0 + j): "at", (j, 5 + j): "below", (j, 10 + j): "zero", (j, nq - 1 - j): "cancel"})
    for (j, row), kind in plant.items():
        if kind == "cancel":
            knn_i[j, row] = cancel
        else:
            knn_d[j, row, 0] = {"at": R.MOVED, "below": below, "zero": 0.0}[kind]
    return knn_d, knn_i, nm, plant


@pytest.mark.parametrize("k", [1, 3, 64])
@pytest.mark.parametrize("nq", [1, 255, 257])
def test_knn_normal(lib, nq, k):
    """Unmoved rows (knn_d[..., 0] < fl32(1e-6): the float32 just below it, and 0) copy the nearest point's normal bit
    for bit; exactly fl32(1e-6) averages.  Averaged rows against float64 within the bound of tests/_aux_ref.knn_normal:
    (K + 2) u on the mean, 6 u on the normalisation, scaled by 1 / |mean normal| -- the sum of squares may fuse, so no
    bits are claimed.  A row whose K normals cancel exactly is exactly 0."""
    knn_d, knn_i, nm, plant = _knn_normal_inputs(nq, k, 7000 + 13 * nq + k)
    rc, out = _knn_normal(lib, _dev(knn_d), _dev(knn_i), _dev(nm))
    assert rc == OK
    got = _np(out)
    for j in range(3):
        want, tol, moved = R.knn_normal(knn_d[j], knn_i[j], nm[j])
        for (jj, row), kind in plant.items():
            if jj == j:
                assert moved[row] == (kind in ("at", "cancel")), (row, kind)
                if kind == "cancel":
                    assert (want[:, row] == 0).all() and (got[j][:, row] == 0).all()
        err = np.abs(got[j].astype(np.float64) - want)
        print("knn_normal nq=%d k=%d cloud %d: max err %.3e, max err/bound %.3f" % (
            nq, k, j, err.max(), (err / np.where(tol > 0, tol, 1.0)).max()))
        assert (err <= tol).all(), np.argwhere(err > tol)[:5]
        copied = ~moved
        assert np.array_equal(got[j][:, copied].view(np.int32), nm[j][:, knn_i[j][copied, 0]].view(np.int32))


# ====================================================================================== the index rule
BAD_N, BAD_K1 = 257, 9


def _bad_tables(nrows, n, cols, seed):
    """(a clean table [3,nrows,cols] into clouds of n points, the same with -1 and n planted in clouds 0 and 2 -- cloud 1
    stays clean --, bool [3,nrows]: the rows that hold one)"""
    g = np.random.default_rng(seed)
    table = np.stack([np.stack([g.permutation(n)[:cols] for _ in range(nrows)]) for _ in range(3)]).astype(np.int32)
    bad = table.copy()
    rows = np.zeros((3, nrows), bool)
    for j, row, col, value in ((0, 5, min(3, cols - 1), -1), (0, 64, cols - 1, n), (2, nrows - 1, cols - 1, -1),
                               (2, 128, 0, n), (2, 255, 0, -1)):
        bad[j, row, col] = value
        rows[j, row] = True
    return table, bad, rows


def _expect_rows(got, clean, rows):
    """NaN in every output of the flagged rows ([..., n] layout per cloud), the clean run's bits everywhere else"""
    want = clean.copy()
    for j in range(3):
        want[j][..., rows[j]] = np.nan
    assert np.isfinite(clean).all()
    assert _same(got, want), np.argwhere(np.isnan(got) != np.isnan(want))[:5]


def test_index_rule_local_frames_and_estimate_normal(lib):
    """A row that holds -1 or N, in column 0 or in a neighbour column, is NaN in evals, evecs and both orientations of the
    normal; every other row has the bits of the run on the clean table."""
    n, k1 = BAD_N, BAD_K1
    pc = np.random.default_rng(81).standard_normal((3, 3, n)).astype(F)
    table, bad, rows = _bad_tables(n, n, k1, 82)
    table[:, :, 0] = np.arange(n)
    bad[:, :, 0] = np.where(rows & ((bad[:, :, 0] < 0) | (bad[:, :, 0] >= n)), bad[:, :, 0], np.arange(n))
    dpc = _dev(pc)

    def frames(t):
        evals, evecs = torch.full((3, 3, n), NAN, device="cuda"), torch.full((3, 3, 3, n), NAN, device="cuda")
        assert lib.geoa3_local_frames(_p(dpc), _p(t), 3, n, k1, _p(evals), _p(evecs), _stream()) == OK
        return _np(evals), _np(evecs)

    def normal(t, orient):
        out = torch.full((3, 3, n), NAN, device="cuda")
        assert lib.geoa3_estimate_normal(_p(dpc), _p(t), 3, n, k1, orient, _p(out), _stream()) == OK
        return _np(out)

    dclean, dbad = _dev(table), _dev(bad)
    (w0, v0), (w1, v1) = frames(dclean), frames(dbad)
    _expect_rows(w1, w0, rows)
    _expect_rows(v1, v0, rows)
    for orient in (0, 1):
        _expect_rows(normal(dbad, orient), normal(dclean, orient), rows)


def test_index_rule_smoothness(lib):
    pc, _, evecs = _smooth_inputs(BAD_N, BAD_K1 - 1, 83)
    table, bad, rows = _bad_tables(BAD_N, BAD_N, BAD_K1, 84)
    rc0, pp0, out0 = _smooth(lib, _dev(pc), _dev(table), _dev(evecs))
    rc1, pp1, out1 = _smooth(lib, _dev(pc), _dev(bad), _dev(evecs))
    assert rc0 == OK and rc1 == OK
    _expect_rows(_np(pp1), _np(pp0), rows)
    out0 = _np(out0)
    assert _same(_np(out1), np.array([np.nan, out0[1], np.nan], F))
    rc, _, out2 = _smooth(lib, _dev(pc), _dev(bad), _dev(evecs), with_pp=False)
    assert rc == OK and _same(_np(out2), _np(out1))


@pytest.mark.parametrize("k", [1, 3, 64])
def test_index_rule_knn_normal(lib, k):
    """... for averaged rows and for unmoved rows alike (rows 5 and 128 are made unmoved: the bad entry is then the copied
    column at k = 1 and column 0 of row 128, and a column the copy does not read otherwise)."""
    nq = BAD_N
    knn_d, _, nm, _ = _knn_normal_inputs(nq, k, 85 + k)
    nr = nm.shape[2]
    table, bad, rows = _bad_tables(nq, nr, k, 86 + k)                 # "N" is the size of the cloud the table points into
    knn_d[:, 5, 0] = knn_d[:, 128, 0] = 0.0
    rc0, out0 = _knn_normal(lib, _dev(knn_d), _dev(table), _dev(nm))
    rc1, out1 = _knn_normal(lib, _dev(knn_d), _dev(bad), _dev(nm))
    assert rc0 == OK and rc1 == OK
    _expect_rows(_np(out1), _np(out0), rows)


def test_wrappers_refuse_a_cloud_smaller_than_its_neighbourhood():
    """5 points, k = 16: the search would pad the table with -1.  Refused by name before any kernel runs."""
    from geoa3_amd import utility as U
    from geoa3_amd._lib import Geoa3Error
    pc = torch.randn(2, 3, 5, generator=torch.Generator().manual_seed(1)).cuda()
    nrm = torch.nn.functional.normalize(pc, dim=1)
    z = torch.zeros(2, 5, device="cuda")
    for call in (lambda: U.local_frames(pc, 16), lambda: U.smoothness(pc, 16, 16), lambda: U.smoothness(pc, 3, 16),
                 lambda: U.estimate_perpendicular(pc, 16, aux=(z, z)), lambda: U.estimate_normal(pc, 16),
                 lambda: U.estimate_normal(pc, 16, "outward"),
                 lambda: U.estimate_normal_via_ori_normal(pc, pc, nrm, 16)):
        with pytest.raises(Geoa3Error, match="needs at least 1[67] points per cloud"):
            call()
    # ... and the smallest cloud that is accepted: k + 1 points (k of them for the cross search)
    assert torch.isfinite(U.local_frames(pc, 4)[0]).all() and torch.isfinite(U.smoothness(pc, 4, 4)).all()
    assert torch.isfinite(U.estimate_normal_via_ori_normal(pc + 0.01, pc, nrm, 5)).all()
