"""geoa3_knn_nd (csrc/geom_knn_nd.hip) and knn_points for D != 3 on the device, BIT FOR BIT against the float32 loops of
tests/_knn_nd_ref.py.  The kernel's sizes: 128 queries per workgroup (one per thread); a reference tile of 8192 / DB points,
DB the dimension's bucket (8, 32, 64, 128): 128 points at D = 64, 64 at D = 128.  Candidate lists hold 40 / 72 / 96
entries for K <= 20 / 40 / 64, so K = 1, 5, 20, 45 takes all three and Nr = 45 compacts at least once for K <= 20."""
import functools

import numpy as np
import pytest
import torch

from tests import _knn_nd_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
OK, EINVAL, ENOSUPPORT = 0, -1, -3


@pytest.fixture(scope="module")
def ops():
    from geoa3_amd import ops as _ops
    assert torch.cuda.is_available(), "needs the MI355X"
    return _ops


def _guarded(shape, dtype=torch.float32, pad=64, fill=-7.0):
    """an output inside a larger buffer: (the contiguous view of `shape`, pre-filled with NaN / -99, check of the guards)"""
    n = int(np.prod(shape))
    buf = torch.full((pad + n + pad,), fill, device="cuda", dtype=dtype)
    view = buf[pad:pad + n].view(shape)
    view.fill_(NAN if dtype == torch.float32 else -99)
    return view, lambda: bool((buf[:pad] == fill).all() and (buf[pad + n:] == fill).all())


def _same_bits(got, want):
    g = np.ascontiguousarray(got.detach().cpu().numpy(), dtype=np.float32).view(np.int32)
    w = np.ascontiguousarray(want, dtype=np.float32).view(np.int32)
    return g.shape == w.shape and bool(np.array_equal(g, w))


def _clouds(B, Nq, Nr, D, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, Nq, D, generator=g) * 2 - 1).float(), (torch.rand(B, Nr, D, generator=g) * 2 - 1).float()


def _search(ops, q, r, K):
    """the search into guarded buffers: (dists, idx) after checking the guard bands"""
    B, Nq, _ = q.shape
    d, dok = _guarded((B, Nq, K))
    i, iok = _guarded((B, Nq, K), torch.int32)
    ops.knn_nd(q.cuda(), r.cuda(), K, out=(d, i))
    torch.cuda.synchronize()
    assert dok() and iok()
    return d, i


@functools.lru_cache(maxsize=None)
def _case(D):
    """B=3, Nq=70, Nr=45 at dimension D with the checker's full ordering (K = 45): computed once, sliced per K"""
    q, r = _clouds(3, 70, 45, D, 1000 + D)
    wd, wi = R.knn_nd(q.numpy(), r.numpy(), 45)
    return q, r, wd, wi


@pytest.mark.parametrize("K", [1, 5, 20, 45])
@pytest.mark.parametrize("D", [1, 2, 4, 7, 64, 65, 128])
def test_bit_for_bit_against_the_float32_loop(ops, D, K):
    q, r, wd, wi = _case(D)
    d, i = _search(ops, q, r, K)
    assert np.array_equal(i.cpu().numpy(), wi[:, :, :K])
    assert _same_bits(d, wd[:, :, :K])


@pytest.mark.parametrize("D,tile", [(64, 128), (128, 64)])
def test_one_point_past_the_reference_tile_and_the_query_block(ops, D, tile):
    """Nr = reference tile + 1, Nq = query block (128) + 1: the last tile holds one point, the last workgroup one query"""
    q, r = _clouds(2, 129, tile + 1, D, 7 + D)
    wd, wi = R.knn_nd(q.numpy(), r.numpy(), 20)
    d, i = _search(ops, q, r, 20)
    assert np.array_equal(i.cpu().numpy(), wi) and _same_bits(d, wd)
    assert (i.cpu().numpy() == tile).any()     # the point alone in its tile is somebody's neighbour


def test_duplicates_and_exact_ties(ops):
    """integer coordinates in {0, 1, 2}, D = 5, every point three times: distances are small integers, tied in dozens --
    the order inside a tie is the index's"""
    g = torch.Generator().manual_seed(3)
    base = torch.randint(0, 3, (2, 30, 5), generator=g).float()
    r = torch.cat((base, base, base), 1)                      # Nr = 90
    q = torch.randint(0, 3, (2, 70, 5), generator=g).float()
    wd, wi = R.knn_nd(q.numpy(), r.numpy(), 20)
    d, i = _search(ops, q, r, 20)
    assert np.array_equal(i.cpu().numpy(), wi) and _same_bits(d, wd)
    d64, i64 = R.knn_nd_f64(q.numpy(), r.numpy(), 20)         # exact arithmetic: the float64 search agrees
    assert np.array_equal(wi, i64) and np.array_equal(wd.astype(np.float64), d64)
    assert (np.diff(wd, axis=2) == 0).mean() > 0.5            # ... and most neighbours ARE tied with the one before


def test_non_finite_coordinates_keep_indices_in_range(ops):
    """a NaN in one query, an inf in another, a NaN and an inf in two reference points (D = 7): every index stays in
    [0, Nr) and is distinct within its row; queries with finite coordinates equal the checker (which orders a NaN distance
    as +inf) everywhere, so the finite part of the cloud is searched as if the bad points were infinitely far away"""
    q, r = _clouds(2, 70, 45, 7, 11)
    q[0, 3, 2] = NAN
    q[1, 5, 0] = float("inf")
    r[0, 9, 1] = NAN
    r[1, 17, 6] = float("-inf")
    K = 45
    wd, wi = R.knn_nd(q.numpy(), r.numpy(), K)
    d, i = _search(ops, q, r, K)
    ii = i.cpu().numpy()
    assert ii.min() >= 0 and ii.max() < 45
    assert all(len(set(row)) == K for row in ii.reshape(-1, K))
    assert np.array_equal(ii, wi) and _same_bits(d, wd)
    assert np.isinf(wd[0, 3]).all() and np.isinf(wd[1, 5]).all()      # the two bad queries: every distance +inf
    assert (wi[0, :, -1] == 9)[np.arange(70) != 3].all()              # the NaN point is everybody's last neighbour
    assert not np.isnan(d.cpu().numpy()).any()


@pytest.mark.parametrize("D,K,Nq,Nr,code", [(0, 5, 70, 45, EINVAL), (129, 5, 70, 45, ENOSUPPORT), (7, 0, 70, 45, EINVAL),
                                            (7, 46, 70, 45, EINVAL), (7, 65, 70, 100, ENOSUPPORT),
                                            (2, 5, 8193, 45, ENOSUPPORT), (2, 5, 70, 8193, ENOSUPPORT)])
def test_refused_sizes_write_nothing(ops, D, K, Nq, Nr, code):
    from geoa3_amd import _lib
    q = torch.zeros(1, Nq, max(D, 1), device="cuda")
    r = torch.zeros(1, Nr, max(D, 1), device="cuda")
    d, dok = _guarded((1, Nq, max(K, 1)))
    i, iok = _guarded((1, Nq, max(K, 1)), torch.int32)
    rc = _lib.load().geoa3_knn_nd(q.data_ptr(), r.data_ptr(), 1, Nq, Nr, D, K, d.data_ptr(), i.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == code
    assert torch.isnan(d).all() and (i == -99).all() and dok() and iok()
    if D >= 1 and K >= 1:
        with pytest.raises(_lib.Geoa3Error):
            ops.knn_nd(q, r, K)


# ------------------------------------------------------------------------------------------------ the operator
def test_knn_points_d7_and_its_gradient(ops):
    p1, p2 = _clouds(3, 70, 45, 7, 21)
    g = torch.Generator().manual_seed(22)
    w = (torch.rand(3, 70, 5, generator=g) + 0.5).float()
    wd, wi = R.knn_nd(p1.numpy(), p2.numpy(), 5)
    a, b = p1.cuda().requires_grad_(), p2.cuda().requires_grad_()
    out = ops.knn_points(a, b, K=5, return_nn=True)
    assert out.idx.dtype == torch.int64 and np.array_equal(out.idx.cpu().numpy(), wi)
    assert _same_bits(out.dists, wd)
    assert torch.equal(out.knn.detach(), torch.gather(p2.cuda(), 1, out.idx.reshape(3, -1, 1).expand(3, 350, 7)).view(3, 70, 5, 7))
    out.dists.backward(w.cuda())
    g1, g2 = R.knn_points_grad(p1.numpy(), p2.numpy(), wi, w.numpy())
    assert _same_bits(a.grad, g1) and _same_bits(b.grad, g2)


def test_knn_points_d3_is_todays_path(ops):
    """D == 3 keeps the planar searches: the same bits as ops.knn_planar / ops.nn1_pair on the same data"""
    p1, p2 = _clouds(3, 70, 45, 3, 31)
    q, r = p1.cuda().permute(0, 2, 1).contiguous(), p2.cuda().permute(0, 2, 1).contiguous()
    for K in (5, 20):
        d, i = ops.knn_planar(q, r, K)
        out = ops.knn_points(p1.cuda(), p2.cuda(), K=K)
        assert torch.equal(out.dists, d) and torch.equal(out.idx, i.long())
    d, i, _, _ = ops.nn1_pair(q, r, both=False, method="auto")
    out = ops.knn_points(p1.cuda(), p2.cuda(), K=1)
    assert torch.equal(out.dists[:, :, 0], d) and torch.equal(out.idx[:, :, 0], i.long())


def test_knn_points_d7_compiles_fullgraph(ops):
    p1, p2 = _clouds(2, 70, 45, 7, 41)

    def f(a, b):
        out = ops.knn_points(a, b, K=5, return_nn=True)
        return out.dists.sum() + out.knn.sum(), out.idx

    res = []
    for fn in (f, torch.compile(f, fullgraph=True, backend="aot_eager")):
        a, b = p1.cuda().requires_grad_(), p2.cuda().requires_grad_()
        val, idx = fn(a, b)
        ga, gb = torch.autograd.grad(val, (a, b))
        res.append((val.detach(), idx, ga, gb))
    assert all(torch.equal(x, y) for x, y in zip(*res))
