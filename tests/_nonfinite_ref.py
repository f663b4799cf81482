"""The NaN / inf rule of the neighbour searches (geoa3_nn1_pair, geoa3_grid_nn1_pair, geoa3_knn, geoa3_knn_self), restated
in plain numpy with float32 arithmetic.  tests/test_nonfinite_ref.py pins it to the oracle on finite clouds and to a table
written by hand; tests/test_gpu_nonfinite.py holds every search to it bit for bit.

The distance is the un-fused expression of geoa3_sqdist (csrc/common.h), every operation rounded to float32:
    dx = ax - bx, dy = ay - by, dz = az - bz;  d = (dx*dx + dy*dy) + dz*dz
so a NaN coordinate, or +inf against +inf on one axis, gives a NaN distance and an inf coordinate against a finite one +inf.

nn1: a running minimum from (+inf, 0) over the candidates in ascending index, a candidate taken only if d < best: neither a
     NaN nor a +inf distance is ever taken; a query without a finite distance answers (+inf, 0).
knn: the candidates are the points whose distance is not NaN (+inf IS one), ordered by (distance, index), the first K kept,
     missing slots (+inf, -1)."""
import numpy as np

ROWS = 512   # queries per block of the distance matrix (memory, not arithmetic)


def sqdist(q, r):
    """q [3,Nq], r [3,Nr] float32 -> [Nq,Nr] float32, un-fused."""
    q = np.asarray(q, dtype=np.float32)
    r = np.asarray(r, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = q[0][:, None] - r[0][None, :]
        dy = q[1][:, None] - r[1][None, :]
        dz = q[2][:, None] - r[2][None, :]
        d = (dx * dx + dy * dy) + dz * dz
    assert d.dtype == np.float32
    return d


def nn1(q, r):
    """-> (d [Nq] float32, i [Nq] int32)"""
    nq = np.asarray(q).shape[1]
    dist = np.empty(nq, dtype=np.float32)
    idx = np.empty(nq, dtype=np.int32)
    for a in range(0, nq, ROWS):
        d = sqdist(np.asarray(q)[:, a:a + ROWS], r)
        takeable = np.where(np.isnan(d), np.float32(np.inf), d)     # d < best is false for NaN ...
        i = np.argmin(takeable, axis=1)                             # (the first of equal minima: ascending index, strict <)
        best = takeable[np.arange(d.shape[0]), i]
        i = np.where(best < np.float32(np.inf), i, 0)               # ... and for +inf: the start value (+inf, 0) stays
        dist[a:a + ROWS] = best
        idx[a:a + ROWS] = i
    return dist, idx


def knn(q, r, K):
    """-> (d [Nq,K] float32, i [Nq,K] int32)"""
    q = np.asarray(q, dtype=np.float32)
    nq, nr = q.shape[1], np.asarray(r).shape[1]
    dist = np.full((nq, K), np.inf, dtype=np.float32)
    idx = np.full((nq, K), -1, dtype=np.int32)
    keep = min(K, nr)
    for a in range(0, nq, ROWS):
        d = sqdist(q[:, a:a + ROWS], r)
        # (distance, index) as ONE integer: a distance is a sum of squares (>= +0 or NaN), so its bits order like its value
        bits = d.view(np.uint32).astype(np.uint64)
        assert not ((bits >> np.uint64(31)) & ~np.isnan(d)).any()
        key = (bits << np.uint64(32)) | np.arange(nr, dtype=np.uint64)[None, :]
        key[np.isnan(d)] = np.uint64(0xFFFFFFFFFFFFFFFF)            # no candidate: behind every real one
        if keep < nr:
            key = np.partition(key, keep - 1, axis=1)[:, :keep]
        key = np.sort(key, axis=1)[:, :keep]
        real = key != np.uint64(0xFFFFFFFFFFFFFFFF)
        dd = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
        ii = (key & np.uint64(0xFFFFFFFF)).astype(np.int64).astype(np.int32)
        dist[a:a + ROWS, :keep] = np.where(real, dd, np.float32(np.inf))
        idx[a:a + ROWS, :keep] = np.where(real, ii, -1)
    return dist, idx


def same_bits(a, b):
    """float32 arrays equal as int32 bit patterns, every NaN equal to every NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.int32)[~na] == b.view(np.int32)[~nb]).all())
