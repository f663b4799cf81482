"""The three formulas of csrc/geom_knn_ops.hip (geoa3_knn_gather, geoa3_knn_gather_grad, geoa3_knn_points_grad) restated
as plain numpy float32 loops in exactly the stated order: every sum sequential in float32, from +0.0, in ascending entry
number e = l K + k (g1: ascending k); an index outside [0, M) gives NaN in the gather and no term in the sums.
tests/test_knn_ops_ref.py pins this restatement to float64 autograd through the oracle; tests/test_gpu_knn_ops.py holds
the kernels to it bit for bit.

`drop`: a set of (b, e) entries to leave out (test_knn_ops_ref.py shows that one missing term is seen)."""
import numpy as np

F = np.float32


def knn_gather(x, idx):
    """x [B,M,U] float32, idx [B,L,K] int64 -> [B,L,K,U]."""
    x = np.asarray(x, dtype=F)
    idx = np.asarray(idx, dtype=np.int64)
    B, M, U = x.shape
    _, L, K = idx.shape
    out = np.full((B, L, K, U), np.nan, dtype=F)
    for b in range(B):
        for l in range(L):
            for k in range(K):
                j = idx[b, l, k]
                if 0 <= j < M:
                    out[b, l, k, :] = x[b, j, :]
    return out


def knn_gather_grad(g, idx, M, drop=()):
    """g [B,L,K,U] float32, idx [B,L,K] int64 -> gx [B,M,U]: gx[b,j,:] = the g[b,l,k,:] with idx[b,l,k] == j, added one
    after the other in ascending e = l K + k."""
    g = np.asarray(g, dtype=F)
    idx = np.asarray(idx, dtype=np.int64)
    B, L, K, U = g.shape
    E = L * K
    ge, ie = g.reshape(B, E, U), idx.reshape(B, E)
    gx = np.zeros((B, M, U), dtype=F)
    for b in range(B):
        for e in range(E):
            j = ie[b, e]
            if 0 <= j < M and (b, e) not in drop:
                gx[b, j, :] = gx[b, j, :] + ge[b, e, :]     # one float32 addition per component
    return gx


def knn_points_terms(p1, p2, idx, gd):
    """t[b,i,k,c] = fl( fl(2 gd[b,i,k]) * fl(p1[b,i,c] - p2[b,idx[b,i,k],c]) ) (float32; garbage where idx is out of range)
    and the mask of the entries whose index is inside [0, N2)."""
    p1, p2, gd = np.asarray(p1, dtype=F), np.asarray(p2, dtype=F), np.asarray(gd, dtype=F)
    idx = np.asarray(idx, dtype=np.int64)
    B, N2 = p2.shape[0], p2.shape[1]
    ok = (idx >= 0) & (idx < N2)
    safe = np.where(ok, idx, 0)
    nb = p2[np.arange(B)[:, None, None], safe]                 # [B,N1,K,3]
    w = (F(2.0) * gd).astype(F)
    df = (p1[:, :, None, :] - nb).astype(F)
    return (w[..., None] * df).astype(F), ok


def knn_points_grad(p1, p2, idx, gd, drop=()):
    """-> (g1 [B,N1,3], g2 [B,N2,3]): g1[b,i,:] = t(i,0,:) + t(i,1,:) + ... in that order; g2[b,j,:] = the -t(i,k,:) with
    idx[b,i,k] == j added one after the other in ascending e = i K + k."""
    t, ok = knn_points_terms(p1, p2, idx, gd)
    idx = np.asarray(idx, dtype=np.int64)
    B, N1, K = idx.shape
    N2 = np.asarray(p2).shape[1]
    g1 = np.zeros((B, N1, 3), dtype=F)
    g2 = np.zeros((B, N2, 3), dtype=F)
    for b in range(B):
        for i in range(N1):
            for k in range(K):
                if not ok[b, i, k] or (b, i * K + k) in drop:
                    continue
                j = idx[b, i, k]
                g1[b, i, :] = g1[b, i, :] + t[b, i, k, :]
                g2[b, j, :] = g2[b, j, :] + (-t[b, i, k, :])
    return g1, g2
