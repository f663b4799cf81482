"""Checkers of the D-dimensional K-NN (csrc/geom_knn_nd.hip) and of knn_points' gradient for D != 3, written from the
contract alone (include/geoa3_hip.h, INTEGRATION.md "Ties"): plain float32 numpy, one rounding per operation.

    dist(q, r) = acc_D,  acc_0 = +0.0,  acc_{d+1} = fl(acc_d + fl(fl(q_d - r_d)^2))
    results ascend by (distance, index), equal distances to the lower index; a NaN distance counts (and reads) as +inf
    t(i,k,:) = fl(fl(2 gd[i,k]) * fl(p1[i,:] - p2[idx[i,k],:]));  g1[i] = sum_k t(i,k) ascending k from +0.0;
    g2[j] = sum of -t(i,k) over idx[i,k] == j in ascending (i, k) from +0.0
"""
import numpy as np

F = np.float32


def sqdist(q, r):
    """q [Nq,D], r [Nr,D] float32 -> [Nq,Nr] float32, the sequential sum over d"""
    q, r = np.asarray(q, F), np.asarray(r, F)
    acc = np.zeros((q.shape[0], r.shape[0]), F)
    with np.errstate(all="ignore"):
        for d in range(q.shape[1]):
            t = (q[:, d, None] - r[None, :, d]).astype(F)
            t = (t * t).astype(F)
            acc = (acc + t).astype(F)
    return acc


def knn_nd(q, r, K):
    """q [B,Nq,D], r [B,Nr,D] -> (dists float32 [B,Nq,K], idx int64 [B,Nq,K])"""
    B, Nq, _ = q.shape
    Nr = r.shape[1]
    dists, idx = np.empty((B, Nq, K), F), np.empty((B, Nq, K), np.int64)
    ar = np.arange(Nr)
    for b in range(B):
        d = sqdist(q[b], r[b])
        d = np.where(np.isnan(d), F(np.inf), d)
        for i in range(Nq):
            o = np.lexsort((ar, d[i]))[:K]      # by distance, then by index
            dists[b, i], idx[b, i] = d[i, o], o
    return dists, idx


def knn_nd_f64(q, r, K):
    """the same search with float64 distances (equal to the float32 ones wherever those are exact, e.g. small integers)"""
    q, r = np.asarray(q, np.float64), np.asarray(r, np.float64)
    d = ((q[:, :, None, :] - r[:, None, :, :]) ** 2).sum(-1)
    ar = np.arange(r.shape[1])
    idx = np.stack([np.stack([np.lexsort((ar, d[b, i]))[:K] for i in range(q.shape[1])]) for b in range(q.shape[0])])
    return np.take_along_axis(d, idx, 2), idx


def knn_points_grad(p1, p2, idx, gd):
    """p1 [B,N1,D], p2 [B,N2,D], idx int [B,N1,K], gd [B,N1,K] -> (g1 [B,N1,D], g2 [B,N2,D]), every sum sequential"""
    p1, p2, gd = np.asarray(p1, F), np.asarray(p2, F), np.asarray(gd, F)
    B, N1, K = idx.shape
    g1, g2 = np.zeros(p1.shape, F), np.zeros(p2.shape, F)
    for b in range(B):
        for i in range(N1):
            for k in range(K):
                j = int(idx[b, i, k])
                t = ((F(2.0) * gd[b, i, k]).astype(F) * (p1[b, i] - p2[b, j]).astype(F)).astype(F)
                g1[b, i] = (g1[b, i] + t).astype(F)
                g2[b, j] = (g2[b, j] - t).astype(F)
    return g1, g2
