"""Float64 numpy restatements of the input-side geometry (PCA normals, the re-sampling's normalisation), written from
the formulas: the yardstick of tests/test_normal_ref.py (CPU) and tests/test_gpu_normal.py (GPU kernels).

    C_i  = 1/(k-1) * sum_{m=1..k} (q_m - mean)(q_m - mean)^T      q_m = the k neighbours of p_i, p_i itself left out
    n_i  = unit eigenvector of the smallest eigenvalue of C_i (numpy.linalg.eigh)
    sign = largest-magnitude component positive (orient None), or <n_i, p_i - centroid> >= 0 ("outward"; a dot product
           of exactly 0 keeps the first sign)
    normalised cloud = (p - mean over the points) / max_i |p_i - mean|
"""
import numpy as np


def knn_table(pc, k1):
    """pc [3,n] -> int64 [n,k1]: the k1 nearest points of every point by (squared distance, index), brute force in
    float64; column 0 is the point itself (or an exact duplicate with a lower index)."""
    p = np.asarray(pc, dtype=np.float64).T
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    return np.argsort(d, axis=1, kind="stable")[:, :k1]


def neighbourhood_cov(pc, idx):
    """pc [3,n], idx [n,k+1] -> covariance [n,3,3] (factor 1/(k-1)) of columns 1..k of every row."""
    p = np.asarray(pc, dtype=np.float64).T
    q = p[np.asarray(idx)[:, 1:]]                        # [n,k,3]
    q = q - q.mean(axis=1, keepdims=True)
    k = q.shape[1]
    return np.einsum("nka,nkb->nab", q, q) / (k - 1)


def canonical_sign(v):
    """v [n,3] -> [n,1]: the sign that makes the largest-magnitude component (the first of equals) positive."""
    lead = np.take_along_axis(v, np.abs(v).argmax(axis=1)[:, None], axis=1)
    return np.where(lead < 0, -1.0, 1.0)


def estimate_normal(pc, idx, orient=None):
    """pc [3,n], idx [n,k+1] -> (normals [3,n] float64, eigenvalues [n,3] ascending)."""
    p = np.asarray(pc, dtype=np.float64)
    w, v = np.linalg.eigh(neighbourhood_cov(p, idx))     # ascending; v[..., :, e] is eigenvector e
    n = v[:, :, 0]
    n = n * canonical_sign(n)
    if orient == "outward":
        d = (n * (p.T - p.mean(axis=1)[None, :])).sum(axis=1, keepdims=True)
        n = np.where(d < 0, -n, n)
    elif orient is not None:
        raise ValueError(orient)
    return n.T, w


def normalize_cloud(pts):
    """pts [3,m] -> (out [3,m], mean [3], scale): centred on the mean, divided by the largest point norm."""
    p = np.asarray(pts, dtype=np.float64)
    mean = p.mean(axis=1)
    q = p - mean[:, None]
    scale = np.sqrt((q * q).sum(axis=0)).max()
    return q / scale, mean, scale
