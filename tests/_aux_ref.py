"""Plain numpy restatements of the kernels of geoa3_amd/csrc/geom_aux.hip that tests/_normal_ref.py does not cover (no
project code, no torch): the yardstick of tests/test_aux_ref.py (CPU) and tests/test_gpu_aux_kernels.py (GPU).

Every function takes ONE cloud and a `dtype`:

* `np.float64` is the high-precision statement of the formula;
* `np.float32` evaluates the same formula in the kernel's stated operation order, one rounding per operation and no
  fused multiply-add.  Where the kernel's chain cannot contract and its roots and quotients are correctly rounded, the
  float32 form is what the kernel returns BIT FOR BIT: fps_sample, sor_statistic, perp_jitter, the copied rows of
  knn_normal and both selections of sor_select.  smoothness and the averaged rows of knn_normal hold products that feed
  sums (the compiler may fuse them), so they are held to float64 within the bounds derived below.

u = 2^-24 is the unit roundoff of float32 (round to nearest); bounds compose to first order and carry one spare u for
the second-order terms (c^2 u^2 with c < 100 is below 1e-5 u).

    fps_sample     d_i = sqrt((dx^2 + dy^2) + dz^2); dist = min(dist, d); next = the FIRST index of the maximum
    sor_statistic  d_ij = (dx^2 + dy^2) + dz^2, dx = (p_j - p_i) + fl32(1e-10); the K+1 smallest ascending, the first
                   dropped, sqrt of each, summed in that order, / K.  A point with a non-finite coordinate is NaN and is
                   no neighbour of the others (d_ij is NaN or +inf and never enters a list of finite values).
    sor_select     mode 0: a stable sort by (-inf < finite < +inf < NaN, -0 == +0), ties to the lower index; the first
                   N - drop_num are kept.  mode 1: dis < fl32(fl32(mean) + fl32(alpha fl32(std))), unbiased std.
    smoothness     s_i = (1/k) sum_{m=1..k} |(dx nx + dy ny) + dz nz|, d = p[table[i,m]] - p_i, n_i = evecs[0,:,i]
    perp_jitter    out_c = clamp(E[2,c] a1) + clamp(E[1,c] a2); the clamp keeps NaN
    knn_normal     knn_d[i,0] < fl32(1e-6): normal[knn_i[i,0]]; else s / (|s| + fl32(1e-12)), s = (sum_m n_m) fl(1/K)
"""
import numpy as np

F = np.float32
U32 = 2.0 ** -24
EPS_SOR = F(1e-10)
EPS_NRM = F(1e-12)
MOVED = F(1e-6)


# ------------------------------------------------------------------ farthest point sampling
def fps_sample(pc, m, start, dtype=F):
    """pc [3,N], first index `start` (clamped into [0,N)) -> (idx int64 [m], points [3,m] = pc[:, idx])."""
    p = np.asarray(pc, dtype)
    n = p.shape[1]
    cur = min(max(int(start), 0), n - 1)
    dist = np.full(n, np.inf, dtype)
    idx = np.empty(m, np.int64)
    for r in range(m):
        idx[r] = cur
        if r == m - 1:
            break
        d = p - p[:, cur:cur + 1]
        dd = d * d
        dist = np.minimum(dist, np.sqrt((dd[0] + dd[1]) + dd[2]))
        cur = int(np.argmax(dist))                       # the first of equal maxima
    return idx, p[:, idx]


# ------------------------------------------------------------------ statistical outlier removal
def sor_sqdist(pc, dtype=F):
    """pc [3,N] -> [N,N], row i = ((p_j - p_i) + 1e-10)^2 summed (x + y) + z."""
    p = np.asarray(pc, dtype)
    eps = dtype(EPS_SOR)
    with np.errstate(all="ignore"):
        d = (p[:, None, :] - p[:, :, None]) + eps        # [3,i,j] = p_j - p_i
        dd = d * d
        return (dd[0] + dd[1]) + dd[2]


def sor_statistic(pc, K, dtype=F):
    """pc [3,N] -> dis [N]."""
    p = np.asarray(pc, dtype)
    n = p.shape[1]
    d = sor_sqdist(p, dtype)
    d = np.where(np.isnan(d), dtype(np.inf), d)          # never below a list's worst entry: passed over
    best = np.sort(d, axis=1)[:, :K + 1]
    with np.errstate(all="ignore"):
        root = np.sqrt(best[:, 1:])
        acc = np.zeros(n, dtype)
        for m in range(K):
            acc = acc + root[:, m]
        out = acc / dtype(K)
    lost = ~np.isfinite(p).all(axis=0)
    return np.where(lost, dtype(np.nan), out)


def sor_statistic_tol(dis64, K):
    """|float32 chain - float64 chain| <= (K + 6) u dis.  Per distance: the difference p_j - p_i (u) and the added 1e-10
    (u) move dx by at most 2u |dx| (1e-10 is far below one ulp of any non-zero difference, and alone it is exact), so the
    square by 4u + u; the two additions u each: d within 7u, its root within 3.5u + u.  The k-th smallest of perturbed
    values moves by no more than the largest perturbation, so the choice of neighbours needs no term.  K - 1 additions
    and the quotient: (K - 1 + 1) u.  4.5 + K, rounded up, and the spare u."""
    return (K + 6) * U32 * np.abs(dis64)


def select_fixnum(dis, drop_num):
    """dis [N] -> the kept indices, ascending: the N - drop_num first of the total order (no torch.topk)."""
    d = np.asarray(dis)
    n = d.shape[0]
    nan = np.isnan(d)
    val = np.where(nan, 0.0, d.astype(np.float64)) + 0.0  # -0 + 0 = +0; +-inf order by themselves
    order = np.lexsort((np.arange(n), val, nan.astype(np.int8)))   # last key first: NaN class, value, index
    return np.sort(order[:n - drop_num])


def variance_stats(dis):
    """dis [N] float32 -> (mean, unbiased std) in float64."""
    d = np.asarray(dis, np.float64)
    mean = d.mean()
    return mean, np.sqrt(((d - mean) ** 2).sum() / (d.shape[0] - 1))


def variance_threshold(mean32, std32, alpha):
    """fl32(fl32(mean) + fl32(alpha * fl32(std))) from the float32 statistics (defense.py:33-35)."""
    with np.errstate(all="ignore"):
        scaled = F(F(alpha) * F(std32))
        return F(F(mean32) + scaled)


def select_variance(dis, mean32, std32, alpha):
    """the kept indices, ascending: dis < threshold (a NaN threshold or a NaN dis keeps nothing of it)."""
    with np.errstate(all="ignore"):
        return np.nonzero(np.asarray(dis, F) < variance_threshold(mean32, std32, alpha))[0]


def ulp32(x):
    """the spacing of float32 at |x|"""
    return float(np.spacing(np.abs(F(x))))


# ------------------------------------------------------------------ smoothness
def smoothness(pc, table, evecs, dtype=np.float64):
    """pc [3,N], table int [N,k+1] (column 0 is not read), evecs [3(e),3(xyz),N] -> (s [N], mag [N]) with
    mag_i = (1/k) sum_m sum_c |d_c n_c| in float64, the magnitude the bound of `smoothness_tol` scales with."""
    p = np.asarray(pc, dtype).T                           # [N,3]
    nrm = np.asarray(evecs, dtype).reshape(3, 3, -1)[0].T  # [N,3]
    nb = np.asarray(table)[:, 1:]
    k = nb.shape[1]
    with np.errstate(all="ignore"):
        d = p[nb] - p[:, None, :]                         # [N,k,3]
        prod = d * nrm[:, None, :]
        t = np.abs((prod[:, :, 0] + prod[:, :, 1]) + prod[:, :, 2])
        acc = np.zeros(p.shape[0], dtype)
        for m in range(k):
            acc = acc + t[:, m]
        s = acc / dtype(k)
        p64, n64 = np.asarray(pc, np.float64).T, np.asarray(evecs, np.float64).reshape(3, 3, -1)[0].T
        mag = np.abs((p64[nb] - p64[:, None, :]) * n64[:, None, :]).sum(axis=(1, 2)) / k
    return s, mag


def smoothness_c(k):
    """C of |got - want| <= C u mag.  One term |(dx nx + dy ny) + dz nz|: each difference u, each product u (none when
    fused: not counted on), the two additions u each on partial sums of at most sum_c |d_c n_c|: 4u sum_c |d_c n_c|; the
    absolute value is exact.  The k terms are added one after the other from 0: k - 1 roundings of partial sums of at
    most the whole sum.  The quotient by k: u.  (4 + k - 1 + 1) u = (k + 4) u, and the spare u."""
    return k + 5


# ------------------------------------------------------------------ tangent-plane jitter
def perp_jitter(evecs, aux1, aux2, clip, dtype=F):
    """evecs [3(e),3(xyz),N], aux1 / aux2 [N] -> [3,N]."""
    e = np.asarray(evecs, dtype).reshape(3, 3, -1)
    c = dtype(clip)
    with np.errstate(all="ignore"):
        t1 = np.clip(e[2] * np.asarray(aux1, dtype)[None, :], -c, c)     # np.clip keeps NaN
        t2 = np.clip(e[1] * np.asarray(aux2, dtype)[None, :], -c, c)
        return t1 + t2


# ------------------------------------------------------------------ normals of moved points
def knn_normal(knn_d, knn_i, normals, dtype=np.float64):
    """knn_d float32 [Nq,K], knn_i int [Nq,K], normals [3,Nr] -> (out [3,Nq], tol [3,Nq], averaged bool [Nq]).  tol is 0
    on the copied rows (they are exact) and on the others the bound a float32 evaluation has to meet:

    s_c = (sum_m n_mc) fl(1/K): K - 1 additions, the rounding of 1/K and the product: e_c = (K + 1) u (1/K) sum_m |n_mc|,
    plus the spare u: (K + 2) u.  |s| = sqrt((sx^2 + sy^2) + sz^2) + 1e-12 computed FROM the float32 s: three squares and
    two additions 3u on the sum, 1.5u after the root, the root u, the addition u, then the quotient u: 4.5u, rounded up
    to 5u, relative to |out_c|.  The shift of s itself moves the quotient by e_c / |s| and, through the norm, by
    |out_c| |e|_2 / |s|:
        tol_c = (e_c + |out_c| |e|_2) / (|s| + 1e-12) + 6u |out_c|."""
    nm = np.asarray(normals, dtype)
    idx = np.asarray(knn_i)
    nq, K = idx.shape
    g = nm[:, idx]                                        # [3,Nq,K]
    with np.errstate(all="ignore"):
        s = np.zeros((3, nq), dtype)
        for m in range(K):
            s = s + g[:, :, m]
        s = s * (dtype(1.0) / dtype(K))
        nrm = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]) + dtype(EPS_NRM)
        avg = s / nrm
        moved = ~(np.asarray(knn_d, F)[:, 0] < MOVED)
        out = np.where(moved[None, :], avg, nm[:, idx[:, 0]])
        e = (K + 2) * U32 * np.abs(np.asarray(normals, np.float64)[:, idx]).sum(axis=2) / K
        tol = (e + np.abs(avg) * np.sqrt((e * e).sum(axis=0))) / nrm + 6 * U32 * np.abs(avg)
    return out, np.where(moved[None, :], tol, 0.0), moved
