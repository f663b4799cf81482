"""A numpy float64 restatement of the kernels of csrc/geom_reg.hip that takes the neighbour table AS GIVEN (no search, no
dense N x N: pair lists), for tables no search would return: repeated indices in a row, the point itself beyond column 0, a
hub, poisoned columns.  It states what the header of geom_reg.hip defines:

  * only columns 1..k of the table are read (column 0 and the columns beyond k never);
  * kNN_smoothing_loss reads the table's DISTANCES for s_i, the threshold (unbiased std) and the mask; its gradient forms
    the pair terms from the cloud's coordinates: 2 w_i (x_i - x_j) added to i and subtracted from j, w_i = mask_i g_b / (N k);
  * repulsion_loss: the forward from the table's distances, the gradient with d recomputed from the coordinates;
  * displacement_loss: theta from the float32 coordinates in double; the pair term is a scalar on d theta;
  * corresponding_normal_loss: the gradient only (the forward is geoa3_kappa's);
  * an index outside [0, N) in columns 1..k makes the instance's gradient NaN (displacement_loss forward: that point only);
    a non-finite distance in columns 1..k makes kNN_smoothing_loss's loss NaN, its mask 0 and its gradient NaN.

Every gradient comes with what the kernel's error bound needs: n [B,N], the number of pair terms a point receives (pairs
with i == j add nothing and are not counted), and tmax [B], the instance's largest |pair term| (the kernel's fixed-point unit
is 2^(ilogb(tmax) - 40)).  tests/test_reg_table_ref.py pins this file to tests/_reg_ref.py on consistent tables."""
import numpy as np

NORM_EPS = 1e-12


def _np(a, dtype=None):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    return a.astype(dtype) if dtype is not None else a


def _pairs(idx_b, k):
    """idx_b [N,ld] -> (i [N k], j [N k]) in the kernel's pair order e = i * k + (m - 1)"""
    N = idx_b.shape[0]
    return np.repeat(np.arange(N, dtype=np.int64), k), idx_b[:, 1:k + 1].reshape(-1).astype(np.int64)


def _scatter(N, i, j, t):
    """sum of +t on i and -t on j over the pairs with i != j; t [pairs] or [pairs,C] -> [C,N] (or [N]), and the counts"""
    keep = i != j
    i, j, t = i[keep], j[keep], t[keep]
    n = np.bincount(i, minlength=N) + np.bincount(j, minlength=N)
    if t.ndim == 1:
        return np.bincount(i, t, N) - np.bincount(j, t, N), n
    return np.stack([np.bincount(i, t[:, c], N) - np.bincount(j, t[:, c], N) for c in range(t.shape[1])]), n


def _finish(B, N, per_instance):
    grad, n, tmax = np.empty((B, 3, N)), np.zeros((B, N), np.int64), np.zeros(B)
    for b in range(B):
        r = per_instance(b)
        if r is None:
            grad[b] = np.nan
            tmax[b] = np.nan
        else:
            grad[b], n[b], tmax[b] = r
    return grad, n, tmax


def _oob(j, N):
    return bool(((j < 0) | (j >= N)).any())


def smoothing(x, d, idx, k, coef, g=None):
    """-> dict(s [B,N], thr [B], mask [B,N] bool, loss [B], grad [B,3,N], n, tmax); g [B] or None = ones"""
    x, d, idx = _np(x, np.float64), _np(d, np.float64), _np(idx)
    B, _, N = x.shape
    g = np.ones(B) if g is None else _np(g, np.float64)
    with np.errstate(all="ignore"):
        s = d[:, :, 1:k + 1].sum(2) / k
        thr = s.mean(1) + coef * s.std(1, ddof=1)
        bad = ~np.isfinite(d[:, :, 1:k + 1]).all((1, 2)) | np.isnan(thr)
        mask = (s > thr[:, None]) & ~bad[:, None]
        loss = np.where(bad, np.nan, np.where(mask, s, 0.0).sum(1) / N)

    def one(b):
        i, j = _pairs(idx[b], k)
        if bad[b] or _oob(j, N) or not np.isfinite(x[b]).all():
            return None
        w = np.where(mask[b][i], g[b] / (N * float(k)), 0.0)
        t = (2.0 * w)[:, None] * (x[b][:, i] - x[b][:, j]).T
        gr, n = _scatter(N, i, j, t)
        return gr, n, np.abs(t).max()
    grad, n, tmax = _finish(B, N, one)
    return dict(s=s, thr=thr, mask=mask, loss=loss, grad=grad, n=n, tmax=tmax)


def repulsion(x, d, idx, k, h2, g=None):
    """h2 = h * h as the caller holds it (the kernels take float32(h * h)).  -> dict(out [B,N], term [B,N,k] (d exp(-u)),
    u [B,N,k] (the forward's, from the table's distances), grad, n, tmax); g [B,N] or None = ones"""
    x, d, idx = _np(x, np.float64), _np(d, np.float64), _np(idx)
    B, _, N = x.shape
    g = np.ones((B, N)) if g is None else _np(g, np.float64)
    with np.errstate(all="ignore"):
        dd = d[:, :, 1:k + 1]
        u = dd * dd / h2
        term = dd * np.exp(-u)
        out = -term.sum(2) / k

    def one(b):
        i, j = _pairs(idx[b], k)
        if _oob(j, N) or not np.isfinite(x[b]).all():
            return None
        dx = (x[b][:, i] - x[b][:, j]).T
        dc = (dx * dx).sum(1)
        uc = dc * dc / h2
        w = g[b][i] * (-(1.0 / k)) * np.exp(-uc) * (1.0 - 2.0 * uc)
        t = (2.0 * w)[:, None] * dx
        gr, n = _scatter(N, i, j, t)
        return gr, n, np.abs(t).max()
    grad, n, tmax = _finish(B, N, one)
    return dict(out=out, term=term, u=u, grad=grad, n=n, tmax=tmax)


def displacement(adv, ori, idx, k, g=None):
    """-> dict(theta [B,N], t [B,N,k] (theta_j - theta_i; NaN where j lies outside the cloud), out [B,N], grad, n, tmax);
    the gradient is 2 (adv - ori) dtheta, dtheta_i the sum of the pair terms (2 / k) (theta_j - theta_i) g_i: -t on i, +t on j"""
    adv, ori, idx = _np(adv, np.float64), _np(ori, np.float64), _np(idx)
    B, _, N = adv.shape
    g = np.ones((B, N)) if g is None else _np(g, np.float64)
    diff = adv - ori
    theta = (diff * diff).sum(1)
    j = idx[:, :, 1:k + 1].astype(np.int64)
    inside = (j >= 0) & (j < N)
    t = np.where(inside, np.take_along_axis(theta, np.where(inside, j, 0).reshape(B, N * k), 1).reshape(B, N, k)
                 - theta[:, :, None], np.nan)
    out = (t * t).sum(2) / k

    def one(b):
        i, jj = _pairs(idx[b], k)
        if _oob(jj, N) or not np.isfinite(theta[b]).all():
            return None
        tt = (2.0 / k) * (theta[b][jj] - theta[b][i]) * g[b][i]
        dth, n = _scatter(N, jj, i, tt)                      # (+t on j, -t on i)
        return 2.0 * diff[b] * dth[None, :], n, np.abs(tt).max()
    grad, n, tmax = _finish(B, N, one)
    return dict(theta=theta, t=t, out=out, grad=grad, n=n, tmax=tmax)


def normal_grad(x, nrm, idx, k, g=None):
    """d (sum g . corresponding_normal_loss) / d x with the table held fixed -> dict(grad, n, tmax)"""
    x, nrm, idx = _np(x, np.float64), _np(nrm, np.float64), _np(idx)
    B, _, N = x.shape
    g = np.ones((B, N)) if g is None else _np(g, np.float64)

    def one(b):
        i, j = _pairs(idx[b], k)
        if _oob(j, N) or not (np.isfinite(x[b]).all() and np.isfinite(nrm[b]).all()):
            return None
        v = (x[b][:, j] - x[b][:, i]).T
        r = np.sqrt((v * v).sum(1))
        inv = 1.0 / np.maximum(r, NORM_EPS)
        u = v * inv[:, None]
        n_i = nrm[b][:, i].T
        t = (u * n_i).sum(1)
        c = -(np.sign(t) * inv / k) * g[b][i]
        tt = np.where(r > NORM_EPS, t, 0.0)                 # (clamped length: v / eps is linear in v)
        term = c[:, None] * (n_i - tt[:, None] * u)
        gr, n = _scatter(N, i, j, term)
        return gr, n, np.abs(term).max()
    grad, n, tmax = _finish(B, N, one)
    return dict(grad=grad, n=n, tmax=tmax)


def grad_bound(ref, scale=None):
    """The header's promise per element: n_i 2^(ex - 41) (times `scale` [B,3,N]: displacement_loss's 2 |adv - ori|) +
    2^-24 |ref_i|, ex = ilogb(tmax) (0 where no term is non-zero).  NaN instances get bound 0 (they are compared apart)."""
    tmax = np.nan_to_num(ref["tmax"])
    ex = np.where(tmax > 0, np.frexp(tmax)[1] - 1.0, 0.0)   # ilogb
    first = ref["n"][:, None, :] * np.exp2(ex - 41)[:, None, None]
    if scale is not None:
        first = first * scale
    return np.nan_to_num(first + 2.0 ** -24 * np.abs(ref["grad"]))
