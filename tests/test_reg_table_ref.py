"""CPU-only: tests/_reg_table_ref.py (the float64 restatement of csrc/geom_reg.hip that takes the table as given) against
tests/_reg_ref.py (pinned to the reference's own values by tests/test_reg_ref.py) on consistent tables -- those of
_reg_ref.knn_self(..., stable=True) with their own distances -- to 1e-12 relative PER ELEMENT (a gradient, the sum of n_i
pair terms added in another order than autograd's, also gets n_i 2^-52 |t|max: one double rounding of the largest term per
term summed), against central differences in float64, and its own rules for the tables no search returns."""
import numpy as np
import pytest
import torch

from tests import _reg_ref as R
from tests import _reg_table_ref as TR

RTOL = 1e-12


def _cloud(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, N, generator=g) * 0.6 - 0.3
    return x.double()     # (float32 values: what the kernels see)


def _close(a, b, what, r=None, scale=None):
    """per element; r: the restatement's dict of a gradient (n, tmax) for the summation-order floor (scale: displacement_loss's
    2 |adv - ori|, its sum being d theta)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bound = RTOL * np.abs(b)
    if r is not None:
        floor = r["n"][:, None, :] * 2.0 ** -52 * r["tmax"][:, None, None]
        bound = bound + (floor if scale is None else floor * scale)
    bad = np.abs(a - b) > bound
    assert not bad.any(), (what, float(np.abs(a - b)[bad].max()), float(np.abs(b)[bad].min()))


@pytest.mark.parametrize("B,N,k", [(2, 2, 1), (3, 64, 63), (2, 200, 4), (2, 513, 5)])
def test_equals_autograd_on_consistent_tables(B, N, k):
    x = _cloud(B, N, 100 + N)
    ori = _cloud(B, N, 200 + N)
    nrm = torch.nn.functional.normalize(_cloud(B, N, 300 + N), dim=1)
    gen = torch.Generator().manual_seed(N)
    gp = (torch.rand(B, N, generator=gen) - 0.3).double()
    gb = (torch.rand(B, generator=gen) - 0.3).double()
    d, idx = R.knn_self(x, k + 1, stable=True)
    coef = 0.3
    v, gr = R.value_and_grad(R.kNN_smoothing_loss, x, gb, k, coef)
    s, thr, cond = R.smoothing_parts(x, k, coef)
    r = TR.smoothing(x, d, idx, k, coef, gb)
    assert np.array_equal(r["mask"], cond.numpy()) and (N == 2 or cond.any())
    _close(r["s"], s, "s"), _close(r["thr"], thr, "thr"), _close(r["loss"], v, "smoothing"), _close(r["grad"], gr, "dsmoothing", r)
    h = 0.2
    v, gr = R.value_and_grad(R.repulsion_loss, x, gp, k, h)
    r = TR.repulsion(x, d, idx, k, h * h, gp)
    _close(r["out"], v, "repulsion"), _close(r["grad"], gr, "drepulsion", r)
    do, io = R.knn_self(ori, k + 1, stable=True)
    v, gr = R.value_and_grad(R.displacement_loss, x, gp, ori, k)
    r = TR.displacement(x, ori, io, k, gp)
    _close(r["out"], v, "displacement")
    _close(r["grad"], gr, "ddisplacement", r, 2 * np.abs((x - ori).numpy()))
    v, gr = R.value_and_grad(R.corresponding_normal_loss, x, gp, nrm, k)
    r = TR.normal_grad(x, nrm, idx, k, gp)
    _close(r["grad"], gr, "dnormal", r)
    # the counts: a search table names every point k times as i and never itself
    for q in (TR.repulsion(x, d, idx, k, h * h), r):
        assert int(q["n"].sum()) == 2 * B * N * k and (q["n"] >= k).all() and (q["tmax"] > 0).all()


def _random_table(B, N, k, ld, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, (B, N, ld))
    idx[:, :10, 1] = idx[:, :10, 2]                        # a repeated index
    idx[:, 10:20, 1:] = np.arange(10, 20)[None, :, None]   # the point itself
    return idx


def _table_dists(x, idx):
    x = np.asarray(x, np.float64)
    B, _, N = x.shape
    nb = np.take_along_axis(x[:, :, None, :], np.broadcast_to(idx[:, None], (B, 3) + idx.shape[1:]), 3)
    return ((x[:, :, :, None] - nb) ** 2).sum(1)


def test_repulsion_and_displacement_agree_with_central_differences():
    B, N, k, h2 = 2, 40, 3, 0.2 ** 2
    x, ori = _cloud(B, N, 1).numpy(), _cloud(B, N, 2).numpy()
    idx = _random_table(B, N, k, k + 3, 3)
    g = np.random.default_rng(4).random((B, N)) - 0.3
    rep = lambda y: float((g * TR.repulsion(y, _table_dists(y, idx), idx, k, h2)["out"]).sum())
    dis = lambda y: float((g * TR.displacement(y, ori, idx, k)["out"]).sum())
    for f, grad in ((rep, TR.repulsion(x, _table_dists(x, idx), idx, k, h2, g)["grad"]),
                    (dis, TR.displacement(x, ori, idx, k, g)["grad"])):
        num, eps = np.zeros_like(x), 1e-6
        for pos in np.ndindex(*x.shape):
            a, b = x.copy(), x.copy()
            a[pos] += eps
            b[pos] -= eps
            num[pos] = (f(a) - f(b)) / (2 * eps)
        assert np.abs(num - grad).max() <= 1e-7 * np.abs(grad).max()


def test_only_columns_1_to_k_are_read():
    B, N, k = 2, 50, 4
    x, ori, nrm = _cloud(B, N, 5), _cloud(B, N, 6), _cloud(B, N, 7)
    idx = _random_table(B, N, k, k + 3, 8)
    d = _table_dists(x, idx)
    idx2, d2 = idx.copy(), d.copy()
    idx2[:, :, 0], idx2[:, :, k + 1:] = N + 5, -7
    d2[:, :, 0], d2[:, :, k + 1:] = np.nan, np.nan
    for a, b in ((TR.smoothing(x, d, idx, k, 0.3), TR.smoothing(x, d2, idx2, k, 0.3)),
                 (TR.repulsion(x, d, idx, k, 0.04), TR.repulsion(x, d2, idx2, k, 0.04)),
                 (TR.displacement(x, ori, idx, k), TR.displacement(x, ori, idx2, k)),
                 (TR.normal_grad(x, nrm, idx, k), TR.normal_grad(x, nrm, idx2, k))):
        for key in a:
            assert np.array_equal(a[key], b[key]) and not np.isnan(a[key]).any(), key


def test_counts_of_a_hub_and_of_self_pairs():
    B, N, k = 1, 30, 3
    x = _cloud(B, N, 9)
    hub = np.full((B, N, k + 1), 7)
    r = TR.repulsion(x, _table_dists(x, hub), hub, k, 0.04)
    want = np.full(N, k)
    want[7] = (N - 1) * k                                   # (its own row holds only itself: nothing)
    assert np.array_equal(r["n"][0], want)
    own = np.broadcast_to(np.arange(N)[None, :, None], (B, N, k + 1)).copy()
    r = TR.repulsion(x, _table_dists(x, own), own, k, 0.04)
    assert not r["n"].any() and not r["grad"].any() and r["tmax"][0] == 0.0


def test_out_of_range_index_and_non_finite_distance():
    B, N, k = 3, 25, 2
    x, ori = _cloud(B, N, 10), _cloud(B, N, 11)
    idx = _random_table(B, N, k, k + 1, 12)
    d = _table_dists(x, idx)
    bad = idx.copy()
    bad[1, 3, 1], bad[1, 20, 2] = N, -1
    for clean, r in ((TR.repulsion(x, d, idx, k, 0.04), TR.repulsion(x, d, bad, k, 0.04)),
                     (TR.displacement(x, ori, idx, k), TR.displacement(x, ori, bad, k)),
                     (TR.smoothing(x, d, idx, k, 0.3), TR.smoothing(x, d, bad, k, 0.3))):
        assert np.isnan(r["grad"][1]).all() and np.array_equal(r["grad"][[0, 2]], clean["grad"][[0, 2]])
    r, clean = TR.displacement(x, ori, bad, k), TR.displacement(x, ori, idx, k)
    where = np.zeros((B, N), bool)
    where[1, 3] = where[1, 20] = True
    assert np.isnan(r["out"][where]).all() and np.array_equal(r["out"][~where], clean["out"][~where])
    for v in (np.nan, np.inf, -np.inf):
        dn = d.copy()
        dn[1, 5, 2] = v
        r, clean = TR.smoothing(x, dn, idx, k, 0.3), TR.smoothing(x, d, idx, k, 0.3)
        assert np.isnan(r["loss"][1]) and not r["mask"][1].any() and np.isnan(r["grad"][1]).all()
        assert np.array_equal(r["loss"][[0, 2]], clean["loss"][[0, 2]]) and np.array_equal(r["grad"][[0, 2]], clean["grad"][[0, 2]])


def test_grad_bound_uses_ilogb():
    ref = dict(tmax=np.array([1.0, 0.999999, 3.0, 0.0]), n=np.ones((4, 1), np.int64), grad=np.zeros((4, 3, 1)))
    assert np.array_equal(TR.grad_bound(ref)[:, 0, 0], [2.0 ** -41, 2.0 ** -42, 2.0 ** -40, 2.0 ** -41])
