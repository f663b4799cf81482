"""CPU-only: the numpy restatement of three_nn / three_interpolate / three_interpolate_grad (tests/_three_ref.py) against
the fixture made by the reference's own ThreeNN / ThreeInterpolate / PointnetFPModule (tests/golden/geoa3_golden_fp.npz), and
the properties of the search it must have before a GPU kernel is held to it bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests import _three_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = ["gauss", "nofeat", "lattice"]
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def gf():
    return np.load(os.path.join(REPO, "tests", "golden", "geoa3_golden_fp.npz"), allow_pickle=False)


def test_fixture_lists_its_cases(gf):
    assert list(gf["fp/cases"]) == CASES


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_fixture(gf, tag):
    pre = "fp/%s/" % tag
    d2, idx = R.three_nn(gf[pre + "unknown"], gf[pre + "known"])
    assert idx.dtype == np.int32 and np.array_equal(idx, gf[pre + "idx"])
    assert np.array_equal(torch.sqrt(torch.from_numpy(d2)).numpy(), gf[pre + "dist"])   # (pointnet2_utils.py:125)
    out = R.three_interpolate(gf[pre + "known_feats"], gf[pre + "idx"], gf[pre + "weight"])
    assert out.dtype == np.float32 and np.array_equal(out, gf[pre + "interp"])
    m = gf[pre + "known"].shape[1]
    g, cnt, mag = R.three_interpolate_grad64(gf[pre + "cot_interp"], gf[pre + "idx"], gf[pre + "weight"], m)
    assert np.array_equal(g.astype(np.float32), gf[pre + "interp_grad_feats"])
    assert not gf[pre + "interp_grad_weight"].any()          # the reference gives the weights a zero gradient
    assert int(cnt.sum()) == 3 * gf[pre + "idx"].shape[0] * gf[pre + "idx"].shape[1]
    assert (np.abs(g) <= mag * (1 + 1e-12)).all()
    # the weights are what pointnet2_modules.py:187-189 makes of the distances
    rec = (1.0 / (gf[pre + "dist"] + np.float32(1e-8))).astype(np.float32)
    np.testing.assert_allclose(rec / rec.sum(2, keepdims=True), gf[pre + "weight"], rtol=1e-6)


@pytest.mark.parametrize("contract", [False, True])
def test_search_agrees_with_float64_sort_where_separated(contract):
    rng = np.random.default_rng(5)
    unknown = rng.standard_normal((2, 90, 3)).astype(np.float32)
    known = rng.standard_normal((2, 50, 3)).astype(np.float32)
    d2, idx = R.three_nn(unknown, known, contract)
    d64 = ((unknown[:, :, None, :].astype(np.float64) - known[:, None, :, :].astype(np.float64)) ** 2).sum(-1)
    order = np.argsort(d64, axis=-1, kind="stable")
    srt = np.take_along_axis(d64, order, -1)
    # float32 evaluation of a squared distance: each difference, product and sum rounded -> relative error below 8 * 2^-24
    tol = 8 * U32 * srt[..., 3]
    sep = (np.diff(srt[..., :4], axis=-1) > 2 * tol[..., None]).all(-1)
    assert sep.mean() > 0.9
    assert np.array_equal(idx[sep], order[..., :3][sep])
    assert (np.abs(d2 - srt[..., :3]) <= tol[..., None]).all()
    assert (np.diff(d2, axis=-1) >= 0).all()


def test_ties_are_ascending_in_index():
    ax = np.array([-1.0, 0.0, 1.0], dtype=np.float32)
    known = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(1, 27, 3)
    known = np.concatenate([known, known[:, :6]], 1)                     # exact duplicates of the first six
    rng = np.random.default_rng(6)
    unknown = np.concatenate([known[:, ::2], (np.round(rng.standard_normal((1, 40, 3)) * 2) / 2).astype(np.float32)], 1)
    for contract in (False, True):
        d2, idx = R.three_nn(unknown, known, contract)
        tie = d2[..., :-1] == d2[..., 1:]
        assert tie.sum() > 20
        assert (idx[..., :-1][tie] < idx[..., 1:][tie]).all()
        # nothing earlier in the scan is as good as a selected point's successor: the selection is the stable sort's
        d_all = ((unknown[:, :, None, :] - known[:, None, :, :]) ** 2).sum(-1)     # exact on this lattice
        order = np.argsort(d_all, axis=-1, kind="stable")[..., :3]
        assert np.array_equal(idx, order)


def test_fewer_than_three_known_points():
    rng = np.random.default_rng(7)
    unknown = rng.standard_normal((2, 5, 3)).astype(np.float32)
    for m in (1, 2):
        d2, idx = R.three_nn(unknown, rng.standard_normal((2, m, 3)).astype(np.float32))
        assert np.isposinf(d2[..., m:]).all() and not idx[..., m:].any()
        assert np.isfinite(d2[..., :m]).all()


def test_nan_and_inf_distances_are_never_selected():
    rng = np.random.default_rng(8)
    unknown = rng.standard_normal((1, 6, 3)).astype(np.float32)
    known = rng.standard_normal((1, 7, 3)).astype(np.float32)
    known[0, 0, 1] = np.nan
    known[0, 3, 2] = np.inf
    d2, idx = R.three_nn(unknown, known)
    assert np.isfinite(d2).all() and not np.isin(idx, (0, 3)).any()
    unknown[0, 2, 0] = np.nan
    d2, idx = R.three_nn(unknown, known)
    assert np.isposinf(d2[0, 2]).all() and not idx[0, 2].any()


# ------------------------------------------------------------------------------------------ three_interpolate_grad32
def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("C", [1, 65])
@pytest.mark.parametrize("kind", ["same3", "sparse"])
def test_grad32_stays_within_the_summation_bound_of_the_float64_sum(kind, C):
    from tests.test_gpu_fp import _grad_inputs
    g, idx, weight, m = _grad_inputs(kind, C, seed=40 + C)
    ref, cnt, mag = R.three_interpolate_grad64(g, idx, weight, m)
    out = R.three_interpolate_grad32(g, idx, weight, m)
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert (np.abs(out.astype(np.float64) - ref) <= (cnt + 2) * 2.0 ** -24 * mag).all()
    assert not _bits(out)[np.broadcast_to(cnt == 0, out.shape)].any()   # +0.0 where nobody points


@pytest.mark.parametrize("kind,C", [(k, c) for k in ("same3", "sparse") for c in (1, 8, 9, 65)] + [("hub", 3)])
def test_grad32_bits_depend_on_the_order(kind, C):
    """The bit test of tests/test_gpu_fp.py can see an order error: the same loop over DESCENDING e changes the bits of at
    least one element on every input that test uses (and stays within the summation bound, which no order can miss)."""
    from tests.test_gpu_fp import _grad_inputs, _hub_inputs
    if kind == "hub":
        g, idx, weight, m = _hub_inputs()
    else:
        g, idx, weight, m = _grad_inputs(kind, C, seed=40 + C)
    up = R.three_interpolate_grad32(g, idx, weight, m)
    down = R.three_interpolate_grad32(g, idx, weight, m, descending=True)
    changed = int((_bits(up) != _bits(down)).sum())
    print("three_interpolate_grad32 %s C=%d: %d of %d elements change bits in descending order" % (kind, g.shape[1], changed, up.size))
    assert changed > 0
    ref, cnt, mag = R.three_interpolate_grad64(g, idx, weight, m)
    assert (np.abs(down.astype(np.float64) - ref) <= (cnt + 2) * 2.0 ** -24 * mag).all()
