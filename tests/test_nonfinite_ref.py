"""tests/_nonfinite_ref.py -- the NaN / inf rule of the neighbour searches in float32 numpy -- against the oracle on finite
clouds (indices and distance bits) and against a table of eight points written by hand.  CPU only."""
import numpy as np
import pytest
import torch

from oracle import geoa3_oracle as O
from tests import _nonfinite_ref as R

NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("nq,nr,K", [(40, 40, 1), (77, 130, 5), (130, 77, 17), (600, 530, 3), (9, 5, 8)])
def test_finite_clouds_match_the_oracle(nq, nr, K):
    a, _ = O.make_synthetic_clouds(2, max(nq, nr), seed=nq + nr)
    q = (a[:, :, :nq] + 0.03 * torch.randn(2, 3, nq, generator=torch.Generator().manual_seed(K))).contiguous()
    r = a[:, :, :nr].clone()
    if nr > 8:
        r[:, :, 7] = r[:, :, 2]                      # an exact tie: the lower index first
    for b in range(2):
        od, oi = O.knn_points(q[b:b + 1].permute(0, 2, 1), r[b:b + 1].permute(0, 2, 1), min(K, nr))
        d, i = R.knn(q[b].numpy(), r[b].numpy(), K)
        keep = min(K, nr)
        assert np.array_equal(i[:, :keep], oi[0].numpy().astype(np.int32))
        assert R.same_bits(d[:, :keep], od[0].numpy())
        assert (i[:, keep:] == -1).all() and np.isposinf(d[:, keep:]).all()
        d1, i1 = R.nn1(q[b].numpy(), r[b].numpy())
        assert np.array_equal(i1, oi[0, :, 0].numpy().astype(np.int32)) and R.same_bits(d1, od[0, :, 0].numpy())


# the searched cloud: finite points, an exact duplicate (1 == 6), a NaN candidate (2), a +inf candidate (3)
TABLE_R = np.array([[0, 0, 0], [1, 0, 0], [NAN, 0, 0], [INF, 0, 0], [0, 2, 0], [0, 0, 3], [1, 0, 0], [-1, -1, -1]],
                   dtype=np.float32).T
# the queries and what each must give, worked out by hand (every value is exact in float32)
TABLE_Q = np.array([[0.25, 0, 0],      # finite: 0.0625 to point 0, 0.5625 to 1 and 6, 3.5625 to 7, 4.0625 to 4, 9.0625 to 5
                    [NAN, 0, 0],       # a NaN query: every distance NaN
                    [INF, 0, 0],       # +inf: NaN to the +inf candidate on the same axis (inf - inf) and to 2, +inf to the rest
                    [1, 0, 0]],        # on the duplicate pair: distance 0 to both
                   dtype=np.float32).T
NN1_WANT = [(0.0625, 0), (INF, 0), (INF, 0), (0.0, 1)]
KNN8_WANT = [
    [(0.0625, 0), (0.5625, 1), (0.5625, 6), (3.5625, 7), (4.0625, 4), (9.0625, 5), (INF, 3), (INF, -1)],   # 7 candidates for K = 8
    [(INF, -1)] * 8,
    [(INF, 0), (INF, 1), (INF, 4), (INF, 5), (INF, 6), (INF, 7), (INF, -1), (INF, -1)],                    # lowest indices first
    [(0.0, 1), (0.0, 6), (1.0, 0), (5.0, 4), (6.0, 7), (10.0, 5), (INF, 3), (INF, -1)],
]


def test_the_distance_is_nan_or_inf_where_the_rule_says():
    d = R.sqdist(TABLE_Q, TABLE_R)
    assert np.isnan(d[:, 2]).all() and np.isnan(d[1]).all()          # a NaN candidate, a NaN query
    assert np.isnan(d[2, 3])                                         # +inf against +inf on the same axis
    assert np.isposinf(d[2, [0, 1, 4, 5, 6, 7]]).all()               # +inf against finite
    assert np.isposinf(d[[0, 3], 3]).all()                           # finite against +inf


def test_nn1_on_the_table():
    d, i = R.nn1(TABLE_Q, TABLE_R)
    assert d.dtype == np.float32 and i.dtype == np.int32
    assert [(float(x), int(y)) for x, y in zip(d, i)] == NN1_WANT


def test_knn_on_the_table():
    d, i = R.knn(TABLE_Q, TABLE_R, 8)
    assert d.dtype == np.float32 and i.dtype == np.int32
    for q in range(4):
        assert [(float(x), int(y)) for x, y in zip(d[q], i[q])] == KNN8_WANT[q], q
    # a shorter list is the front of the longer one; K beyond the cloud pads
    d3, i3 = R.knn(TABLE_Q, TABLE_R, 3)
    assert np.array_equal(i3, i[:, :3]) and R.same_bits(d3, d[:, :3])
    d11, i11 = R.knn(TABLE_Q, TABLE_R, 11)
    assert np.array_equal(i11[:, :8], i) and (i11[:, 8:] == -1).all() and np.isposinf(d11[:, 8:]).all()


def test_knn_first_column_and_nn1_differ_only_where_nothing_is_finite():
    """K = 1 of knn takes a +inf distance (index of the first such candidate), nn1 never does (index 0): the two rules
    agree wherever a finite distance exists."""
    d1, i1 = R.nn1(TABLE_Q, TABLE_R)
    dk, ik = R.knn(TABLE_Q, TABLE_R, 1)
    fin = np.isfinite(d1)
    assert fin.tolist() == [True, False, False, True]
    assert np.array_equal(i1[fin], ik[fin, 0]) and R.same_bits(d1[fin], dk[fin, 0])
    assert ik[1, 0] == -1 and ik[2, 0] == 0 and i1[1] == 0 and i1[2] == 0


def test_same_bits_tells_signed_zero_and_equates_nans():
    assert R.same_bits(np.array([NAN, 1.0], np.float32), np.array([-NAN, 1.0], np.float32))
    assert not R.same_bits(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    assert not R.same_bits(np.array([NAN], np.float32), np.array([INF], np.float32))
