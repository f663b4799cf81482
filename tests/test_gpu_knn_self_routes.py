"""The position-list slab kernels the way the attack loop reaches them: chosen by geoa3_knn_self itself (methods 0 and 1)
because the launch is large -- tests/test_gpu_geometry.py runs three instances, where only method 4 gets there.
130 instances of 1001 points are 4 x 130 = 520 workgroups (more than the 512 of the dispatcher); the last workgroup of an
instance is ragged (233 live rows), and a staged run whose length is no multiple of four is padded with NaN points."""
import pytest
import torch

from oracle import geoa3_oracle as O

pytestmark = pytest.mark.gpu
SLABP32, SLABP56 = 5, 6     # GEOA3_KNN_ROUTE_* of include/geoa3_hip_debug.h
B, N = 130, 1001


@pytest.fixture(scope="module")
def clouds():
    from geoa3_amd import ops
    assert torch.cuda.is_available(), "needs the MI355X"
    ori, _ = O.make_synthetic_clouds(B, N, seed=5)
    adv = ori + 0.02 * torch.randn(B, 3, N, generator=torch.Generator().manual_seed(29))
    adv[:, :, 5] = adv[:, :, 4]                      # duplicate points: exact ties, the lower index first
    adv[:, :, 9] = adv[:, :, 11]
    return ops, ori.contiguous().cuda(), adv.contiguous().cuda(), ops.knn_self_scratch(B, N, "cuda")


@pytest.mark.parametrize("K,method,route", [(17, 0, SLABP32), (33, 1, SLABP56)])
def test_large_launches_take_the_position_list_kernels_and_match_all_pairs(clouds, K, method, route):
    from geoa3_amd import _lib
    ops, ori, adv, scratch = clouds
    assert _lib.load().geoa3_debug_knn_self_route(B, N, K, method, 1, 1) == route
    bd, bi = ops.knn_planar(adv, adv, K)
    _, clean = ops.knn_planar(ori, ori, K)
    bad = clean.clone()
    bad[:, ::3, 1] = bad[:, ::3, 0]                  # every third row degenerate: fewer than K distinct candidates in its radius
    for name, prior in (("clean", clean), ("degenerate", bad)):
        d, i = ops.knn_self_planar(adv, K, prior=prior, scratch=scratch, method=method)
        assert torch.equal(i, bi) and torch.equal(d, bd), name
