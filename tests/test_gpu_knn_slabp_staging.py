"""The position-list slab kernels' staging (cloud, old rows and sorted run are requested with every load in flight and a
compile-time trip count, the addresses clamped): the shapes at which unrolled, clamped staging goes wrong -- a ragged last
load of every batch (N = 17, 20, 255, 257, 1000, 1023), whole batches (256, 1024), K at the unroll bound (20), K = 1 and
N = K -- with three kinds of prior, against the all-pairs route on the same input: distances as bit patterns, indices exactly.

knn_slabp_kernel<32, false> is reached with method 4 at three instances for every N <= 1024, K <= 20.  The dispatcher sends
no such shape to knn_slabp_kernel<56, true> (tests/test_knn_self_route.py): that kernel -- it shares the sorted run's staging,
not the cloud's and the old rows' -- is run with the same method at the nearest shapes that reach it, K = 21 for the
same N and N = 1025 for the same K.  Every case asserts its route (geoa3_debug_knn_self_route)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
ALLPAIRS, SLABP32, SLABP56 = 0, 5, 6     # GEOA3_KNN_ROUTE_* of include/geoa3_hip_debug.h
B, METHOD = 3, 4                          # GEOA3_KNN_SELF_SLAB_POSITIONS
SIZES = (17, 20, 255, 256, 257, 1000, 1023, 1024)
CASES = ([(SLABP32, N, K) for N in SIZES for K in (1, 17, 20) if K <= N] +
         [(SLABP56, N, 21) for N in SIZES if N >= 21] + [(SLABP56, 1025, K) for K in (1, 17, 20)])


def _bits(d):
    return d.contiguous().view(torch.int32)


def _cloud(N, seed):
    g = torch.Generator().manual_seed(seed)
    pc = torch.randn(B, 3, N, generator=g) * torch.tensor([1.0, 0.6, 0.3]).view(1, 3, 1)
    if N > 12:
        pc[:, :, 5] = pc[:, :, 4]          # duplicate points: exact ties, the lower index first
        pc[:, :, 9] = pc[:, :, 11]
    return pc


def _check(ops, lib, route, pc, priors):
    _, _, N = pc.shape
    K = priors[0][1].shape[2]
    scratch = ops.knn_self_scratch(B, N, "cuda")
    assert lib.geoa3_debug_knn_self_route(B, N, K, METHOD, 1, 1) == route
    assert lib.geoa3_debug_knn_self_route(B, N, K, METHOD, 0, 1) == ALLPAIRS
    rd, ri = ops.knn_self_planar(pc, K, prior=None, scratch=scratch, method=METHOD)      # the all-pairs route
    for name, prior in priors:
        d, i = ops.knn_self_planar(pc, K, prior=prior, scratch=scratch, method=METHOD)
        assert torch.equal(i, ri), (name, N, K)
        assert torch.equal(_bits(d), _bits(rd)), (name, N, K)
    return rd, ri, scratch


@pytest.fixture(scope="module")
def env():
    from geoa3_amd import _lib, ops
    assert torch.cuda.is_available(), "needs the MI355X"
    return ops, _lib.load()


@pytest.mark.parametrize("route,N,K", CASES)
def test_staged_search_matches_all_pairs(env, route, N, K):
    ops, lib = env
    pc = _cloud(N, seed=1000 * K + N)
    near = (pc + 0.01 * torch.randn(B, 3, N, generator=torch.Generator().manual_seed(N))).contiguous().cuda()
    pc = pc.contiguous().cuda()
    _, perturbed = ops.knn_planar(near, near, K)                 # the table of a perturbed copy of the cloud
    broken = perturbed.clone()                                    # rows without a usable radius: the full scan
    broken[:, ::3, K // 2] = -1
    broken[:, 1::5, K - 1] = N
    broken[1, :, 0] = N
    rd, ri, scratch = _check(ops, lib, route, pc, [("perturbed", perturbed), ("out of range", broken)])
    # the previous call's own output, as the loop hands it over
    _, own = ops.knn_self_planar(pc, K, prior=perturbed, scratch=scratch, method=METHOD)
    d, i = ops.knn_self_planar(pc, K, prior=own, scratch=scratch, method=METHOD)
    assert torch.equal(i, ri) and torch.equal(_bits(d), _bits(rd))


@pytest.mark.parametrize("route,N,K", [(SLABP32, 257, 17), (SLABP32, 20, 20), (SLABP56, 257, 21)])
def test_an_instance_whose_points_all_coincide(env, route, N, K):
    ops, lib = env
    pc = _cloud(N, seed=7)
    pc[1] = pc[1, :, :1]                                          # every point of instance 1 is its first point
    pc = pc.contiguous().cuda()
    _, own = ops.knn_planar(pc, pc, K)
    shifted = ((own + 1) % N).to(torch.int32)                     # any in-range rows give the same (zero) radius there
    _check(ops, lib, route, pc, [("own", own), ("shifted", shifted)])
