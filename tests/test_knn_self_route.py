"""CPU-only: which search geoa3_knn_self runs (geoa3_debug_knn_self_route: a pure host function, no GPU work) and how much
scratch it asks for.  Every route returns the same bits, so no value test can see a dispatcher that sends the attack loop
to the slower kernel: the table below is the dispatcher as it stood before the routing became a function of its own
(the `if` chain of geoa3_knn_self), written out by hand -- not derived from the code under test."""
import pytest

from geoa3_amd import _lib

ALLPAIRS, CELLGRID, SLAB40, SLAB72, SLAB96, SLABP32, SLABP56 = range(7)   # GEOA3_KNN_ROUTE_* of include/geoa3_hip_debug.h
EINVAL = -1

# (B, N, K, method) -> route; a prior and an aligned scratch buffer are given
ROUTES = [
    (250, 1024, 17, 0, SLABP32),    # the attack loop (configs[1])
    (32, 1024, 17, 0, SLAB40),      # a small shard: 128 workgroups
    (128, 1024, 17, 0, SLAB40),     # 512 workgroups is not "more than 512"
    (129, 1024, 17, 0, SLABP32),
    (250, 1024, 17, 3, SLAB40),
    (3, 1024, 17, 4, SLABP32),
    (3, 1024, 20, 4, SLABP32),
    (3, 1024, 21, 4, SLABP56),
    (3, 1024, 40, 4, SLABP56),
    (3, 1025, 17, 4, SLABP56),      # more than one staging chunk
    (250, 1024, 21, 0, CELLGRID),
    (250, 1024, 21, 1, SLABP56),
    (3, 1024, 21, 1, SLAB72),
    (3, 1024, 41, 1, SLAB96),
    (250, 1024, 41, 4, SLAB96),     # no position-list kernel holds more than 40
    (250, 2047, 17, 0, SLABP56),
    (3, 2047, 17, 0, SLAB40),
    (250, 2048, 17, 0, CELLGRID),
    (3, 300, 64, 2, CELLGRID),
    (250, 1024, 17, 7, SLABP32),    # an unknown method behaves as 1
    (2, 8192, 5, 1, SLAB40),
    (2, 8193, 5, 1, ALLPAIRS),      # more points than the counting sort holds
    (3, 10, 17, 1, ALLPAIRS),       # K > N
]

# geoa3_knn_self_scratch_bytes as the library returned it before the two searches shared one carving function
SCRATCH_BYTES = [((1, 1), 17408), ((3, 300), 65280), ((250, 1024), 8288000), ((250, 4096), 20576000), ((2, 8192), 295680)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


def test_route_values_are_the_headers():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "geoa3_hip_debug.h")).read()
    assert dict(re.findall(r"#define GEOA3_KNN_ROUTE_(\w+) (\d+)", hdr)) == {
        "ALLPAIRS": "0", "CELLGRID": "1", "SLAB40": "2", "SLAB72": "3", "SLAB96": "4", "SLABP32": "5", "SLABP56": "6"}


@pytest.mark.parametrize("B,N,K,method,route", ROUTES)
def test_route_follows_the_dispatcher_table(lib, B, N, K, method, route):
    assert lib.geoa3_debug_knn_self_route(B, N, K, method, 1, 1) == route


def test_nothing_to_prune_with_is_all_pairs(lib):
    for method in range(5):
        assert lib.geoa3_debug_knn_self_route(250, 1024, 17, method, 0, 1) == ALLPAIRS   # no prior
        assert lib.geoa3_debug_knn_self_route(250, 1024, 17, method, 1, 0) == ALLPAIRS   # no (or a misaligned) scratch buffer


def test_refused_sizes(lib):
    assert lib.geoa3_debug_knn_self_route(250, 1024, 0, 0, 1, 1) == EINVAL
    assert lib.geoa3_debug_knn_self_route(250, 1024, 65, 0, 1, 1) == EINVAL
    assert lib.geoa3_debug_knn_self_route(0, 1024, 17, 0, 1, 1) == EINVAL
    assert lib.geoa3_debug_knn_self_route(250, 1024, 64, 0, 1, 1) == CELLGRID


@pytest.mark.parametrize("shape,nbytes", SCRATCH_BYTES)
def test_scratch_bytes_are_unchanged(lib, shape, nbytes):
    assert lib.geoa3_knn_self_scratch_bytes(*shape) == nbytes
