"""CPU-only: which kernel geoa3_geo_loss_grad runs (geoa3_debug_geo_route: a pure host function that follows no pointer)
and how much scratch it asks for.  The routes of the sizes served before the two-pass kernels existed are written out by
hand from the dispatcher as it stood; they must not move (their bits would)."""
import pytest

from geoa3_amd import _lib

FUSED, BIG, LISTS, ATOMICS, WIDE, REFUSED = range(6)   # GEOA3_GEO_ROUTE_* of include/geoa3_hip_debug.h
EINVAL = -1
PTR = 0x1000   # "given": the route function tests pointers against NULL only


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


def _args(N, *, B=250, k=16, scratch=True, det=True, curv=True, Nr=0, grad=True, single_side=False, dis_type=1):
    a = _lib.GeoArgs(adv=PTR, ori=PTR, d_ao=PTR, i_ao=PTR, d_oa=None if single_side else PTR, i_oa=None if single_side else PTR,
                     B=B, N=N, k=k if curv else 0, Nr=Nr, dis_type=dis_type, single_side=int(single_side), w_dis=1.0, w_hd=0.1,
                     w_curv=1.0 if curv else 0.0, constrain=PTR, grad=PTR if grad else None, deterministic=int(det),
                     scratch=PTR if scratch else None)
    if curv:
        a.normal_ori = a.kappa_ori = a.knn_adv = PTR
    return a


def _route(lib, *a, **kw):
    import ctypes
    return lib.geoa3_debug_geo_route(ctypes.byref(_args(*a, **kw)))


def test_route_values_are_the_headers():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "geoa3_hip_debug.h")).read()
    assert dict(re.findall(r"#define GEOA3_GEO_ROUTE_(\w+) (\d+)", hdr)) == {
        "FUSED": "0", "BIG": "1", "LISTS": "2", "ATOMICS": "3", "WIDE": "4", "REFUSED": "5"}


# with the curvature term, deterministic, k = 16
@pytest.mark.parametrize("N,scratch,route", [
    (1024, True, FUSED), (1024, False, FUSED), (1025, True, BIG), (4096, True, BIG),
    (4096, False, LISTS), (4500, False, LISTS), (4500, True, LISTS),      # 4097..5839: one workgroup, scratch or not
    (5500, True, ATOMICS), (5500, False, ATOMICS), (5839, True, ATOMICS), (5839, False, ATOMICS),
    (5840, True, WIDE), (6001, True, WIDE), (8192, True, WIDE),
    (5840, False, REFUSED), (8192, False, REFUSED), (8193, True, REFUSED), (8193, False, REFUSED)])
def test_route_follows_the_dispatcher_table(lib, N, scratch, route):
    assert _route(lib, N, scratch=scratch) == route


def test_the_wide_route_serves_what_the_smaller_sizes_serve(lib):
    for kw in (dict(curv=False), dict(single_side=True), dict(dis_type=2), dict(Nr=8192), dict(grad=False), dict(det=False),
               dict(k=64), dict(k=1), dict(B=1)):
        assert _route(lib, 6144, **kw) == WIDE, kw
    assert _route(lib, 6144, k=65) == REFUSED
    assert _route(lib, 6144, dis_type=2, Nr=8192) == EINVAL     # norm_l2_loss needs equal sizes, at any size


def test_smaller_sizes_without_the_flags_stay_where_they_were(lib):
    assert _route(lib, 1024, det=False) == ATOMICS
    assert _route(lib, 2048, det=False) == ATOMICS
    assert _route(lib, 2048, curv=False) == LISTS               # no table: nothing for geo_big_kernel to stream
    assert _route(lib, 1024, k=40) == BIG and _route(lib, 1024, k=40, scratch=False) == LISTS   # (rows of 3 * 41 + 16 ids do not fit)
    assert _route(lib, 0) == EINVAL


@pytest.mark.parametrize("B,N", [(250, 4096), (3, 1500), (1, 64)])
def test_scratch_bytes_up_to_4096_points_are_the_record_table(lib, B, N):
    assert lib.geoa3_geo_scratch_bytes(B, N, 16) == 16 * B * N


def test_scratch_bytes_beyond_hold_records_and_partials(lib):
    for B, N in ((2, 5840), (250, 8192), (3, 4097)):
        n = lib.geoa3_geo_scratch_bytes(B, N, 32)
        assert n == lib.geoa3_debug_geo_wide_scratch_bytes(B, N) and 16 * B * N < n <= 16 * B * N + 512 * B
    assert lib.geoa3_debug_geo_wide_scratch_bytes(3, 1500) > 16 * 3 * 1500
