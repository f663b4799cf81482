"""CPU-only: where reg_bwd_kernel (csrc/geom_reg.hip) and uniform_main_kernel (csrc/geom_uniform.hip) keep their per-point
fixed-point gradient sums -- in LDS beside the cloud or in the workspace (geoa3_debug_reg_route, geoa3_debug_uniform_route:
pure host functions, the predicates the launches themselves call) -- and that the workspace queries hold the sums wherever
the route says WORKSPACE.  The boundaries are written out by hand from the formulas as they stand; they must not move.

reg_bwd_kernel, dynamic LDS limit 160 KiB - 6144 = 157696 bytes:
  kNN_smoothing_loss   37 N bytes (3 int64 sums + 3 floats + 1 mask byte per point): 37 * 4262 = 157694, 37 * 4263 = 157731
  repulsion / normal   36 N bytes:                                                   36 * 4380 = 157680, 36 * 4381 = 157716
  displacement_loss    16 N bytes (1 int64 sum + theta in double): 131072 at N = 8192, the largest cloud taken
uniform_main_kernel, dynamic LDS limit 160 KiB - 1024 = 162816 bytes, 36 N + 32 nsmax bytes with the sums in LDS
(3 int64 + 3 floats per point, 8 index rows of nsmax = int(N * 4 * max percentage) ints):
  (0.004,)             N = 4459: ns 71, 160524 + 2272 = 162796;  N = 4460: ns 71, 160560 + 2272 = 162832
  the default five     N = 4337: ns int(208.176) = 208, 156132 + 6656 = 162788;  N = 4338: ns 208, 156168 + 6656 = 162824
geoa3_uniform_loss_workspace_bytes does not know the percentages: it adds the sums from 36 N + 32 * 512 > 162816 on, that
is from N = 4068 (36 * 4067 + 16384 = 162796)."""
import ctypes

import pytest

from geoa3_amd import _lib

LDS, WORKSPACE, REFUSED = 0, 1, 2          # GEOA3_REG_ROUTE_* / GEOA3_UNIFORM_ROUTE_* of include/geoa3_hip_debug.h
SMOOTH, REPULSE, DISPLACE, NORMAL = range(4)   # the order of the kernel's enum
EINVAL, ENOSUPPORT = -1, -3
DEFAULT = (0.004, 0.006, 0.008, 0.010, 0.012)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


def _uni(lib, N, pcts=DEFAULT, B=2, radius=1.0, k=2):
    arr = (ctypes.c_double * max(len(pcts), 1))(*pcts)
    return lib.geoa3_debug_uniform_route(B, N, arr, len(pcts), radius, k)


def _align256(x):
    return (x + 255) & ~255


def test_route_values_are_the_headers():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "geoa3_hip_debug.h")).read()
    assert dict(re.findall(r"#define GEOA3_REG_ROUTE_(\w+) (\d+)", hdr)) == {"LDS": "0", "WORKSPACE": "1", "REFUSED": "2"}
    assert dict(re.findall(r"#define GEOA3_UNIFORM_ROUTE_(\w+) (\d+)", hdr)) == {"LDS": "0", "WORKSPACE": "1"}


@pytest.mark.parametrize("mode,N,route", [
    (SMOOTH, 5, LDS), (SMOOTH, 4262, LDS), (SMOOTH, 4263, WORKSPACE), (SMOOTH, 8192, WORKSPACE),
    (REPULSE, 4262, LDS), (REPULSE, 4263, LDS), (REPULSE, 4380, LDS), (REPULSE, 4381, WORKSPACE), (REPULSE, 8192, WORKSPACE),
    (NORMAL, 4263, LDS), (NORMAL, 4380, LDS), (NORMAL, 4381, WORKSPACE), (NORMAL, 8192, WORKSPACE),
    (DISPLACE, 4263, LDS), (DISPLACE, 4381, LDS), (DISPLACE, 8192, LDS),
    (SMOOTH, 8193, REFUSED), (REPULSE, 8193, REFUSED), (DISPLACE, 8193, REFUSED), (NORMAL, 8193, REFUSED)])
def test_reg_route_boundaries(lib, mode, N, route):
    assert lib.geoa3_debug_reg_route(mode, N, 4) == route


def test_reg_route_does_not_depend_on_k_and_refuses_what_the_entry_points_refuse(lib):
    for k in (1, 16, 63):
        assert lib.geoa3_debug_reg_route(SMOOTH, 4262, k) == LDS and lib.geoa3_debug_reg_route(SMOOTH, 4263, k) == WORKSPACE
    assert lib.geoa3_debug_reg_route(SMOOTH, 64, 63) == LDS
    for mode, N, k in ((SMOOTH, 64, 64), (SMOOTH, 4, 4), (SMOOTH, 100, 0), (SMOOTH, 0, 1), (-1, 100, 4), (4, 100, 4)):
        assert lib.geoa3_debug_reg_route(mode, N, k) == REFUSED, (mode, N, k)


def test_reg_route_has_one_boundary_per_mode(lib):
    """every N the entry points take: LDS up to the boundary, WORKSPACE beyond, nothing else"""
    for mode, last in ((SMOOTH, 4262), (REPULSE, 4380), (DISPLACE, 8192), (NORMAL, 4380)):
        got = [lib.geoa3_debug_reg_route(mode, N, 1) for N in range(2, 8193)]
        assert got == [LDS] * (last - 1) + [WORKSPACE] * (8192 - last), mode


def test_reg_workspace_holds_the_sums_wherever_a_mode_takes_the_workspace(lib):
    for B, k in ((1, 4), (3, 16)):
        for N in (20, 4262, 4263, 4380, 4381, 8192):
            table = 2 * _align256(B * N * (k + 1) * 4)
            want_sums = any(lib.geoa3_debug_reg_route(m, N, k) == WORKSPACE for m in range(4))
            assert want_sums == (N >= 4263)
            assert lib.geoa3_reg_workspace_bytes(B, N, k) == table + (B * 3 * N * 8 if want_sums else 0), (B, N, k)
    assert lib.geoa3_reg_workspace_bytes(1, 8193, 4) == 0


@pytest.mark.parametrize("pcts,N,route", [
    ((0.004,), 188, LDS), ((0.004,), 4459, LDS), ((0.004,), 4460, WORKSPACE), ((0.004,), 8192, WORKSPACE),
    (DEFAULT, 188, LDS), (DEFAULT, 4293, LDS), (DEFAULT, 4337, LDS), (DEFAULT, 4338, WORKSPACE), (DEFAULT, 8192, WORKSPACE),
    ((0.0625,), 2048, LDS),                                   # ns = 512, the limit
    (DEFAULT, 8193, ENOSUPPORT), (DEFAULT, 187, ENOSUPPORT),  # ns = int(187 * 0.016) = 2 < k + 1
    ((0.0625,), 2064, ENOSUPPORT),                            # ns = 516 > 512
    (DEFAULT, 19, ENOSUPPORT),                                # npoint = 0
    ((0.0,), 1024, EINVAL), ((), 1024, EINVAL), (DEFAULT, 0, EINVAL)])
def test_uniform_route_boundaries(lib, pcts, N, route):
    assert _uni(lib, N, pcts) == route


def test_uniform_route_is_the_formula_at_every_size(lib):
    for pcts in ((0.004,), DEFAULT):
        for N in range(188, 8193):
            ns = int(N * (max(pcts) * 4))
            assert _uni(lib, N, pcts) == (LDS if 36 * N + 32 * ns <= 160 * 1024 - 1024 else WORKSPACE), (pcts, N)


def test_uniform_route_refusals(lib):
    assert _uni(lib, 1024, k=9) == ENOSUPPORT and _uni(lib, 1024, k=0) == EINVAL
    assert _uni(lib, 1024, pcts=(0.01,) * 9) == ENOSUPPORT and _uni(lib, 1024, pcts=(0.01,) * 8) == LDS
    assert _uni(lib, 1024, radius=0.0) == EINVAL and _uni(lib, 1024, B=0) == EINVAL
    assert lib.geoa3_debug_uniform_route(2, 1024, None, 1, 1.0, 2) == EINVAL


def test_uniform_workspace_holds_the_sums_wherever_the_route_takes_the_workspace(lib):
    for B in (1, 3):
        for N in (188, 4067, 4068, 4337, 4338, 4459, 4460, 8192):
            base = _align256(B * 8 * 8) + _align256(B * N * 12) + _align256(B * N * 4)
            have_sums = N >= 4068
            assert lib.geoa3_uniform_loss_workspace_bytes(B, N) == base + (B * 3 * N * 8 if have_sums else 0), (B, N)
    # every route to the workspace lies beyond the size from which the query includes the sums, whatever the percentages
    for pcts in ((0.004,), DEFAULT, (0.0004,), (0.03,)):
        for N in range(2500, 4068):
            assert _uni(lib, N, pcts, k=1) != WORKSPACE, (pcts, N)
