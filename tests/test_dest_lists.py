"""CPU-only: the scratch sizes of the three ordered scatter-add backward passes.  Both size functions answer from the one
layout of csrc/dest_lists.h (int32: start [B][M+1] | cursor [B][M] | bucket [B][E] | order [B][E]) and keep the ranges each
operator documents in include/geoa3_hip.h -- the corners on both sides of every limit."""
from geoa3_amd import _lib

INT_MAX = (1 << 31) - 1


def _lists_bytes(B, E, M):
    return 4 * B * ((M + 1) + M + 2 * E)


def _lib_built():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


def test_knn_scatter_scratch_bytes_formula_and_limits():
    f = _lib_built().geoa3_knn_scatter_scratch_bytes
    for B, E, M in [(1, 1, 1), (250, 1024 * 17, 1024), (3, 350, 18840), (65535, 1 << 15, 8), (1, INT_MAX - 256, 1),
                    (1, 1, INT_MAX - 257), (1 << 20, 2047, 2046)]:
        assert f(B, E, M) == _lists_bytes(B, E, M), (B, E, M)
    # B E and B (M + 1) stay below 2^31 - 256; nothing is empty
    for B, E, M in [(1 << 16, 1 << 15, 8), (1, INT_MAX - 255, 1), (1, 1, INT_MAX - 256), (1 << 20, 2048, 8), (1 << 20, 8, 2047),
                    (0, 8, 8), (2, 0, 8), (2, 8, 0), (-1, 8, 8)]:
        assert f(B, E, M) < 0, (B, E, M)


def test_three_interpolate_scratch_bytes_formula_and_limits():
    f = _lib_built().geoa3_pn2_three_interpolate_scratch_bytes
    nmax = (INT_MAX - 255) // 3
    # (no limit on B n here: 3 B n may pass 2^31)
    for B, n, m in [(1, 1, 1), (3, 300, 3), (16, 4096, 4096), (65535, 1 << 15, 8), (70000, 1 << 15, 8), (1, nmax, 1),
                    (2, 1, INT_MAX - 256)]:
        assert f(B, n, m) == _lists_bytes(B, 3 * n, m), (B, n, m)
    for B, n, m in [(1, nmax + 1, 1), (1, 1, INT_MAX - 255), (0, 8, 8), (2, 0, 8), (2, 8, 0), (2, -1, 8)]:
        assert f(B, n, m) < 0, (B, n, m)
