"""CPU-only: which launch sequence geoa3_pointnet_forward / _backward run (geoa3_debug_pointnet_route: the plan both entry
points compute once per call, as a bit mask; a pure host function that follows no pointer).  The expected routes are written
out by hand from the dispatcher as it stood when the decisions were spread over the file: they must not move.  And the
argument check both directions share, which runs before any HIP call (so it can be seen here, without a GPU)."""
import ctypes as C

import pytest

from geoa3_amd import _lib

# GEOA3_PN_ROUTE_* of include/geoa3_hip_debug.h
SPLIT, CHAIN, FUSE_TRUNK, FUSE_T64, FUSE_T3, PRE_LISTS, FC_KSPLIT, GRAM_F16, CLEAR_KEYS = (1 << i for i in range(9))
ALL = 511
NO_FUSE_BWD, NO_CHAIN, KEYS_CLEAN, NO_PRE_LISTS = 1, 2, 4, 8   # GEOA3_PN_* of include/geoa3_hip.h
EINVAL = -1
PTR = 0x1000   # "given" (and 256-byte aligned): the route function tests pointers against NULL only


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


def _fill(cls, **over):
    """every pointer given, every scale 1"""
    kw = {n: (PTR if t is _lib.vp else 1.0) for n, t in cls._fields_ if t in (_lib.vp, C.c_float)}
    kw.update(over)
    return cls(**kw)


def _weights(flags=0, f32=False, drop=(), classes=40, K3=3, K64=64):
    t3, t64 = _fill(_lib.TnetWeights, K=K3), _fill(_lib.TnetWeights, K=K64)
    w = _fill(_lib.PointNetWeights, classes=classes, t3=t3, t64=t64, flags=flags)
    if f32:
        w.w5h = None
    for name in drop:
        obj, _, field = name.rpartition(".")
        setattr(getattr(w, obj) if obj else w, field, None)
    return w


def _route(lib, B, N, **kw):
    return lib.geoa3_debug_pointnet_route(C.byref(_weights(**kw)), B, N)


def test_route_values_are_the_headers():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "geoa3_hip_debug.h")).read()
    assert dict(re.findall(r"#define GEOA3_PN_ROUTE_(\w+) (\d+)", hdr)) == {
        "SPLIT": "1", "CHAIN": "2", "FUSE_TRUNK": "4", "FUSE_T64": "8", "FUSE_T3": "16", "PRE_LISTS": "32",
        "FC_KSPLIT": "64", "GRAM_F16": "128", "CLEAR_KEYS": "256"}
    pub = open(os.path.join(os.path.dirname(__file__), "..", "include", "geoa3_hip.h")).read()
    assert dict(re.findall(r"#define GEOA3_PN_(NO_\w+|KEYS_CLEAN) (\d+)", pub)) == {
        "NO_FUSE_BWD": "1", "NO_CHAIN": "2", "KEYS_CLEAN": "4", "NO_PRE_LISTS": "8"}


FUSED = FUSE_TRUNK | FUSE_T64 | FUSE_T3


# B = 250, N = 1024 (the benchmark's shape), split-fp16 fragments given
@pytest.mark.parametrize("kw,route", [
    (dict(), ALL),
    (dict(flags=NO_FUSE_BWD), ALL & ~(FUSED | PRE_LISTS)),        # no fused backward: nobody would read the forward's lists
    (dict(flags=NO_CHAIN), ALL & ~CHAIN),
    (dict(flags=NO_PRE_LISTS), ALL & ~PRE_LISTS),
    (dict(flags=NO_FUSE_BWD | NO_CHAIN | NO_PRE_LISTS), SPLIT | FC_KSPLIT | GRAM_F16 | CLEAR_KEYS),
    (dict(flags=KEYS_CLEAN), ALL & ~CLEAR_KEYS),
    (dict(drop=("w4th",)), ALL & ~FUSE_TRUNK),                    # a missing transposed fragment unfuses its own layer pair only
    (dict(drop=("t3.w2th",)), ALL & ~FUSE_T3),
    (dict(drop=("t64.w2th",)), ALL & ~FUSE_T64),
    (dict(drop=("w4th", "t3.w2th", "t64.w2th")), ALL & ~FUSED),   # (the lists are still built: the condition never looked)
])
def test_route_follows_the_dispatcher_table(lib, kw, route):
    assert _route(lib, 250, 1024, **kw) == route


@pytest.mark.parametrize("flags", [0, NO_FUSE_BWD, NO_CHAIN, NO_PRE_LISTS, NO_FUSE_BWD | NO_CHAIN | NO_PRE_LISTS])
def test_f32_mode_clears_every_split_dependent_bit(lib, flags):
    """w5h NULL = fp32 MFMA throughout, whatever the flags say and whichever other fragments are given"""
    assert _route(lib, 250, 1024, f32=True, flags=flags) == FC_KSPLIT | CLEAR_KEYS
    assert _route(lib, 250, 1024, f32=True, flags=flags | KEYS_CLEAN) == FC_KSPLIT
    assert _route(lib, 250, 1024, f32=True, flags=flags, drop=("w4th", "t3.w2th", "t64.w2th", "t3.w3h", "t64.w3h")) == \
        FC_KSPLIT | CLEAR_KEYS


def test_hit_lists_up_to_4096_points(lib):
    assert _route(lib, 2, 4096) == ALL
    assert _route(lib, 2, 4097) == ALL & ~PRE_LISTS


@pytest.mark.parametrize("B,N,on", [(1, 511, False), (1, 512, True),      # 16 * 4096 <= 128 N
                                    (17, 60, False), (17, 61, True),      # 32 * 4096 = 131072 <= 17 * 128 N = 2176 N
                                    (16, 32, True), (16, 31, False),      # a full tile of rows: 4096 <= 128 N
                                    (3, 77, False), (3, 257, True)])      # the shapes of the GPU test of the flags
def test_fc_ksplit_when_G128_holds_the_partials(lib, B, N, on):
    """ceil(B / 16) * 16 * 4096 <= B * 128 * N, in every mode"""
    assert _route(lib, B, N) == (ALL if on else ALL & ~FC_KSPLIT)
    assert _route(lib, B, N, f32=True) == (FC_KSPLIT if on else 0) | CLEAR_KEYS


BAD_WEIGHTS = [dict(K3=4), dict(K3=64), dict(K64=3), dict(K64=0), dict(classes=0), dict(classes=-1)]


def test_route_refuses_what_the_entry_points_refuse(lib):
    assert lib.geoa3_debug_pointnet_route(None, 2, 1024) == EINVAL
    assert _route(lib, 0, 1024) == EINVAL and _route(lib, 2, 0) == EINVAL and _route(lib, -1, -1) == EINVAL
    for kw in BAD_WEIGHTS:
        assert _route(lib, 2, 1024, **kw) == EINVAL, kw
    assert _route(lib, 2, 1024) == ALL


def test_both_directions_share_the_argument_check_before_any_hip_call(lib):
    """No GPU here: a call that got as far as a HIP call could not return GEOA3_EINVAL.  (Only refused calls are made: the
    pointers are dummies.)"""
    def fwd(w, B=2, N=1024, ws=PTR, x=PTR, out=PTR):
        return lib.geoa3_pointnet_forward(C.byref(w) if w is not None else None, x, B, N, out, ws, None)

    def bwd(w, B=2, N=1024, ws=PTR, x=PTR, g=PTR, dx=PTR):
        return lib.geoa3_pointnet_backward(C.byref(w) if w is not None else None, x, g, B, N, dx, ws, None)

    for call in (fwd, bwd):
        for kw in BAD_WEIGHTS:
            assert call(_weights(**kw)) == EINVAL, (call.__name__, kw)
        good = _weights()
        assert call(good, ws=PTR + 16) == EINVAL and call(good, ws=PTR + 255) == EINVAL   # not 256-byte aligned
        assert call(good, ws=None) == EINVAL and call(None) == EINVAL
        assert call(good, B=0) == EINVAL and call(good, N=0) == EINVAL and call(good, x=None) == EINVAL
    assert fwd(_weights(), out=None) == EINVAL
    assert bwd(_weights(), g=None) == EINVAL and bwd(_weights(), dx=None) == EINVAL
