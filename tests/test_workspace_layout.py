"""CPU-only: the workspaces of both victims, buffer by buffer, against a record taken from the library when struct members,
carve-up and names were still three hand-written lists (tests/golden/workspace_layouts.json: names, byte offsets, total).
tools/iteration_replay_soak.py, tools/bench_wide_bwd.py and the kernel tests address buffers by these names and offsets."""
import ctypes as C
import json
import os

import pytest

from geoa3_amd import _lib

RECORD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "workspace_layouts.json")))
CAP = 128


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _lib.load()


def _layout(fn, *sizes):
    names, offs = (C.c_char_p * CAP)(), (C.c_int64 * CAP)()
    n = fn(*sizes, names, offs, CAP)
    assert 0 < n <= CAP
    return [names[i].decode() for i in range(n)], [int(offs[i]) for i in range(n)]


def _check_shape(offs, total):
    assert offs[0] == 0 and all(a < b for a, b in zip(offs, offs[1:]))        # address order, no buffer empty
    assert all(o % 256 == 0 for o in offs) and total % 256 == 0
    assert offs[-1] < total


def test_the_record_covers_the_sizes_it_should():
    assert [(r["B"], r["N"]) for r in RECORD["pointnet"]] == [(1, 1), (2, 77), (3, 257), (250, 1024), (1, 4100)]
    assert [(r["B"], r["N"]) for r in RECORD["pn2ssg"]] == [(1, 32), (2, 100), (250, 1024)]


@pytest.mark.parametrize("rec", RECORD["pointnet"], ids=lambda r: "B%d-N%d" % (r["B"], r["N"]))
def test_pointnet_workspace_is_the_recorded_one(lib, rec):
    names, offs = _layout(lib.geoa3_debug_pointnet_workspace_layout, rec["B"], rec["N"], rec["classes"])
    total = lib.geoa3_pointnet_workspace_bytes(rec["B"], rec["N"], rec["classes"])
    assert names == rec["names"] and offs == rec["offsets"] and total == rec["total"]
    _check_shape(offs, total)
    assert lib.geoa3_pointnet_workspace_bytes(rec["B"], rec["N"], 10) == total    # (the classifier's width takes no room)


@pytest.mark.parametrize("rec", RECORD["pn2ssg"], ids=lambda r: "B%d-N%d" % (r["B"], r["N"]))
def test_pn2ssg_workspace_is_the_recorded_one(lib, rec):
    names, offs = _layout(lib.geoa3_debug_pn2ssg_workspace_layout, rec["B"], rec["N"])
    total = lib.geoa3_pn2ssg_workspace_bytes(rec["B"], rec["N"])
    assert names == rec["names"] and offs == rec["offsets"] and total == rec["total"]
    assert names[-1] == "end" and offs[-1] == total
    _check_shape(offs[:-1], total)
