#!/usr/bin/env python3
"""Phase times inside knn_slabp_kernel<32, false> (probe build: python -m geoa3_amd.build --variant tools/ub/lib_sp_stamps
-DGEOA3_SP_STAMPS; run with GEOA3_LIB_PATH=tools/ub/lib_sp_stamps/libgeoa3_hip.so): s_memtime (shader cycles)
at the phase boundaries of wavefront 0 of eight workgroups (the second of instances 7, 39, ... 231), in the
LAST launch of the attack loop at B = 250, N = 1024, K = 17 after 150 presteps -- the loop's own iterates and its own prior.

    python tools/sp_stamps.py [--parent]      (--parent: the boundary names in the order of the kernel before the rewrite)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

# stamp i is taken at the END of phase NAMES[i - 1]
NAMES = ["head: query's index arrived", "cloud staged", "prior rows staged", "seed radius", "run staged",
         "window / barrier", "scan", "final ranking", "write-back"]
NAMES_PARENT = ["head loads", "cloud staged", "prior rows staged", "seed radius", "window / barrier", "run staged", "scan",
                "final ranking", "write-back"]


def main():
    names = NAMES_PARENT if "--parent" in sys.argv else NAMES
    import bench
    sys.argv = [sys.argv[0], "--gpus", "1", "--steps", "2", "--warmup", "0", "--presteps", "150", "--no-cpu-baseline"]
    bench.main()
    import torch
    from geoa3_amd import _lib
    torch.cuda.synchronize()
    lib = _lib.load()
    buf = (C.c_ulonglong * (8 * 16))()
    lib.geoa3_debug_sp_stamps.argtypes = [C.c_void_p]
    assert lib.geoa3_debug_sp_stamps(buf) == 0
    t = np.array(buf[:], dtype=np.int64).reshape(8, 16)[:, :len(names) + 1]
    d = np.diff(t, axis=1)
    print("shader cycles; total per workgroup", (t[:, -1] - t[:, 0]).tolist())
    for i, n in enumerate(names):
        print("   %-28s median %6d   %s" % (n, int(np.median(d[:, i])), d[:, i].tolist()))


if __name__ == "__main__":
    main()
