"""Timings of the mesh input path (GPU): the area table and the surface sampler at B = 250 meshes of about 1e4 faces and
S = 16384 samples each, next to the numpy loop the reference defines (Provider/gen_data_mat.py:88-119, restated in
tests/_mesh_ref.py) on ONE mesh, and mesh_clouds' whole path to 1024- and 10000-point clouds."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from geoa3_amd import mesh  # noqa: E402
from tests import _mesh_ref as R  # noqa: E402


def timeit(fn, n=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def ellipsoid_mesh(g, rings=71, segs=70):
    """a closed grid over an ellipsoid with random semi-axes and a radial ripple: 2 * segs * rings triangles, very unequal
    in area (thin ones near the poles, one of every pair AT a pole without any)"""
    th = np.linspace(0.0, np.pi, rings + 1)[:, None]
    ph = np.linspace(0.0, 2 * np.pi, segs, endpoint=False)[None, :]
    r = 1.0 + 0.1 * np.sin(3 * th) * np.cos(4 * ph + g.uniform(0, 6.28))
    ax = g.uniform(0.3, 1.0, 3)
    v = np.stack([ax[0] * r * np.sin(th) * np.cos(ph), ax[1] * r * np.sin(th) * np.sin(ph),
                  ax[2] * r * np.cos(th) * np.ones_like(ph)], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(rings), np.arange(segs), indexing="ij")
    a, b = i * segs + j, i * segs + (j + 1) % segs
    c, d = a + segs, b + segs
    f = np.concatenate([np.stack([a, c, b], -1).reshape(-1, 3), np.stack([b, c, d], -1).reshape(-1, 3)]).astype(np.int32)
    return v, f


def main():
    B, S = 250, 16384
    g = np.random.default_rng(0)
    meshes = [ellipsoid_mesh(g) for _ in range(B)]
    packed = mesh.pack_meshes(meshes)
    print("B=%d meshes, %d faces each, S=%d" % (B, len(meshes[0][1]), S))
    u = torch.rand(B, S, 3, device="cuda")
    print("area table                         : %.3f ms" % timeit(lambda: mesh.area_table(packed)))
    print("table + sampler (sample_surface)   : %.3f ms" % timeit(lambda: mesh.sample_surface(packed, S, u=u)))
    print("mesh_clouds -> 1024 and 10000      : %.1f ms" % timeit(lambda: mesh.mesh_clouds(packed, 1024, 10000, S, u=u),
                                                                  n=3, warm=1))
    v, f = meshes[0]
    u0 = u[0].cpu().numpy()
    t0 = time.perf_counter()
    R.sample(v, f, u0)
    one = (time.perf_counter() - t0) * 1e3
    print("numpy loop restatement, ONE mesh   : %.1f ms (x %d meshes = %.1f s)" % (one, B, one * B / 1e3))


if __name__ == "__main__":
    main()
