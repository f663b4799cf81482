"""Numpy restatements of geoa3_amd/csrc/mesh_sample.hip, written from its specification (include/geoa3_hip.h), one mesh
at a time:

    area_weights   A_f = 0.5 |(b-a) x (c-a)| in float64 from the float32 vertices; a face with an index outside [0,V) or a
                   non-finite area is bad and weighs 0; unit = 2^(e-40), (m, e) = frexp(max A_f); w_f = rint(A_f / unit)
    area_table     the inclusive prefix sum of w in uint64
    pick           t = min(T-1, uint64(float64(u0) * float64(T))); the first f with table[f] > t; -1 when T = 0 or a draw
                   is NaN
    points         float32, one operation at a time: r1, r2 = u1, u2, both 1 - r when r1 + r2 >= 1 (decided on the same
                   float32 bits as the kernel), r3 = (1 - r1) - r2, p = (r1 a + r2 b) + r3 c
    normals        (b-a) x (c-a) / |.| in float64, rounded to float32 by the caller
"""
import numpy as np

F = np.float32
D = np.float64


def _corners(verts, faces):
    """-> (ok [F], a, b, c f32 [F,3]) with the corners of a face that is not ok set to 0 (never gathered)."""
    verts = np.asarray(verts, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(verts))).all(1)
    safe = np.where(ok[:, None], faces, 0)
    if len(verts) == 0:
        z = np.zeros((len(faces), 3), F)
        return ok, z, z, z
    return ok, verts[safe[:, 0]], verts[safe[:, 1]], verts[safe[:, 2]]


def cross(verts, faces):
    """-> (index_ok [F], n f64 [F,3] = (b-a) x (c-a))"""
    ok, a, b, c = _corners(verts, faces)
    u, v = b.astype(D) - a.astype(D), c.astype(D) - a.astype(D)
    n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                  u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    return ok, n


def areas(verts, faces):
    """-> (A f64 [F] with 0 for a bad face, bad bool [F])"""
    ok, n = cross(verts, faces)
    with np.errstate(all="ignore"):
        a = 0.5 * np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    bad = ~ok | ~np.isfinite(a)
    return np.where(bad, 0.0, a), bad


def scaled_areas(verts, faces):
    """-> (A_f / unit f64 [F], bad [F]): what the weights are rounded from (scaling by a power of two is exact)"""
    a, bad = areas(verts, faces)
    if len(a) == 0:
        return a, bad
    _, e = np.frexp(a.max())
    return np.ldexp(a, 40 - int(e)), bad


def area_weights(verts, faces):
    """-> (w uint64 [F], number of bad faces)"""
    x, bad = scaled_areas(verts, faces)
    return np.rint(x).astype(np.uint64), int(bad.sum())


def area_table(verts, faces):
    w, nbad = area_weights(verts, faces)
    return np.cumsum(w, dtype=np.uint64), nbad


def pick(table, u0):
    """table uint64 [F], u0 f32 [S] -> face index int32 [S]"""
    u0 = np.asarray(u0, F)
    out = np.full(len(u0), -1, np.int32)
    if len(table) == 0 or int(table[-1]) == 0:
        return out
    T = int(table[-1])
    for s, x in enumerate(u0):
        if np.isnan(x):
            continue
        y = D(x) * D(T)
        t = 0 if y <= 0 else min(T - 1, int(y))
        out[s] = np.searchsorted(table, np.uint64(t), side="right")
    return out


def points(verts, faces, fidx, u):
    """u f32 [S,3] -> p f32 [S,3]; NaN where fidx < 0 or a draw is NaN"""
    verts, faces, u = np.asarray(verts, F).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(u, F)
    out = np.full((len(u), 3), np.nan, F)
    one = F(1)
    for s in range(len(u)):
        if fidx[s] < 0 or np.isnan(u[s]).any():
            continue
        a, b, c = (verts[j] for j in faces[fidx[s]])
        r1, r2 = u[s, 1], u[s, 2]
        if F(r1 + r2) >= one:
            r1, r2 = F(one - r1), F(one - r2)
        r3 = F(F(one - r1) - r2)
        out[s] = ((r1 * a).astype(F) + (r2 * b).astype(F)).astype(F) + (r3 * c).astype(F)
    return out


def normals(verts, faces, fidx):
    """-> n f64 [S,3] (unit, signed by the winding); NaN where fidx < 0"""
    _, n = cross(verts, faces)
    out = np.full((len(fidx), 3), np.nan, D)
    sel = np.asarray(fidx) >= 0
    m = n[np.asarray(fidx)[sel]]
    out[sel] = m / np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])[:, None]
    return out


def sample(verts, faces, u):
    """The whole path for one mesh: u f32 [S,3] -> (p f32 [S,3], n f64 [S,3], fidx int32 [S], bad count).  A sample with
    a NaN draw has fidx -1."""
    u = np.asarray(u, F)
    table, nbad = area_table(verts, faces)
    fidx = pick(table, u[:, 0])
    fidx[np.isnan(u).any(1)] = -1
    return points(verts, faces, fidx, u), normals(verts, faces, fidx), fidx, nbad


# ------------------------------------------------------------------ the solids the tests share
def cube(half=0.5):
    """12 faces, outward winding: face 2k and 2k+1 lie on the side with normal -x, +x, -y, +y, -z, +z for k = 0..5"""
    h = half
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], F)   # index = 4 ix + 2 iy + iz
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6],
                  [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f


def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    return v, f


def prism():
    """a triangular prism: two caps and three sides of two triangles each, of different areas"""
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 3], [2, 0, 3], [0, 1, 3]], F)
    f = np.array([[0, 2, 1], [3, 4, 5], [0, 1, 4], [0, 4, 3], [1, 2, 5], [1, 5, 4], [2, 0, 3], [2, 3, 5]], np.int32)
    return v, f


def lattice_mesh(rng, nv, nf):
    """vertices on the lattice of multiples of 1/64 in [-8, 8]: every cross product and sum of squares is exact in double"""
    v = (rng.integers(-512, 513, (nv, 3)) / 64.0).astype(F)
    f = rng.integers(0, nv, (nf, 3)).astype(np.int32)
    return v, f
