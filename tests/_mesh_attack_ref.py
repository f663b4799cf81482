"""Numpy restatements of geoa3_amd/csrc/mesh_attack.hip, written from the definitions of the mesh attack (include/geoa3_hip.h,
"Mesh attack"), one mesh at a time and in float64 unless a name ends in 32:

    topology        the unique undirected edges {i,j}, i < j, of the faces whose indices all lie in [0,V), sorted by (i, j),
                    and N(i), the neighbours of i in ascending order
    laplacian       delta_i = (sum_{j in N(i)} v_j) / deg_i - v_i (0 when deg_i = 0), Lap = (1/V) sum_i |delta_i| (0 when V = 0)
    laplacian_grad  (1/V) (-u_i [deg_i > 0] + sum_{j in N(i)} u_j / deg_j), u_i = delta_i / |delta_i| taken as 0 at 0
    edge            (1/E) sum_{edges} (l_ij - t_ij)^2 (0 when E = 0); t a number or one value per (i, position in N(i))
    edge_grad       (2/E) sum_{j in N(i)} (l_ij - t_ij) (v_i - v_j) / l_ij, the summand 0 when l_ij = 0
    weights32       the sampler's barycentric weights of a draw, float32 (the form of tests/_mesh_ref.py: points)
    points32/64     p = (r1 a + r2 b) + r3 c, float32 one operation at a time / float64 from the float32 weights
    pullback64/32   g_v = sum of w_k(s) g[s] over the (sample, corner) entries of vertex v, ascending (s, k); the 32 form is
                    the sequential float32 loop the kernel promises to equal bit for bit
Every sum over N(i) runs in ascending j, in the order the kernels use.
"""
import numpy as np

F = np.float32
D = np.float64


# ------------------------------------------------------------------ topology
def topology(nv, faces):
    """-> (edges int64 [E,2] with i < j sorted by (i, j), nbrs: list of nv ascending int64 arrays)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    seen = set()
    for f in faces:
        if not all(0 <= x < nv for x in f):
            continue
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            if a != b:
                seen.add((int(min(a, b)), int(max(a, b))))
    edges = np.array(sorted(seen), np.int64).reshape(-1, 2)
    nbrs = [[] for _ in range(nv)]
    for i, j in edges:
        nbrs[i].append(j)
        nbrs[j].append(i)
    return edges, [np.array(sorted(n), np.int64) for n in nbrs]


# ------------------------------------------------------------------ the two terms
def _delta(v, nbrs):
    v = np.asarray(v, D).reshape(-1, 3)
    delta = np.zeros_like(v)
    for i, n in enumerate(nbrs):
        if len(n):
            s = np.zeros(3, D)
            for j in n:
                s = s + v[j]
            delta[i] = s / D(len(n)) - v[i]
    with np.errstate(all="ignore"):
        norm = np.sqrt((delta[:, 0] * delta[:, 0] + delta[:, 1] * delta[:, 1]) + delta[:, 2] * delta[:, 2])
        unit = np.where(norm[:, None] == 0, 0.0, delta / np.where(norm == 0, 1.0, norm)[:, None])
    return delta, norm, unit


def laplacian(v, nbrs):
    """-> (Lap, |delta_i| [V], u_i [V,3])"""
    _, norm, unit = _delta(v, nbrs)
    return (norm.sum() / len(nbrs) if len(nbrs) else 0.0), norm, unit


def laplacian_grad(v, nbrs):
    _, _, unit = _delta(v, nbrs)
    g = np.zeros((len(nbrs), 3), D)
    for i, n in enumerate(nbrs):
        if len(n):
            g[i] = -unit[i]
        for j in n:
            g[i] = g[i] + unit[j] / D(len(nbrs[j]))
    return g / max(len(nbrs), 1)


def _target(target, nbrs, i, pos, offs):
    return D(target) if np.ndim(target) == 0 else D(target[offs[i] + pos])


def _offsets(nbrs):
    return np.concatenate([[0], np.cumsum([len(n) for n in nbrs])]).astype(np.int64)


def lengths(v, nbrs):
    """l_ij of every (i, position in N(i)) entry, float64 [nnz]"""
    v = np.asarray(v, D).reshape(-1, 3)
    out = []
    for i, n in enumerate(nbrs):
        for j in n:
            d = v[i] - v[j]
            out.append(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    return np.array(out, D)


def edge(v, nbrs, target=0.0):
    """target: a number, or one value per (i, position in N(i)) entry (both directions of an edge hold the same)"""
    v = np.asarray(v, D).reshape(-1, 3)
    offs, total, count = _offsets(nbrs), 0.0, 0
    for i, n in enumerate(nbrs):
        for pos, j in enumerate(n):
            if j > i:
                d = v[i] - v[j]
                l = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                total += (l - _target(target, nbrs, i, pos, offs)) ** 2
                count += 1
    return total / count if count else 0.0


def edge_grad(v, nbrs, target=0.0):
    v = np.asarray(v, D).reshape(-1, 3)
    offs = _offsets(nbrs)
    count = sum(len(n) for n in nbrs) // 2
    g = np.zeros((len(nbrs), 3), D)
    for i, n in enumerate(nbrs):
        for pos, j in enumerate(n):
            d = v[i] - v[j]
            l = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if l != 0:
                g[i] = g[i] + (l - _target(target, nbrs, i, pos, offs)) / l * d
    return 2.0 * g / max(count, 1)


# ------------------------------------------------------------------ surface points of the current vertices
def weights32(u):
    """u f32 [S,3] -> w f32 [S,3] = (r1, r2, r3), the fold decided on the float32 sum as the kernel does"""
    u = np.asarray(u, F)
    one = F(1)
    w = np.empty((len(u), 3), F)
    for s in range(len(u)):
        r1, r2 = u[s, 1], u[s, 2]
        if F(r1 + r2) >= one:
            r1, r2 = F(one - r1), F(one - r2)
        w[s] = (r1, r2, F(F(one - r1) - r2))
    return w


def _valid(nv, faces, fidx, s):
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return 0 <= fidx[s] < len(faces) and all(0 <= x < nv for x in faces[fidx[s]])


def points32(verts, faces, fidx, u):
    """verts f32 [V,3] -> p f32 [S,3], NaN for a sample without a face (the form of tests/_mesh_ref.py: points)"""
    verts, faces = np.asarray(verts, F).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    w = weights32(u)
    out = np.full((len(w), 3), np.nan, F)
    for s in range(len(w)):
        if not _valid(len(verts), faces, fidx, s):
            continue
        a, b, c = (verts[j] for j in faces[fidx[s]])
        out[s] = ((w[s, 0] * a).astype(F) + (w[s, 1] * b).astype(F)).astype(F) + (w[s, 2] * c).astype(F)
    return out


def points64(verts, faces, fidx, u):
    verts, faces = np.asarray(verts, D).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    w = weights32(u).astype(D)
    out = np.full((len(w), 3), np.nan, D)
    for s in range(len(w)):
        if _valid(len(verts), faces, fidx, s):
            a, b, c = (verts[j] for j in faces[fidx[s]])
            out[s] = (w[s, 0] * a + w[s, 1] * b) + w[s, 2] * c
    return out


def pullback64(g, nv, faces, fidx, u):
    """g [S,3] -> (g_verts f64 [nv,3], mag [nv,3] = the sum of |w g| behind every entry, terms [nv] = entries per vertex)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    g, w = np.asarray(g, D), weights32(u).astype(D)
    out, mag, terms = np.zeros((nv, 3), D), np.zeros((nv, 3), D), np.zeros(nv, np.int64)
    for s in range(len(w)):
        if _valid(nv, faces, fidx, s):
            for k in range(3):
                v = faces[fidx[s], k]
                out[v] += w[s, k] * g[s]
                mag[v] += np.abs(w[s, k] * g[s])
                terms[v] += 1
    return out, mag, terms


def pullback32(g, nv, faces, fidx, u):
    """the kernel's promise: float32 products added one after the other from +0.0 in ascending (s, k)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    g, w = np.asarray(g, F), weights32(u)
    out = np.zeros((nv, 3), F)
    for s in range(len(w)):
        if _valid(nv, faces, fidx, s):
            for k in range(3):
                v = faces[fidx[s], k]
                out[v] = (out[v] + (w[s, k] * g[s]).astype(F)).astype(F)
    return out


# ------------------------------------------------------------------ the solids the tests share
def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def subdivide(v, f, on_sphere=True):
    """every triangle into four through its edge midpoints (pushed to the unit sphere when on_sphere)"""
    v = [tuple(x) for x in np.asarray(v, D)]
    mid, out = {}, []

    def m(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            p = (np.array(v[a]) + np.array(v[b])) / 2
            if on_sphere:
                p = p / np.linalg.norm(p)
            mid[key] = len(v)
            v.append(tuple(p))
        return mid[key]

    for a, b, c in np.asarray(f, np.int64):
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [[a, ab, ca], [ab, b, bc], [ca, bc, c], [ab, bc, ca]]
    return np.array(v, F), np.array(out, np.int32)


def fan(n, lift=0.25):
    """a hub (vertex 0, lifted off the plane of the ring) joined to a closed ring of n vertices: the hub has degree n"""
    ang = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0, 0, lift]], np.stack([np.cos(ang), np.sin(ang), 0.1 * np.sin(3 * ang)], 1)]).astype(F)
    f = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)
    return v, f


def isolated():
    """a tetrahedron and a fifth vertex no face names"""
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [3, 3, 3]], F)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    return v, f


def coincident():
    """a square fan whose hub sits exactly at the mean of its ring (delta_hub = 0), with vertices 5 and 6 at the same
    place and joined by an edge (l_56 = 0); every coordinate is a small integer, so these zeros are exact in any precision"""
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [-2, 0, 0], [0, -2, 0], [2, 2, 1], [2, 2, 1]], F)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1], [1, 5, 2], [5, 6, 2], [1, 6, 5]], np.int32)
    return v, f


def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    return v, f


def grid_mesh(nv, rng):
    """nv >= 3 vertices at random places, triangulated as a strip (i, i+1, i+2): every vertex in a face; nv = 1, 2: no faces"""
    v = rng.standard_normal((nv, 3)).astype(F)
    f = np.array([[i, i + 1, i + 2] for i in range(max(nv - 2, 0))], np.int32).reshape(-1, 3)
    return v, f


def cases():
    """name -> (verts f32 [V,3], faces i32 [F,3]): the meshes of the gradient checks"""
    octa = subdivide(*octahedron())
    return {"tetrahedron": tetrahedron(), "octahedron_1": octa, "fan_70": fan(70), "isolated": isolated(),
            "coincident": coincident()}
