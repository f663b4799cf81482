"""GPU: the kernels of geoa3_amd/csrc/mesh_attack.hip, each alone through geoa3_amd.mesh's thin wrappers, against the
float64 restatements of tests/_mesh_attack_ref.py (which tests/test_mesh_attack_ref.py pins to central differences), and the
three operators built on them.

Bounds, u = 2^-24 (a float32 rounding, relative), all per entry and derived, none fitted:
  points        bit for bit: the sampler's own float32 operations (mesh_sample.hip:208-217), no contraction.
  pullback      bit for bit against the sequential float32 loop (pullback32), and against float64:
                |got - ref| <= (n + 2) u mag, n = the entries of the vertex's list, mag = sum |w g| behind the entry.  Each
                term is rounded once as a product and at most n - 1 times in the additions (the first is added to +0.0
                exactly): a factor (1 + u)^n - 1 <= n u / (1 - n u) <= (n + 2) u while n^2 u <= 2, i.e. n <= 5792; the
                float64 reference takes the float32 weights as they are, so the weights add nothing.
  Lap_b, Edge_b per-vertex terms in double, per-mesh sums in double in a fixed order, ONE float32 rounding of the result: u |ref|
                plus NOISE = 2^-52 (deg_max + V + 16) times the magnitudes for the double chain.  The kernel rounds every
                length to float32 once (so that the clean mesh's own lengths cancel exactly): |l~ - l| <= u l, so a squared
                residual moves by at most u l (2 |l - t| + u l), summed over the edges and divided by E_b.
  gradient      the kernel reads u_i rounded to float32: |u~ - u| <= 2^-25 per component (|u| <= 1), plus the double chain's
                (deg_i + 4) 2^-52 vmax / |delta_i|; through (1/V)(-u_i + sum_j u_j / deg_j) that is
                (1/V)(err_i + sum_j err_j / deg_j).  Edge: (1 - t / l~) against (1 - t / l) differs by at most
                |t| u (1 + 2^-23) / l, times |v_i - v_j| <= l: |t_ij| u (1 + 2^-23) per neighbour, times 2 / E_b.  Then one
                float32 rounding of the sum, u |ref|, and with `add` one more of old + g."""
import functools

import numpy as np
import pytest
import torch

from tests import _mesh_attack_ref as R

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
U = 2.0 ** -24
OK, EINVAL, ENOSUPPORT = 0, -1, -3
POISON = -77.0


@pytest.fixture(scope="module")
def M():
    from geoa3_amd import _lib, mesh
    assert torch.cuda.is_available(), "needs the MI355X"
    _lib.load()
    return mesh


def _np(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), F(np.nan), a).view(np.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ mesh_points
@functools.lru_cache(maxsize=None)
def _point_meshes():
    """B = 3, ragged: 4, 65 and 300 vertices"""
    rng = np.random.default_rng(11)
    return [R.tetrahedron(), R.grid_mesh(65, rng), R.grid_mesh(300, rng)]


@pytest.mark.parametrize("S", [1, 63, 64, 65, 1000])
def test_points_equal_the_samplers_bits_and_the_float32_restatement(M, S):
    meshes = _point_meshes()
    packed = M.pack_meshes(meshes)
    verts, nv = M.to_planar(packed)
    assert verts.shape == (3, 3, 300)
    u = torch.rand(3, S, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(S))
    pts, _, fidx, bad = M.sample_surface(packed, S, u=u)
    assert not _np(bad).any() and (_np(fidx) >= 0).all()
    got = M.mesh_points_forward(verts, nv, packed.faces, packed.face_off, fidx, u)
    assert np.array_equal(_bits(_np(got)), _bits(_np(pts)))                       # clean vertices: the sampler's points
    moved = verts + 0.05 * torch.randn(verts.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    fidx2 = fidx.clone()
    fidx2[1, S // 2] = -1                                                         # no face: NaN for that sample alone
    got = _np(M.mesh_points_forward(moved, nv, packed.faces, packed.face_off, fidx2, u))
    mv, fi, uu = _np(moved), _np(fidx2), _np(u)
    for b, (v, f) in enumerate(meshes):
        want = R.points32(mv[b, :, :len(v)].T, f, fi[b], uu[b])
        assert np.array_equal(_bits(got[b].T), _bits(want)), b
    assert np.isnan(got[1, :, S // 2]).all() and np.isnan(got).sum() == 3


# ------------------------------------------------------------------ corner index and pullback
@pytest.mark.parametrize("S", [200, 64])
def test_pullback_ordered_sum_against_float64_and_the_float32_loop(M, S):
    """mesh 0: ONE triangle -- with S = 200 every vertex's list holds 200 entries, the long-list path of the destination
    lists (more than 64); mesh 1: 300 vertices -- with S = 64 at most 192 of them get an entry, the others +0.0.
    Vp = 300: columns 3.. of mesh 0 are padding and must be exactly 0."""
    rng = np.random.default_rng(S)
    tri = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], F), np.array([[0, 1, 2]], np.int32))
    meshes = [tri, R.grid_mesh(300, rng)]
    packed = M.pack_meshes(meshes)
    verts, nv = M.to_planar(packed)
    gen = torch.Generator("cuda").manual_seed(S)
    u = torch.rand(2, S, 3, device="cuda", generator=gen)
    _, _, fidx, _ = M.sample_surface(packed, S, u=u)
    fidx[1, 3] = -1                                                               # its three entries are in no list
    g = torch.randn(2, 3, S, device="cuda", generator=gen)
    corner = _np(M.mesh_corner_index(nv, packed.faces, packed.face_off, fidx, 300))
    fi, uu, gg = _np(fidx), _np(u), _np(g)
    for b, (v, f) in enumerate(meshes):
        want = np.where(fi[b][:, None] >= 0, f[np.maximum(fi[b], 0)], -1)
        assert np.array_equal(corner[b].reshape(S, 3), want)
    lists = M.mesh_point_lists(nv, packed.faces, packed.face_off, fidx, 300)
    out = torch.full((2, 3, 300), POISON, device="cuda")
    M.mesh_points_backward(g, u, lists, 300, out=out)
    got = _np(out)
    again = _np(M.mesh_points_backward(g, u, M.mesh_point_lists(nv, packed.faces, packed.face_off, fidx, 300), 300))
    assert np.array_equal(_bits(got), _bits(again))                               # two runs, two list builds: identical bits
    for b, (v, f) in enumerate(meshes):
        ref, mag, terms = R.pullback64(gg[b].T, len(v), f, fi[b], uu[b])
        mine = got[b, :, :len(v)].T
        assert (np.abs(mine - ref) <= (terms[:, None] + 2) * U * mag).all(), b
        assert np.array_equal(_bits(mine), _bits(R.pullback32(gg[b].T, len(v), f, fi[b], uu[b]))), b
        assert not got[b, :, len(v):].any() and not np.signbit(got[b, :, len(v):]).any()      # padding: +0.0
        assert not mine[terms == 0].any()
        if b == 0 and S == 200:
            assert terms.tolist() == [200, 200, 200]
        if b == 1 and S == 64:
            assert (terms == 0).sum() >= 300 - 192


# ------------------------------------------------------------------ mesh_reg / mesh_reg_grad
@functools.lru_cache(maxsize=None)
def _reg_meshes():
    """the meshes of the CPU gradient checks, plus V in {1, 63, 64, 65}: one ragged padded batch, Vp = 71"""
    rng = np.random.default_rng(5)
    named = R.cases()
    return [named[k] for k in sorted(named)] + [R.grid_mesh(n, rng) for n in (1, 63, 64, 65)]


class _Batch:
    def __init__(self, M, meshes):
        self.meshes = meshes
        self.packed = M.pack_meshes(meshes)
        self.verts, self.nv = M.to_planar(self.packed)
        self.topo = M.MeshTopology.from_packed(self.packed)
        self.nbrs = [R.topology(len(v), f)[1] for v, f in meshes]
        self.vp = self.topo.vp
        off = _np(self.topo.row_off)
        self.entry = [(int(off[b * self.vp]), int(off[b * self.vp + len(v)])) for b, (v, _) in enumerate(meshes)]

    def call(self, M, verts, target, scalar):
        t = self.topo
        return M.mesh_reg_forward(verts, self.nv, t.row_off, t.col, t.ne, target, scalar)

    def grad(self, M, verts, target, scalar, unit, **kw):
        t = self.topo
        return M.mesh_reg_backward(verts, self.nv, t.row_off, t.col, t.ne, target, scalar, unit, **kw)


def _noise(v, nbrs):
    deg = max([len(n) for n in nbrs] + [1])
    return 2.0 ** -52 * (deg + len(nbrs) + 16)


def _forward_bounds(v, nbrs, tgt):
    """-> (Lap, tol), (Edge, tol) of one mesh in float64 from the float32 vertices v [V,3]"""
    v = v.astype(D)
    vmax = np.abs(v).max() if len(v) else 0.0
    lap = R.laplacian(v, nbrs)[0]
    ed = R.edge(v, nbrs, tgt)
    ls = R.lengths(v, nbrs)
    ts = np.full(len(ls), tgt, D) if np.ndim(tgt) == 0 else np.asarray(tgt, D)
    ne = max(len(ls) // 2, 1)
    moved = (U * ls * (2 * np.abs(ls - ts) + U * ls)).sum() / 2 / ne         # every edge is listed twice
    scale = ((ls.max() if len(ls) else 0.0) + (np.abs(ts).max() if len(ts) else 0.0)) ** 2
    return (lap, U * abs(lap) + _noise(v, nbrs) * (vmax + 1)), (ed, moved + U * abs(ed) + _noise(v, nbrs) * (scale + 1))


def _grad_bounds(v, nbrs, tgt):
    """-> (dLap [V,3], tol [V,1]), (dEdge, tol) before weights and the final rounding"""
    v = v.astype(D)
    nv = len(nbrs)
    vmax = np.abs(v).max() if nv else 0.0
    _, norm, _ = R.laplacian(v, nbrs)
    deg = np.array([len(n) for n in nbrs], D)
    with np.errstate(all="ignore"):
        err_u = 2.0 ** -25 + np.where(norm > 0, (deg + 4) * 2.0 ** -52 * vmax / np.where(norm > 0, norm, 1.0), 0.0)
    tol_l = np.zeros(nv, D)
    for i, n in enumerate(nbrs):
        tol_l[i] = ((err_u[i] if len(n) else 0.0) + sum(err_u[j] / deg[j] for j in n)) / nv
    ls = R.lengths(v, nbrs)
    ts = np.abs(np.full(len(ls), tgt, D) if np.ndim(tgt) == 0 else np.asarray(tgt, D))
    ne = max(len(ls) // 2, 1)
    tol_e, q = np.zeros(nv, D), 0
    for i, n in enumerate(nbrs):
        tol_e[i] = 2.0 / ne * sum(ts[q + p] * U * (1 + 2.0 ** -23) + _noise(v, nbrs) * (ls[q + p] + ts[q + p]) for p in range(len(n)))
        q += len(n)
    return (R.laplacian_grad(v, nbrs), tol_l[:, None]), (R.edge_grad(v, nbrs, tgt), tol_e[:, None])


def _targets(batch, kind):
    """-> (device target or None, scalar, per-mesh restatement target)"""
    if kind == "zero":
        return None, 0.0, [0.0] * len(batch.meshes)
    if kind == "scalar":
        return None, 0.7, [D(F(0.7))] * len(batch.meshes)
    # one value per CSR entry, the same on both directions of an edge: the lengths of OTHER vertices
    rng = np.random.default_rng(3)
    per = []
    for (v, f), nbrs in zip(batch.meshes, batch.nbrs):
        per.append(R.lengths(v.astype(D) + 0.1 * rng.standard_normal(v.shape), nbrs).astype(F))
    return _dev(np.concatenate(per).astype(F)), 0.0, [p.astype(D) for p in per]


@pytest.mark.parametrize("kind", ["zero", "scalar", "per_edge"])
def test_reg_forward_and_gradient_against_float64(M, kind):
    batch = _Batch(M, _reg_meshes())
    assert batch.vp == 71 and batch.topo.batch == 9
    target, scalar, ref_t = _targets(batch, kind)
    lap, edge, unit = batch.call(M, batch.verts, target, scalar)
    lap2, edge2, unit2 = batch.call(M, batch.verts, target, scalar)
    lap_np, edge_np, unit_np = _np(lap), _np(edge), _np(unit)
    assert np.array_equal(_bits(lap_np), _bits(_np(lap2))) and np.array_equal(_bits(edge_np), _bits(_np(edge2)))
    assert np.array_equal(_bits(unit_np), _bits(_np(unit2)))                      # two runs: identical bits
    gl = _dev(np.linspace(0.5, 1.5, 9).astype(F))
    ge = _dev(np.linspace(2.0, 0.25, 9).astype(F))
    old = torch.randn(9, 3, 71, device="cuda", generator=torch.Generator("cuda").manual_seed(4))
    runs = {}
    for name, kw in (("lap", dict(w_lap=1.0, w_edge=0.0)), ("edge", dict(w_lap=0.0, w_edge=1.0)),
                     ("both", dict(w_lap=0.3, w_edge=2.0, g_lap=gl, g_edge=ge)),
                     ("add", dict(w_lap=0.3, w_edge=2.0, g_lap=gl, g_edge=ge, out=old.clone(), add=True))):
        kw.setdefault("g_lap", None), kw.setdefault("g_edge", None)
        runs[name] = _np(batch.grad(M, batch.verts, target, scalar, unit, **kw))
    again = _np(batch.grad(M, batch.verts, target, scalar, unit, w_lap=0.3, w_edge=2.0, g_lap=gl, g_edge=ge))
    assert np.array_equal(_bits(runs["both"]), _bits(again))
    # a weight of 0 SKIPS its term: poison in what only that term reads must not show
    bad_unit = torch.full_like(unit, float("nan"))
    skipped = _np(batch.grad(M, batch.verts, target, scalar, bad_unit, g_lap=None, g_edge=None, w_lap=0.0, w_edge=1.0))
    assert np.array_equal(_bits(skipped), _bits(runs["edge"]))
    nan_target = torch.full((batch.topo.nnz,), float("nan"), device="cuda")
    skipped = _np(batch.grad(M, batch.verts, nan_target, 0.0, unit, g_lap=None, g_edge=None, w_lap=1.0, w_edge=0.0))
    assert np.array_equal(_bits(skipped), _bits(runs["lap"]))
    gl_np, ge_np, old_np = _np(gl).astype(D), _np(ge).astype(D), _np(old).astype(D)
    for b, ((v, f), nbrs) in enumerate(zip(batch.meshes, batch.nbrs)):
        n = len(v)
        (l_ref, l_tol), (e_ref, e_tol) = _forward_bounds(v, nbrs, ref_t[b])
        assert abs(lap_np[b] - l_ref) <= l_tol, (b, lap_np[b], l_ref, l_tol)
        assert abs(edge_np[b] - e_ref) <= e_tol, (b, edge_np[b], e_ref, e_tol)
        _, norm, u_ref = R.laplacian(v.astype(D), nbrs)
        assert np.abs(unit_np[b, 3, :n] - norm).max(initial=0) <= U * norm.max(initial=0) + 1e-12
        assert not unit_np[b, :, n:].any()
        (dl, tl), (de, te) = _grad_bounds(v, nbrs, ref_t[b])
        for name, ref, tol in (("lap", dl, tl), ("edge", de, te),
                               ("both", 0.3 * gl_np[b] * dl + 2.0 * ge_np[b] * de, 0.3 * gl_np[b] * tl + 2.0 * ge_np[b] * te)):
            got = runs[name][b, :, :n].T
            assert (np.abs(got - ref) <= tol + U * np.abs(ref) + 1e-30).all(), (b, name, np.abs(got - ref).max())
            assert not runs[name][b, :, n:].any()                                  # padding columns: exactly 0
        ref = 0.3 * gl_np[b] * dl + 2.0 * ge_np[b] * de
        tol = 0.3 * gl_np[b] * tl + 2.0 * ge_np[b] * te + U * np.abs(ref) + U * np.abs(old_np[b, :, :n].T + ref) + 1e-30
        assert (np.abs(runs["add"][b, :, :n].T - (old_np[b, :, :n].T + ref)) <= tol).all(), b
        assert np.array_equal(runs["add"][b, :, n:], _np(old)[b, :, n:])            # old + 0
    # the zeros the definitions choose: the hub of `coincident` (delta = 0) has u = 0, the isolated vertex no gradient
    names = sorted(R.cases())
    assert not unit_np[names.index("coincident"), :, 0].any()
    assert not runs["both"][names.index("isolated"), :, 4].any()


def test_reg_own_lengths_cancel_exactly_and_constrain_fold(M):
    """target = topo.edge_lengths(verts): Edge_b and its gradient are exactly 0 at those vertices (the kernels work with
    the float32 length on both sides); constrain = ((constrain_add ? constrain : 0) + w_lap Lap) + w_edge Edge in float32."""
    from geoa3_amd import _lib
    batch = _Batch(M, _reg_meshes())
    t = batch.topo
    own = t.edge_lengths(batch.verts)
    lengths = _np(own)
    for b, ((v, f), nbrs) in enumerate(zip(batch.meshes, batch.nbrs)):
        ref = R.lengths(v.astype(D), nbrs)
        assert (np.abs(lengths[batch.entry[b][0]:batch.entry[b][1]] - ref) <= U * ref).all()
    lap, edge, unit = batch.call(M, batch.verts, own, 0.0)
    assert not _np(edge).any()
    g = _np(batch.grad(M, batch.verts, own, 0.0, unit, g_lap=None, g_edge=None, w_lap=0.0, w_edge=1.0))
    assert not g.any()
    moved = batch.verts + 0.01
    moved[:, :, 0] += 0.02
    assert (_np(batch.call(M, moved, own, 0.0)[1])[[0, 2, 6]] > 0).all()
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    lap_np, edge_np = _np(lap), _np(batch.call(M, moved, own, 0.0)[1])
    for add, w_lap, w_edge in ((0, 0.5, 3.0), (1, 0.5, 3.0), (1, 0.0, 3.0), (0, 0.5, 0.0)):
        c = torch.full((9,), 2.25, device="cuda")
        l2, e2, u2 = (torch.empty_like(x) for x in (lap, edge, unit))
        assert lib.geoa3_mesh_reg(moved.data_ptr(), batch.nv.data_ptr(), t.row_off.data_ptr(), t.col.data_ptr(), t.ne.data_ptr(),
                                  own.data_ptr(), 0.0, 9, 71, t.nnz, w_lap, w_edge, u2.data_ptr(), l2.data_ptr(), e2.data_ptr(),
                                  c.data_ptr(), add, s) == OK
        want = np.full(9, 2.25 if add else 0.0, F)
        lm = _np(l2)
        if w_lap != 0:
            want = (want + (F(w_lap) * lm).astype(F)).astype(F)
        if w_edge != 0:
            want = (want + (F(w_edge) * edge_np).astype(F)).astype(F)
        assert np.array_equal(_bits(_np(c)), _bits(want)) and np.array_equal(_bits(_np(e2)), _bits(edge_np))


def test_reg_nan_vertex_is_loud_in_its_own_mesh_only(M):
    BAD = 3                                                                      # octahedron_1: 18 vertices
    batch = _Batch(M, _reg_meshes())
    keep = [b for b in range(9) if b != BAD]
    lap, edge, unit = batch.call(M, batch.verts, None, 0.7)
    g = batch.grad(M, batch.verts, None, 0.7, unit, g_lap=None, g_edge=None, w_lap=1.0, w_edge=1.0)
    for bad in (float("nan"), float("inf")):
        verts = batch.verts.clone()
        verts[BAD, 1, 5] = bad
        lap2, edge2, unit2 = batch.call(M, verts, None, 0.7)
        g2 = batch.grad(M, verts, None, 0.7, unit2, g_lap=None, g_edge=None, w_lap=1.0, w_edge=1.0)
        assert np.isnan(_np(lap2)[BAD]) and np.isnan(_np(edge2)[BAD])
        for a, b in ((lap, lap2), (edge, edge2), (unit, unit2), (g, g2)):
            assert np.array_equal(_bits(_np(a)[keep]), _bits(_np(b)[keep]))
        assert np.isnan(_np(g2)[BAD]).any()
    # a padding column is never read: poison there moves nothing
    verts = batch.verts.clone()
    verts[BAD, :, 18:] = float("nan")
    lap2, edge2, unit2 = batch.call(M, verts, None, 0.7)
    assert np.array_equal(_bits(_np(lap2)), _bits(_np(lap))) and np.array_equal(_bits(_np(edge2)), _bits(_np(edge)))
    g2 = batch.grad(M, verts, None, 0.7, unit2, g_lap=None, g_edge=None, w_lap=1.0, w_edge=1.0)
    assert np.array_equal(_bits(_np(g2)), _bits(_np(g)))
    # ... and the points on its faces, alone: every sample on face 0 of its mesh (-1 where a mesh has no face)
    packed = batch.packed
    u = torch.rand(9, 64, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(9))
    has_faces = (packed.face_off[1:] - packed.face_off[:-1]) > 0
    fidx = torch.where(has_faces[:, None], 0, -1).to(torch.int32).expand(9, 64).contiguous()
    clean = _np(M.mesh_points_forward(batch.verts, batch.nv, packed.faces, packed.face_off, fidx, u))
    verts = batch.verts.clone()
    verts[BAD, 0, int(batch.meshes[BAD][1][0, 0])] = float("nan")
    dirty = _np(M.mesh_points_forward(verts, batch.nv, packed.faces, packed.face_off, fidx, u))
    assert np.isnan(dirty[BAD, 0]).all() and np.array_equal(_bits(dirty[BAD, 1:]), _bits(clean[BAD, 1:]))
    assert np.array_equal(_bits(dirty[keep]), _bits(clean[keep]))
    assert np.isnan(clean[5]).all() and np.isfinite(clean[3]).all()              # (V = 1: no face, no point)


# ------------------------------------------------------------------ size limits: a code, and nothing launched
def test_size_limits_return_their_codes_without_a_launch(M):
    from geoa3_amd import _lib
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    x = torch.full((4096,), POISON, device="cuda")
    i = torch.zeros(4096, dtype=torch.int32, device="cuda")
    off = torch.zeros(8, dtype=torch.int64, device="cuda")
    p, ip, op = x.data_ptr(), i.data_ptr(), off.data_ptr()
    big = 2 ** 31 - 1
    points = lambda B, Vp, S, tf: lib.geoa3_mesh_points(p, ip, ip, op, ip, p, B, Vp, S, tf, p, s)
    assert [points(0, 4, 4, 4), points(1, 0, 4, 4), points(1, 4, 0, 4), points(1, 4, 4, -1)] == [EINVAL] * 4
    assert [points(65536, 4, 4, 4), points(2, big // 2, 4, 4), points(1, 4, big // 3, 4), points(1, 4, 4, 2 ** 31)] == [ENOSUPPORT] * 4
    assert lib.geoa3_mesh_points(None, ip, ip, op, ip, p, 1, 4, 4, 4, p, s) == EINVAL
    corner = lambda B, Vp, S, tf: lib.geoa3_mesh_corner_index(ip, ip, op, ip, B, Vp, S, tf, ip, s)
    assert [corner(0, 4, 4, 4), corner(65536, 4, 4, 4), corner(1, 4, big // 3, 4)] == [EINVAL, ENOSUPPORT, ENOSUPPORT]
    assert lib.geoa3_mesh_points_scratch_bytes(0, 4, 4) == EINVAL and lib.geoa3_mesh_points_scratch_bytes(2, big // 2, 4) == ENOSUPPORT
    assert lib.geoa3_mesh_points_scratch_bytes(3, 10, 7) == 4 * 3 * (11 + 10 + 2 * 21)
    assert lib.geoa3_mesh_points_lists(ip, 0, 4, 4, ip, s) == EINVAL and lib.geoa3_mesh_points_lists(ip, 1, 4, 4, None, s) == EINVAL
    assert lib.geoa3_mesh_points_grad(p, p, ip, 1, 4, big // 3, p, s) == ENOSUPPORT
    assert lib.geoa3_mesh_points_grad(p, p, None, 1, 4, 4, p, s) == EINVAL
    reg = lambda B, Vp, nnz: lib.geoa3_mesh_reg(p, ip, ip, ip, ip, None, 0.0, B, Vp, nnz, 0.0, 0.0, p, p, p, None, 0, s)
    assert [reg(0, 4, 4), reg(1, 0, 4), reg(1, 4, -1), reg(65536, 4, 4), reg(2, big // 2, 4)] == [EINVAL] * 3 + [ENOSUPPORT] * 2
    grad = lambda B, Vp, nnz: lib.geoa3_mesh_reg_grad(p, ip, ip, ip, ip, None, 0.0, p, None, None, 1.0, 1.0, B, Vp, nnz, p, 0, s)
    assert [grad(0, 4, 4), grad(1, 4, -1), grad(2, big // 2, 4)] == [EINVAL, EINVAL, ENOSUPPORT]
    assert lib.geoa3_mesh_reg_grad(p, ip, ip, ip, ip, None, 0.0, None, None, None, 1.0, 1.0, 1, 4, 4, p, 0, s) == EINVAL
    assert lib.geoa3_mesh_edge_lengths(p, ip, ip, ip, 0, 4, 4, p, s) == EINVAL
    assert lib.geoa3_mesh_edge_lengths(p, ip, ip, ip, 2, big // 2, 4, p, s) == ENOSUPPORT
    assert (_np(x) == POISON).all() and not _np(i).any()


# ------------------------------------------------------------------ the operators
def test_operators_backward_is_the_kernels_gradient_and_compiles(M):
    meshes = _reg_meshes()[:5]
    batch = _Batch(M, meshes)
    t, packed = batch.topo, batch.packed
    gen = torch.Generator("cuda").manual_seed(21)
    S = 96
    u = torch.rand(5, S, 3, device="cuda", generator=gen)
    _, _, fidx, _ = M.sample_surface(packed, S, u=u)
    own = t.edge_lengths(batch.verts)
    x0 = batch.verts + 0.03 * torch.randn(batch.verts.shape, device="cuda", generator=gen)
    gp = torch.randn(5, 3, S, device="cuda", generator=gen)
    c1, c2 = torch.rand(5, device="cuda", generator=gen), torch.rand(5, device="cuda", generator=gen)
    lists = M.mesh_point_lists(batch.nv, packed.faces, packed.face_off, fidx, batch.vp)

    def grad_of(fn):
        x = x0.clone().requires_grad_()
        out = fn(x)
        (g,) = torch.autograd.grad(out, x)
        return out.detach(), g

    # surface_points: values are the kernel's, the backward is the ordered pullback (with or without the draw's lists)
    want = M.mesh_points_backward(gp, u, lists, batch.vp)
    for ls in (None, lists):
        val, g = grad_of(lambda x: (M.surface_points(x, batch.nv, packed, fidx, u, lists=ls) * gp).sum())
        assert torch.equal(g, want)
    assert torch.equal(M.surface_points(x0, batch.nv, (packed.faces, packed.face_off), fidx, u),
                       M.mesh_points_forward(x0, batch.nv, packed.faces, packed.face_off, fidx, u))
    # the two terms: per-mesh values [B], backward through the gather kernel with the upstream weights
    lap, edge, unit = batch.call(M, x0, own, 0.0)
    val, g = grad_of(lambda x: (M.mesh_laplacian_smoothing(x, batch.nv, t) * c1).sum())
    assert torch.equal(g, batch.grad(M, x0, None, 0.0, unit, g_lap=c1, g_edge=None, w_lap=1.0, w_edge=0.0))
    assert torch.equal(M.mesh_laplacian_smoothing(x0, batch.nv, t), lap)
    val, g = grad_of(lambda x: (M.mesh_edge_loss(x, batch.nv, t, own) * c2).sum())
    assert torch.equal(g, batch.grad(M, x0, own, 0.0, unit, g_lap=None, g_edge=c2, w_lap=0.0, w_edge=1.0))
    assert torch.equal(M.mesh_edge_loss(x0, batch.nv, t, own), edge)
    assert torch.equal(M.mesh_edge_loss(x0, batch.nv, t, 0.5, reduction="mean"), batch.call(M, x0, None, 0.5)[1].mean())
    assert torch.equal(M.mesh_laplacian_smoothing(x0, batch.nv, t, reduction="mean"), lap.mean())
    # against float64, through autograd: the derived bounds
    _, g = grad_of(lambda x: M.mesh_laplacian_smoothing(x, batch.nv, t).sum() + M.mesh_edge_loss(x, batch.nv, t, 0.7).sum())
    g_np, x_np = _np(g), _np(x0)
    for b, ((v, f), nbrs) in enumerate(zip(meshes, batch.nbrs)):
        xb = x_np[b, :, :len(v)].T
        (dl, tl), (de, te) = _grad_bounds(xb, nbrs, D(F(0.7)))
        tol = tl + te + U * (np.abs(dl) + np.abs(de)) + U * np.abs(dl + de) + 1e-30       # two kernels' roundings and their sum
        assert (np.abs(g_np[b, :, :len(v)].T - (dl + de)) <= tol).all(), b
    # no second derivative
    x = x0.clone().requires_grad_()
    (g1,) = torch.autograd.grad(M.mesh_laplacian_smoothing(x, batch.nv, t).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="first derivative"):
        g1.sum().backward()

    # torch.compile(fullgraph=True) traces a composition of the three
    def f(x):
        pts = M.surface_points(x, batch.nv, packed, fidx, u, lists=lists)
        return (pts * gp).sum() + M.mesh_laplacian_smoothing(x, batch.nv, t).sum() + (M.mesh_edge_loss(x, batch.nv, t, own) * c2).sum()

    eager = grad_of(f)
    x = x0.clone().requires_grad_()
    out = torch.compile(f, fullgraph=True, backend="aot_eager")(x)
    (g,) = torch.autograd.grad(out, x)
    assert torch.equal(out.detach(), eager[0]) and torch.equal(g, eager[1])
