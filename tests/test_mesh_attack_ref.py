"""CPU: the float64 restatements of tests/_mesh_attack_ref.py against central differences, MeshTopology.from_packed against
the restatement's edge sets and neighbour order, the new entries' declarations (header and ctypes mirror), and the command
line of --attack GeoA3_mesh (parsing, directory name, refusals, the synthetic meshes)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import _mesh_attack_ref as R

F, D = np.float32, np.float64
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ------------------------------------------------------------------ gradients against central differences
def _central(fn, v, h=1e-6):
    g = np.zeros_like(v)
    for i in range(v.shape[0]):
        for c in range(3):
            vp, vm = v.copy(), v.copy()
            vp[i, c] += h
            vm[i, c] -= h
            g[i, c] = (fn(vp) - fn(vm)) / (2 * h)
    return g


@pytest.mark.parametrize("name", sorted(R.cases()))
def test_gradients_against_central_differences(name):
    """Central differences in float64 with h = 1e-6 on coordinates of magnitude <= 3 and lengths >= 0.08 (the shortest
    edge of fan_70's ring is 2 sin(pi/70) = 0.0897): truncation h^2 f''' / 6 <= 1e-12 / l^2 < 2e-10, rounding
    2^-53 |f| / h < 1e-9.  Tolerance 1e-7.  At the kinks the cases hold ON PURPOSE (delta_hub = 0, l_56 = 0 in
    `coincident`) the difference quotient is symmetric, so it gives the 0 the definitions choose there."""
    verts, faces = R.cases()[name]
    v = verts.astype(D)
    edges, nbrs = R.topology(len(v), faces)
    rng = np.random.default_rng(len(v))
    target = np.zeros(sum(len(n) for n in nbrs), D)      # a per-edge target: the same value on both directions of an edge
    value = {tuple(e): t for e, t in zip(edges.tolist(), rng.uniform(0.2, 1.5, len(edges)))}
    q = 0
    for i, n in enumerate(nbrs):
        for j in n:
            target[q] = value[(min(i, j), max(i, j))]
            q += 1
    np.testing.assert_allclose(R.laplacian_grad(v, nbrs), _central(lambda x: R.laplacian(x, nbrs)[0], v), rtol=0, atol=1e-7)
    for t in (0.0, 0.7, target):
        np.testing.assert_allclose(R.edge_grad(v, nbrs, t), _central(lambda x: R.edge(x, nbrs, t), v), rtol=0, atol=1e-7)
    if name == "coincident":
        _, norm, unit = R.laplacian(v, nbrs)
        assert norm[0] == 0 and not unit[0].any() and R.lengths(v, nbrs).min() == 0
    if name == "isolated":
        assert len(nbrs[4]) == 0 and not R.laplacian_grad(v, nbrs)[4].any() and not R.edge_grad(v, nbrs, 0.7)[4].any()
    if name == "fan_70":
        assert len(nbrs[0]) == 70
    # the edge term with the mesh's own lengths as target: zero with a zero gradient
    own = R.lengths(v, nbrs)
    assert R.edge(v, nbrs, own) == 0 and not R.edge_grad(v, nbrs, own).any()


def test_laplacian_and_edge_on_a_hand_worked_mesh():
    """one triangle (0,0,0), (3,0,0), (0,4,0): delta_0 = (1.5, 2, 0), delta_1 = (-3, 2, 0), delta_2 = (1.5, -4, 0); lengths 3, 4, 5"""
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], D)
    edges, nbrs = R.topology(3, [[0, 1, 2]])
    assert edges.tolist() == [[0, 1], [0, 2], [1, 2]] and [n.tolist() for n in nbrs] == [[1, 2], [0, 2], [0, 1]]
    lap, norm, _ = R.laplacian(v, nbrs)
    assert norm.tolist() == [2.5, np.sqrt(13.0), np.sqrt(18.25)] and lap == (2.5 + np.sqrt(13.0) + np.sqrt(18.25)) / 3
    assert R.edge(v, nbrs, 0.0) == (9 + 16 + 25) / 3 and R.edge(v, nbrs, 3.0) == (0 + 1 + 4) / 3
    assert R.lengths(v, nbrs).tolist() == [3, 4, 3, 5, 4, 5]


def test_pullback_restatements_agree_and_points_match_the_sampler_form():
    from tests import _mesh_ref as S
    rng = np.random.default_rng(2)
    v, f = R.subdivide(*R.octahedron())
    u = rng.random((300, 3)).astype(F)
    fidx = rng.integers(0, len(f), 300).astype(np.int32)
    fidx[7] = -1
    p32 = R.points32(v, f, fidx, u)
    assert np.array_equal(p32.view(np.int32), S.points(v, f, fidx, u).view(np.int32))        # the sampler's restatement
    assert np.isnan(p32[7]).all() and np.isfinite(np.delete(p32, 7, 0)).all()
    np.testing.assert_allclose(p32, R.points64(v, f, fidx, u), rtol=0, atol=4 * 2.0 ** -24, equal_nan=True)
    g = rng.standard_normal((300, 3)).astype(F)
    g64, mag, terms = R.pullback64(g, len(v), f, fidx, u)
    assert terms.sum() == 3 * 299
    assert (np.abs(R.pullback32(g, len(v), f, fidx, u) - g64) <= (terms[:, None] + 2) * 2.0 ** -24 * mag).all()
    # <S(v), g> = <v, S^T g>: the pullback is the transpose of the point map
    keep = fidx >= 0
    assert abs((R.points64(v, f, fidx, u)[keep] * g[keep]).sum() - (v.astype(D) * g64).sum()) < 1e-9


# ------------------------------------------------------------------ topology
def _ragged_batch():
    tet, octa = R.tetrahedron(), R.subdivide(*R.octahedron())
    empty = (np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    v, f = R.fan(5)
    odd = (v, np.concatenate([f, [[0, 1, 9]], [[2, 2, 3]], [[-1, 0, 1]], [[4, 4, 4]]]).astype(np.int32))
    return [tet, empty, octa, odd, R.isolated()]


def test_topology_from_packed_matches_the_restatement():
    """a ragged batch with an empty mesh, faces with an out-of-range index (contribute nothing) and faces that repeat an
    index (only their i != j pairs: [2,2,3] gives {2,3}, [4,4,4] nothing)"""
    from geoa3_amd import mesh
    meshes = _ragged_batch()
    packed = mesh.pack_meshes(meshes, device="cpu")
    topo = mesh.MeshTopology.from_packed(packed)
    vp = max(len(v) for v, _ in meshes)
    assert topo.vp == vp and topo.batch == 5 and topo.nv.tolist() == [len(v) for v, _ in meshes]
    row_off, col = topo.row_off.numpy(), topo.col.numpy()
    assert topo.row_off.dtype == topo.col.dtype == topo.ne.dtype == topo.edges.dtype == topo.nv.dtype
    assert str(topo.col.dtype) == "torch.int32" and len(row_off) == 5 * vp + 1 and row_off[-1] == len(col) == topo.nnz
    eo = topo.edge_off.numpy()
    for b, (v, f) in enumerate(meshes):
        edges, nbrs = R.topology(len(v), f)
        assert topo.ne[b].item() == len(edges)
        assert topo.edges.numpy()[eo[b]:eo[b + 1]].tolist() == edges.tolist()
        for i in range(vp):
            row = col[row_off[b * vp + i]:row_off[b * vp + i + 1]].tolist()
            assert row == (nbrs[i].tolist() if i < len(v) else []), (b, i)       # ascending; a padding row is empty
    edges, nbrs = R.topology(6, meshes[3][1])
    assert [2, 3] in edges.tolist() and nbrs[4].tolist() == [0, 3, 5]        # ([4,4,4] adds nothing, [0,1,9] neither)
    wide = mesh.MeshTopology.from_packed(packed, vp=vp + 3)
    assert wide.vp == vp + 3 and wide.col.tolist() == topo.col.tolist() and len(wide.row_off) == 5 * (vp + 3) + 1
    with pytest.raises(ValueError):
        mesh.MeshTopology.from_packed(packed, vp=vp - 1)


def test_to_planar_and_back():
    import torch
    from geoa3_amd import mesh
    meshes = _ragged_batch()
    packed = mesh.pack_meshes(meshes, device="cpu")
    verts, nv = mesh.to_planar(packed)
    assert verts.shape == (5, 3, 18) and nv.tolist() == [4, 0, 18, 6, 5] and nv.dtype == torch.int32
    for b, (v, _) in enumerate(meshes):
        assert np.array_equal(verts[b, :, :len(v)].numpy(), v.T) and not verts[b, :, len(v):].any()
    back = mesh.from_planar(verts + 1.0, nv, packed)
    assert torch.equal(back.verts, packed.verts + 1.0) and back.faces is packed.faces and back.max_faces == packed.max_faces


# ------------------------------------------------------------------ ABI
def test_binding_and_header_declare_the_mesh_attack_entries():
    from geoa3_amd import _lib
    vp, i64, i, fl = C.c_void_p, C.c_int64, C.c_int, C.c_float
    want = {
        "geoa3_mesh_points": (i, [vp] * 6 + [i, i, i, i64, vp, vp]),
        "geoa3_mesh_corner_index": (i, [vp] * 4 + [i, i, i, i64, vp, vp]),
        "geoa3_mesh_points_scratch_bytes": (i64, [i, i, i]),
        "geoa3_mesh_points_lists": (i, [vp, i, i, i, vp, vp]),
        "geoa3_mesh_points_grad": (i, [vp, vp, vp, i, i, i, vp, vp]),
        "geoa3_mesh_reg": (i, [vp] * 6 + [fl, i, i, i, fl, fl, vp, vp, vp, vp, i, vp]),
        "geoa3_mesh_reg_grad": (i, [vp] * 6 + [fl, vp, vp, vp, fl, fl, i, i, i, vp, i, vp]),
        "geoa3_mesh_edge_lengths": (i, [vp] * 4 + [i, i, i, vp, vp]),
    }
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name
    text = open(os.path.join(REPO, "include", "geoa3_hip.h")).read()
    hdr = re.sub(r"\s+", " ", text)
    for decl in (
            "int geoa3_mesh_points(const float* verts, const int32_t* nv, const int32_t* faces, const int64_t* face_off, "
            "const int32_t* face_idx, const float* u, int B, int Vp, int S, int64_t total_faces, float* pts, void* stream);",
            "int geoa3_mesh_corner_index(const int32_t* nv, const int32_t* faces, const int64_t* face_off, "
            "const int32_t* face_idx, int B, int Vp, int S, int64_t total_faces, int32_t* corner, void* stream);",
            "int64_t geoa3_mesh_points_scratch_bytes(int B, int Vp, int S);",
            "int geoa3_mesh_points_lists(const int32_t* corner, int B, int Vp, int S, void* scratch, void* stream);",
            "int geoa3_mesh_points_grad(const float* g_pts, const float* u, const void* scratch, int B, int Vp, int S, "
            "float* g_verts, void* stream);",
            "int geoa3_mesh_reg(const float* verts, const int32_t* nv, const int32_t* row_off, const int32_t* col, "
            "const int32_t* ne, const float* target, float target_scalar, int B, int Vp, int nnz, float w_lap, float w_edge, "
            "float* unit, float* lap, float* edge, float* constrain, int constrain_add, void* stream);",
            "int geoa3_mesh_reg_grad(const float* verts, const int32_t* nv, const int32_t* row_off, const int32_t* col, "
            "const int32_t* ne, const float* target, float target_scalar, const float* unit, const float* g_lap, "
            "const float* g_edge, float w_lap, float w_edge, int B, int Vp, int nnz, float* g_verts, int add, void* stream);",
            "int geoa3_mesh_edge_lengths(const float* verts, const int32_t* nv, const int32_t* row_off, const int32_t* col, "
            "int B, int Vp, int nnz, float* len, void* stream);"):
        assert decl in hdr, decl
    # every entry cites what it stands in for
    assert hdr.count("main_attack.py:27-28, 283-293") >= 1 and hdr.count("sample_points_from_meshes") >= 2
    assert hdr.count("mesh_laplacian_smoothing") >= 3 and hdr.count("mesh_edge_loss") >= 4
    assert int(re.search(r"#define GEOA3_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION == 609
    from geoa3_amd import build as B
    assert B.FILE_FLAGS["mesh_attack.hip"][0] == "-ffp-contract=off" and B.FILE_FLAGS["mesh_sample.hip"][0] == "-ffp-contract=off"


# ------------------------------------------------------------------ command line
def test_mesh_attack_parses_and_names_its_directory():
    import main_attack
    p = main_attack.build_parser()
    cfg = p.parse_args(["--attack", "GeoA3_mesh", "--attack_label", "Untarget", "--synthetic", "--laplacian_loss_weight", "0.5",
                        "--edge_loss_weight", "2"])
    assert cfg.attack == "GeoA3_mesh" and cfg.mesh_dir is None and cfg.mesh_split == "test" and cfg.shape_names_file is None
    name = main_attack.saved_dir_name(cfg)
    assert "GeoA3_mesh_0_" in name and name.endswith("_CurLoss1.0_k16_LapLoss0.5_EdgeLoss2.0")
    plain = main_attack.saved_dir_name(p.parse_args(["--attack", "GeoA3_mesh"]))
    assert "_LapLoss" not in plain and "_EdgeLoss" not in plain


@pytest.mark.parametrize("flags, named", [
    (["--is_subsample_opt"], "--is_subsample_opt"), (["--is_partial_var"], "--is_partial_var"),
    (["--is_pre_jitter_input"], "--is_pre_jitter_input"), (["--is_pro_grad"], "--is_pro_grad"),
    (["--uniform_loss_weight", "0.5"], "--uniform_loss_weight"), (["--is_use_knn_smoothing_loss"], "--is_use_knn_smoothing_loss"),
    (["--displacement_loss_weight", "1"], "--displacement_loss_weight"), (["--repulsion_loss_weight", "1"], "--repulsion_loss_weight"),
    (["--corr_normal_loss_weight", "1"], "--corr_normal_loss_weight")])
def test_mesh_attack_refuses_by_name(flags, named, tmp_path):
    import main_attack
    from geoa3_amd import mesh_attack
    cfg = main_attack.build_parser().parse_args(["--attack", "GeoA3_mesh", "--attack_label", "Untarget", "--synthetic",
                                                 "--out_root", str(tmp_path)] + flags)
    with pytest.raises(ValueError, match=re.escape(named)):
        mesh_attack.refuse_unsupported(cfg)
    with pytest.raises(ValueError, match=re.escape(named)):      # the command line refuses before it touches a device
        main_attack.main(cfg)


def test_mesh_attack_refuses_sharded_runs_and_missing_inputs(tmp_path, monkeypatch):
    import main_attack
    from geoa3_amd import mesh_attack
    p = main_attack.build_parser()
    cfg = p.parse_args(["--attack", "GeoA3_mesh", "--attack_label", "Untarget", "--out_root", str(tmp_path)])
    mesh_attack.refuse_unsupported(cfg)
    with pytest.raises(ValueError, match="sharded"):
        mesh_attack.refuse_unsupported(cfg, world_size=2)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="sharded"):
        main_attack.main(cfg)
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="--mesh_dir"):
        main_attack.load_meshes(cfg)
    with pytest.raises(ValueError, match="--attack_label"):
        main_attack.main(p.parse_args(["--attack", "GeoA3_mesh", "--synthetic", "--out_root", str(tmp_path)]))


def test_synthetic_meshes_are_deterministic_unit_icospheres():
    from geoa3_amd import mesh_attack
    v, f = mesh_attack.icosphere(2)
    assert v.shape == (162, 3) and f.shape == (320, 3) and v.dtype == F and f.dtype == np.int32
    edges, nbrs = R.topology(162, f)
    assert len(edges) == 480 and sorted(set(len(n) for n in nbrs)) == [5, 6]          # V - E + F = 2; 12 vertices of degree 5
    a, b = mesh_attack.synthetic_meshes(4, seed=0), mesh_attack.synthetic_meshes(4, seed=0)
    for (va, fa), (vb, fb) in zip(a, b):
        assert np.array_equal(va.view(np.int32), vb.view(np.int32)) and np.array_equal(fa, fb) and np.array_equal(fa, f)
        assert abs(np.sqrt((va.astype(D) ** 2).sum(1)).max() - 1) < 1e-6 and np.abs(va.astype(D).mean(0)).max() < 1e-6
    assert not np.array_equal(a[0][0], a[1][0])                                        # stretched per instance
    assert not np.array_equal(a[0][0], mesh_attack.synthetic_meshes(1, seed=1)[0][0])


def test_load_meshes_walks_a_mesh_directory(tmp_path):
    import main_attack
    from geoa3_amd import mesh
    names = tmp_path / "names.txt"
    names.write_text("chair\ntable\nempty\n")
    tet, octa = R.tetrahedron(), R.octahedron()
    for cls, fname, (v, f), write in (("chair", "b.off", tet, mesh.write_off), ("chair", "a.obj", octa, mesh.write_obj),
                                      ("table", "t.off", octa, mesh.write_off)):
        d = tmp_path / "root" / cls / "test"
        d.mkdir(parents=True, exist_ok=True)
        write(str(d / fname), v * 3 + 1, f)
    cfg = main_attack.build_parser().parse_args(["--attack", "GeoA3_mesh", "--mesh_dir", str(tmp_path / "root"),
                                                 "--shape_names_file", str(names)])
    items = main_attack.load_meshes(cfg)
    assert [(n, lab) for n, _, _, lab in items] == [("a", 0), ("b", 0), ("t", 1)]
    for _, v, f, _ in items:          # centred, unit radius, faces untouched
        assert abs(np.sqrt((v.astype(D) ** 2).sum(1)).max() - 1) < 1e-6 and np.abs(v.astype(D).mean(0)).max() < 1e-6
    assert np.array_equal(items[1][2], tet[1])
