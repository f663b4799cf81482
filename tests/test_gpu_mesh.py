"""GPU: the mesh input path above the C ABI -- geoa3_amd.mesh.sample_surface against the restatement of tests/_mesh_ref.py
on three solids, mesh_clouds' two normalised clouds, and Provider/gen_data_mat.py on a mesh directory the test writes
itself (OFF and OBJ files, one with ModelNet's first-line quirk), read back by the dataset."""
import importlib.util
import os

import numpy as np
import pytest
import torch
from scipy.io import loadmat

from tests import _mesh_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
SOLIDS = [R.cube(), R.tetrahedron(), R.prism()]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_sample_surface_against_the_restatement():
    from geoa3_amd import mesh
    s = 777
    u = np.random.default_rng(11).random((3, s, 3)).astype(F)
    packed = mesh.pack_meshes(SOLIDS)
    pts, nrm, fidx, bad = mesh.sample_surface(packed, s, u=torch.from_numpy(u).cuda())
    assert pts.shape == (3, 3, s) and nrm.shape == (3, 3, s) and fidx.shape == (3, s) and fidx.dtype == torch.int32
    assert bad.tolist() == [0, 0, 0]
    pts, nrm, fidx = pts.cpu().numpy(), nrm.cpu().numpy(), fidx.cpu().numpy()
    for j, (v, f) in enumerate(SOLIDS):
        p_ref, n_ref, f_ref, _ = R.sample(v, f, u[j])
        assert np.array_equal(fidx[j], f_ref)
        assert np.array_equal(pts[j].T.view(np.int32), p_ref.view(np.int32))
        assert np.abs(nrm[j].T.astype(np.float64) - n_ref).max() <= 2.0 ** -23
        assert len(set(f_ref.tolist())) == len(f)                     # every face of every solid is hit
    # the plain 4-tuple is accepted too, and draws of its own are made when none are given
    g = torch.Generator(device="cuda").manual_seed(5)
    a = mesh.sample_surface(tuple(packed[:4]), 100, generator=g)
    b = mesh.sample_surface(packed, 100, generator=torch.Generator(device="cuda").manual_seed(5))
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a[:2], b[:2])) and torch.equal(a[2], b[2])
    assert (a[2] >= 0).all() and not torch.isnan(a[0]).any()


def test_mesh_clouds_are_normalised_and_reproducible():
    from geoa3_amd import mesh
    packed = mesh.pack_meshes(SOLIDS)
    s, n_small, n_dense = 2048, 64, 256
    u = torch.rand(3, s, 3, generator=torch.Generator().manual_seed(2)).cuda()
    first = (torch.tensor([0, 5, 9]).cuda(), torch.tensor([7, 7, 1000]).cuda())
    (pts, nrm), (dpts, dnrm) = mesh.mesh_clouds(packed, n_small, n_dense, surface_samples=s, first=first, u=u)
    for p, n, m in ((pts, nrm, n_small), (dpts, dnrm, n_dense)):
        assert p.shape == (3, 3, m) and n.shape == (3, 3, m)
        p64, n64 = p.double().cpu(), n.double().cpu()
        # geoa3_normalize_cloud in float32: the mean is a sum of m terms (each addition within 2^-24 of a partial sum that
        # the scale keeps near 1), then one subtraction and one division per coordinate
        assert p64.mean(2).abs().max() <= (m + 3) * 2.0 ** -24
        assert (p64.norm(dim=1).max(1)[0] - 1).abs().max() <= 8 * 2.0 ** -24
        # a face normal: three components each rounded once from a unit vector in double
        assert (n64.norm(dim=1) - 1).abs().max() <= 3 * 2.0 ** -24
    # the cube's normals are its axes, exactly
    cube_n = nrm[0].cpu().t()
    assert ((cube_n.abs() == 1).sum(1) == 1).all() and ((cube_n == 0).sum(1) == 2).all()
    again = mesh.mesh_clouds(packed, n_small, n_dense, surface_samples=s, first=first, u=u)
    for x, y in zip((pts, nrm, dpts, dnrm), again[0] + again[1]):
        assert torch.equal(_bits(x), _bits(y))
    small_only = mesh.mesh_clouds(packed, n_small, 0, surface_samples=s, first=first[0], u=u)
    assert small_only[1] is None and torch.equal(_bits(small_only[0][0]), _bits(pts))


def _tool():
    spec = importlib.util.spec_from_file_location(
        "gen_data_mat", os.path.join(os.path.dirname(__file__), "..", "Provider", "gen_data_mat.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def _scaled(solid, k):
    v, f = solid
    return (v * F(1.0 + 0.25 * k) + F(0.125 * k)).astype(F), f


def test_gen_data_mat_on_point_files(tmp_path):
    """the reference's own source: <datadir>/<class>/<id>.txt rows x,y,z,nx,ny,nz listed by modelnet40_test.txt; the first
    npoint rows, points centred and scaled, normals as they are; -outc = the number of names takes every class"""
    tool = _tool()
    root = tmp_path / "resampled"
    names = ["chair", "night_stand", "vase"]
    ids = ["chair_0001", "chair_0002", "night_stand_0001", "vase_0001"]
    root.mkdir()
    (root / "modelnet40_shape_names.txt").write_text("\n".join(names) + "\n")
    (root / "modelnet40_test.txt").write_text("\n".join(ids) + "\n")
    (root / "modelnet40_train.txt").write_text("vase_0002\n")
    g = np.random.default_rng(6)
    rows = {}
    for i in ids:
        name = "_".join(i.split("_")[:-1])
        (root / name).mkdir(exist_ok=True)
        rows[i] = g.standard_normal((48, 6)).astype(F)
        np.savetxt(str(root / name / (i + ".txt")), rows[i], delimiter=",", fmt="%.9g")
    cfg = tool.build_parser().parse_args(["--datadir", str(root), "--out_datadir", str(tmp_path / "Data"), "-outc", "3",
                                          "--npoint", "32", "--synthetic", "--keep_misclassified", "--seed", "1"])
    written = tool.main(cfg)
    assert [os.path.basename(w) for w in written] == ["modelnet3_4instances32_PointNet.mat"]     # no dense file here
    mat = loadmat(written[0])
    assert mat["data"].shape == (4, 3, 32) and mat["label"].ravel().tolist() == [0, 0, 1, 2]
    # two instances of `chair` in a drawn order: match each written instance to its file by its (untouched) normals
    for j in range(4):
        src = [r for r in rows.values() if np.array_equal(r[:32, 3:].T, mat["normal"][j])]
        assert len(src) == 1
        p = src[0][:32, :3].astype(np.float64)
        p = p - p.mean(0)
        want = (p / np.linalg.norm(p, axis=1).max()).T
        # fp32 subtraction and division of values <= 1 after an fp32-rounded mean and scale: a few 2^-24
        assert np.abs(mat["data"][j] - want).max() <= 8 * 2.0 ** -24


def test_gen_data_mat_on_a_mesh_directory(tmp_path, capsys):
    """three classes, OFF and OBJ files, one OFF with `OFF8 12 0` on its first line and one OBJ face that names a vertex
    the file does not hold: both .mat files in the reference's schema, and the dataset loads them"""
    from geoa3_amd import mesh
    from geoa3_amd.data import ModelNet40
    tool = _tool()
    root = tmp_path / "meshes"
    names = ["chair", "lamp", "table", "vase"]                      # `lamp` is not one of the ten: passed over
    (tmp_path / "names.txt").write_text("\n".join(names) + "\n")
    count = {"chair": 3, "table": 2, "vase": 4}
    for c, (name, solid) in enumerate(zip(("chair", "table", "vase"), SOLIDS)):
        folder = root / name / "test"
        folder.mkdir(parents=True)
        (root / name / "train").mkdir()
        for k in range(count[name]):
            v, f = _scaled(solid, k)
            if (c + k) % 2:
                mesh.write_obj(str(folder / ("%s_%04d.obj" % (name, k))), v, f)
            else:
                mesh.write_off(str(folder / ("%s_%04d.off" % (name, k))), v, f)
    v, f = R.cube()
    (root / "chair" / "test" / "chair_quirk.off").write_text(
        "\n".join(["OFF8 12 0"] + ["%r %r %r" % tuple(x) for x in v.tolist()] + ["3 %d %d %d" % tuple(x) for x in f.tolist()])
        + "\n")
    count["chair"] += 1
    with open(root / "vase" / "test" / "vase_0001.obj", "a") as fp:
        fp.write("f 1 2 99\n")
    out = tmp_path / "Data"
    cfg = tool.build_parser().parse_args(["--mesh_dir", str(root), "--shape_names_file", str(tmp_path / "names.txt"),
                                          "--out_datadir", str(out), "--npoint", "64", "--dense_npoints", "256",
                                          "--surface_samples", "1024", "--synthetic", "--keep_misclassified", "--seed", "0"])
    assert cfg.split == "test" and not cfg.swap_yz and cfg.arch == "PointNet" and cfg.out_classes == 10
    written = tool.main(cfg)
    assert "vase_0001.obj: 1 bad faces" in capsys.readouterr().out
    total = sum(count.values())
    assert [os.path.basename(w) for w in written] == ["modelnet10_%dinstances64_PointNet.mat" % total,
                                                      "modelnet10_%dinstances256_PointNet.mat" % total]
    want_label = [0] * 4 + [2] * 2 + [3] * 4                         # TEN_LABEL_NAMES order: chair, table, vase
    for path, n in zip(written, (64, 256)):
        mat = loadmat(path)
        assert mat["data"].shape == (total, 3, n) and mat["normal"].shape == (total, 3, n)
        assert mat["data"].dtype == F and mat["normal"].dtype == F
        assert mat["label"].shape == (total, 1) and mat["label"].ravel().tolist() == want_label
        assert np.isfinite(mat["data"]).all()
        assert np.abs(np.linalg.norm(mat["data"].astype(np.float64), axis=1).max(1) - 1).max() <= 8 * 2.0 ** -24
        assert np.abs(np.linalg.norm(mat["normal"].astype(np.float64), axis=1) - 1).max() <= 3 * 2.0 ** -24
        ds = ModelNet40(data_mat_file=path, attack_label="Untarget")
        assert len(ds) == total
        pc, nm, gt = ds[total - 1]
        assert pc.shape == (1, n, 3) and nm.shape == (1, n, 3) and gt.tolist() == [3]
    # the same seed writes the same bits; --swap_yz permutes the stored axes
    first = loadmat(written[0])
    again = tool.main(cfg)
    assert np.array_equal(loadmat(again[0])["data"].view(np.int32), first["data"].view(np.int32))
    cfg.swap_yz, cfg.out_datadir = True, str(tmp_path / "Swapped")
    swapped = loadmat(tool.main(cfg)[0])
    assert np.array_equal(swapped["data"], first["data"][:, [0, 2, 1]])
    assert np.array_equal(swapped["normal"], first["normal"][:, [0, 2, 1]])
