"""GPU: the mesh attack's loop (geoa3_amd/mesh_attack.py) and its command line.  Every case: b = 4 twice-subdivided icosahedra
(162 vertices, 320 faces, each stretched differently: geoa3_amd.mesh_attack.synthetic_meshes), S = 256 surface points, the
synthetic PointNet of the oracle (the DGCNN case: S = 64, the smallest cloud its k = 20 graph is tested on)."""
import glob
import os

import numpy as np
import pytest
import scipy.io as sio
import torch

from oracle import geoa3_oracle as O
from tests import _mesh_attack_ref as R
from tests.test_gpu_mesh_attack_kernels import U, _forward_bounds, _grad_bounds

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
B, V, S = 4, 162, 256
W_LAP, W_EDGE = 0.5, 20.0


@pytest.fixture(scope="module")
def net():
    from geoa3_amd.pointnet import PointNet
    n = PointNet(40)
    n.load_state_dict(O.make_pointnet_state_dict(40, seed=0))
    return n.cuda().eval()


def _meshes():
    from geoa3_amd.mesh_attack import synthetic_meshes
    return synthetic_meshes(B, seed=0)


def _draw(s=S, seed=7):
    return torch.rand(B, s, 3, generator=torch.Generator().manual_seed(seed))


def _inits(steps, scale=1e-2, seed=8):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, 3, V, generator=g) * scale for _ in range(steps)]


def _cfg(**kw):
    base = dict(npoint=S, curv_loss_knn=8, binary_max_steps=1, iter_max_steps=1, laplacian_loss_weight=W_LAP,
                edge_loss_weight=W_EDGE)
    base.update(kw)
    return O.AttackCfg(**base)


def _runner(net, cfg, u):
    from geoa3_amd import mesh
    from geoa3_amd.mesh_attack import MeshAttackRunner
    packed = mesh.pack_meshes(_meshes())
    r = MeshAttackRunner(net, B, V, cfg, torch.device("cuda"))
    gt = torch.tensor([0, 3, 7, 11])
    r.setup_mesh(packed, gt, gt, u=u)
    return r


def _state(r):
    torch.cuda.synchronize()
    out = {}
    for k, v in r.t.items():
        if k.endswith("scratch"):          # uninitialised work buffers of geoa3_knn_self: no state of the attack
            continue
        if isinstance(v, torch.Tensor):
            out[k] = v.detach().cpu().clone()
        else:
            out.update({"%s[%d]" % (k, n): e.detach().cpu().clone() for n, e in enumerate(v)})
    return out


# ------------------------------------------------------------------ one iteration, geometry only
def test_one_iteration_geometry_only_against_the_float64_composition(net):
    """cls_loss_type = "None"; CD + 0.1 HD + curvature on xe = S(x), plus W_LAP Lap + W_EDGE Edge on x, in float64:
    the oracle's point terms (oracle/geoa3_oracle.py) evaluated at the float32 points S(x) -- S is DEFINED in float32, and
    the kernel's points are held to its restatement bit for bit here -- their gradient pulled back through S^T with the
    float32 weights, and the restatement's mesh terms with the clean mesh's own float32 edge lengths as target.
    Bounds: the point objective's of tests/test_gpu_geometry.py (constrain: rtol 5e-5 + 1e-7; gradient with the curvature
    term, ordered sums: rtol 1e-4 + 2e-6 per point entry), carried through the pullback entry by entry (weights >= 0), plus
    the pullback's own (n + 2) u mag, plus the mesh terms' derived bounds (tests/test_gpu_mesh_attack_kernels.py) times
    their weights, plus one float32 rounding per fold / add."""
    cfg = _cfg(cls_loss_type="None")
    u = _draw()
    r = _runner(net, cfg, u)
    r.begin_search_step(_inits(1)[0])
    g_cls, g_geo = r.objective(0, 0)
    torch.cuda.synchronize()
    assert g_cls is None and g_geo.shape == (B, 3, V)
    x = r.t["x"].cpu().numpy()
    xe = r.t["xe"].cpu().numpy()
    fidx, un = r.face_idx.cpu().numpy(), u.numpy()
    meshes = _meshes()
    k = cfg.curv_loss_knn
    ori, nrm = r.geo_ori.cpu().double(), r.geo_nrm.cpu().double()
    for b, (v, f) in enumerate(meshes):
        assert np.array_equal(xe[b].T.view(np.int32), R.points32(x[b].T, f, fidx[b], un[b]).view(np.int32)), b
    adv = torch.from_numpy(xe).double().requires_grad_()
    kap_ori = O.get_kappa_ori(ori, nrm, k)
    kap_adv, _ = O.get_kappa_adv(adv, ori, nrm, k)
    con_pts = (O.chamfer_loss(adv, ori) + cfg.hd_loss_weight * O.hausdorff_loss(adv, ori)
               + cfg.curv_loss_weight * O.curvature_loss(adv, ori, kap_adv, kap_ori))
    (g_pts,) = torch.autograd.grad(con_pts.sum(), adv)
    con_pts, g_pts = con_pts.detach().numpy(), g_pts.numpy()
    target = r.edge_target.cpu().numpy()
    off = r.topo.row_off.cpu().numpy()
    got_con, got_g = r.geo_out["constrain"].cpu().numpy(), g_geo.cpu().numpy()
    assert np.array_equal(got_g, r.t["g_geo_full"].cpu().numpy())
    for b, (v, f) in enumerate(meshes):
        _, nbrs = R.topology(V, f)
        tgt = target[off[b * V]:off[(b + 1) * V]].astype(D)
        xb = x[b].T
        (lap, lap_tol), (edge, edge_tol) = _forward_bounds(xb, nbrs, tgt)
        assert lap > 1e-3 and edge > 1e-6                       # both terms are there to be compared
        want = con_pts[b] + W_LAP * lap + W_EDGE * edge
        tol = 5e-5 * abs(con_pts[b]) + 1e-7 + W_LAP * lap_tol + W_EDGE * edge_tol + 3 * U * abs(want)
        assert abs(got_con[b] - want) <= tol, (b, got_con[b], want, tol)
        np.testing.assert_allclose(r.t["lap_loss"][b].item(), lap, rtol=0, atol=lap_tol)
        np.testing.assert_allclose(r.t["edge_loss"][b].item(), edge, rtol=0, atol=edge_tol)
        # the gradient on the vertices
        gp = g_pts[b].T
        pulled, mag, terms = R.pullback64(gp, V, f, fidx[b], un[b])
        carried, _, _ = R.pullback64(1e-4 * np.abs(gp) + 2e-6, V, f, fidx[b], un[b])
        (dl, tl), (de, te) = _grad_bounds(xb, nbrs, tgt)
        mesh_g = W_LAP * dl + W_EDGE * de
        want = pulled + mesh_g
        tol = (carried + (terms[:, None] + 2) * U * mag + W_LAP * tl + W_EDGE * te + U * np.abs(mesh_g) + U * np.abs(want)
               + 1e-30)
        err = np.abs(got_g[b].T - want)
        assert (err <= tol).all(), (b, float((err / tol).max()))
        assert np.abs(mesh_g).max() > 1e-3 * np.abs(want).max() and np.abs(pulled).max() > 1e-3 * np.abs(want).max()


# ------------------------------------------------------------------ flag-off identity
def test_mesh_weights_zero_is_the_point_objective_on_xe_bit_for_bit(net):
    from geoa3_amd.attack import AttackRunner
    cfg = _cfg(cls_loss_type="None", laplacian_loss_weight=0.0, edge_loss_weight=0.0)
    u = _draw()
    r = _runner(net, cfg, u)
    r.begin_search_step(_inits(1)[0])
    _, g_geo = r.objective(0, 0)
    torch.cuda.synchronize()
    p = AttackRunner(net, B, S, cfg, torch.device("cuda"))
    gt = torch.tensor([0, 3, 7, 11])
    p.setup(r.geo_ori, r.geo_nrm, gt, gt)
    p.begin_search_step(torch.zeros(B, 3, S))
    p.t["x"].copy_(r.t["xe"])
    _, pg = p.objective(0, 0)
    torch.cuda.synchronize()
    for name in ("constrain", "dis_loss", "hd_loss", "curv_loss"):
        assert torch.equal(p.geo_out[name], r.geo_out[name]), name
    assert torch.equal(pg, r.t["g_geo"]) and float(r.geo_out["constrain"].abs().min()) > 0
    # ... and the vertex-level gradient is that gradient's ordered pullback, nothing else
    from geoa3_amd import mesh
    assert torch.equal(g_geo, mesh.mesh_points_backward(pg, r.u, r.lists, V))


# ------------------------------------------------------------------ replay
def test_two_runs_from_the_same_draw_are_bit_identical(net):
    """2 binary steps x 8 iterations, twice from the same draw and initial offsets: every state buffer bit-identical (the
    property tests/test_gpu_replay.py holds for clouds)"""
    from geoa3_amd import mesh
    from geoa3_amd.mesh_attack import MeshAttackRunner, attack_mesh
    cfg = _cfg(binary_max_steps=2, iter_max_steps=8)
    u, inits = _draw().cuda(), [o.cuda() for o in _inits(2, 1e-3)]
    gt = torch.tensor([0, 3, 7, 11])
    states, outs = [], []
    for _ in range(2):
        r = MeshAttackRunner(net, B, V, cfg, torch.device("cuda"))
        out = attack_mesh(net, mesh.pack_meshes(_meshes()), gt, gt, cfg, init_offsets=inits, hooks={"mesh_u": lambda: u},
                          runner=r)
        states.append(_state(r))
        outs.append(out)
    assert states[0].keys() == states[1].keys() and len(states[0]) > 25
    for k in states[0]:
        assert np.array_equal(states[0][k].numpy().view(np.uint8), states[1][k].numpy().view(np.uint8)), k
    for name in ("xe", "g_cls_full", "g_geo_full", "mesh_unit", "lap_loss", "edge_loss", "best_attack", "m", "v", "offset"):
        assert name in states[0]
    adv, target, success, best_step, hist = outs[0]
    assert len(adv) == B and all(a.shape == (3, V) for a in adv) and target.tolist() == gt.tolist()
    assert len(success) == B and len(best_step) == B and len(hist) == 8
    assert all(torch.equal(a, b) for a, b in zip(adv, outs[1][0]))
    ori = mesh.to_planar(mesh.pack_meshes(_meshes()))[0].cpu()
    assert not torch.equal(states[0]["x"], ori) and torch.isfinite(states[0]["x"]).all()        # the iterate moved
    assert float(states[0]["lap_loss"].min()) > 0 and float(states[0]["edge_loss"].min()) > 0


# ------------------------------------------------------------------ victims
def test_native_victim_takes_a_step(net):
    cfg = _cfg()
    r = _runner(net, cfg, _draw())
    assert r.native
    init = _inits(1, 1e-3)[0]
    r.begin_search_step(init)
    x0 = r.t["x"].clone()
    r.step(0, 0)
    torch.cuda.synchronize()
    moved = (r.t["x"] - x0).abs()
    assert torch.isfinite(r.t["x"]).all() and float(moved.max()) > 1e-3 and float(r.t["g_cls_full"].abs().max()) > 0
    assert 0.5 * cfg.lr < float(moved.max()) <= 1.01 * cfg.lr          # the first Adam step is lr in every moved coordinate


def test_autograd_victim_takes_a_step():
    from tests.test_gpu_dgcnn import make_net
    dg = make_net(16).cuda()
    cfg = _cfg(npoint=64)
    r = _runner(dg, cfg, _draw(64))
    assert not r.native and r.ne == 64
    r._freeze()
    try:
        r.begin_search_step(_inits(1, 1e-3)[0])
        x0 = r.t["x"].clone()
        r.step(0, 0)
        torch.cuda.synchronize()
    finally:
        r._unfreeze()
    assert torch.isfinite(r.t["x"]).all() and float((r.t["x"] - x0).abs().max()) > 1e-3
    assert float(r.t["g_cls_full"].abs().max()) > 0 and float(r.t["g_geo_full"].abs().max()) > 0


def test_setup_refuses_a_mesh_without_area_by_name(net):
    from geoa3_amd import mesh
    from geoa3_amd.mesh_attack import MeshAttackRunner
    meshes = _meshes()
    flat = (np.zeros_like(meshes[2][0]), meshes[2][1])                    # every vertex at the origin: no area
    r = MeshAttackRunner(net, B, V, _cfg(), torch.device("cuda"))
    gt = torch.tensor([0, 3, 7, 11])
    with pytest.raises(ValueError, match="mesh 2 .*no surface area"):
        r.setup_mesh(mesh.pack_meshes(meshes[:2] + [flat] + meshes[3:]), gt, gt)
    broken = (meshes[1][0], meshes[1][1].copy())
    broken[1][5, 1] = V + 3
    with pytest.raises(ValueError, match="mesh 1 .*1 bad faces"):
        r.setup_mesh(mesh.pack_meshes(meshes[:1] + [broken] + meshes[2:]), gt, gt)


# ------------------------------------------------------------------ command line
def test_main_attack_mesh_end_to_end(tmp_path, monkeypatch):
    import main_attack
    from geoa3_amd import mesh
    monkeypatch.chdir(tmp_path)
    args = ["--attack", "GeoA3_mesh", "--attack_label", "Untarget", "--synthetic", "-b", "4", "--npoint", "256",
            "--binary_max_steps", "1", "--iter_max_steps", "4", "--curv_loss_knn", "8", "--laplacian_loss_weight", "0.5",
            "--edge_loss_weight", "20", "--initial_const", "0.01", "--lr", "0.05", "--quiet"]
    saved_dir = main_attack.main(main_attack.build_parser().parse_args(args))
    assert saved_dir.startswith(os.path.join("Exps", "PointNet_npoint256", "Untarget", "GeoA3_mesh_0_BiStep1_IterStep4_"))
    assert saved_dir.endswith("_LapLoss0.5_EdgeLoss20.0")
    res = open(os.path.join(saved_dir, "attack_result.txt")).read()
    assert res.startswith("attack success: ")
    rate = float(res.split(":")[1])
    objs = sorted(glob.glob(os.path.join(saved_dir, "Mesh", "*.obj")))
    mats = sorted(glob.glob(os.path.join(saved_dir, "Mat", "*.mat")))
    assert len(objs) == len(mats) == round(rate / 100 * 4)
    faces = _meshes()[0][1]
    for obj, mat in zip(objs, mats):
        name = os.path.basename(obj)[:-4]
        assert name == os.path.basename(mat)[:-4] and name.startswith("adv_") and "_gt" in name and "_attack" in name
        v, f = mesh.read_obj(obj)
        assert v.shape == (162, 3) and np.array_equal(f, faces) and np.isfinite(v).all()
        m = sio.loadmat(mat)
        assert np.array_equal(m["faces"], faces) and np.array_equal(m["vert"].astype(F).view(np.int32), v.view(np.int32))
    assert objs, "with a constant of 0.01 and lr 0.05 the untargeted attack on the synthetic victim succeeds within 4 steps"
