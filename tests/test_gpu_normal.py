"""GPU: the input side -- PCA normals (geoa3_estimate_normal), the re-sampling helpers and their normalisation
(geoa3_normalize_cloud), the dataset and the command line on a file without normals -- against the float64
restatements of tests/_normal_ref.py, against the kernels they share code with, bit for bit, and end to end."""
import os

import numpy as np
import pytest
import torch
from scipy.io import loadmat, savemat

from tests import _normal_ref as R

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24          # unit roundoff of fp32


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------ same bits as the shared path
@pytest.mark.parametrize("b,n,k", [(2, 64, 3), (3, 257, 16), (1, 1025, 8)])
def test_estimate_normal_is_the_first_eigenvector_of_local_frames(b, n, k):
    """One partial workgroup; a ragged second one; more than one block row (blockIdx.y > 0) -- and, at n = 1025, five
    workgroups per cloud.  The two kernels share local_frame_solve, so the bits agree."""
    from geoa3_amd import utility as U
    from geoa3_amd.data import synthetic_cad_clouds
    pc = synthetic_cad_clouds(b, n, seed=11)[0].cuda()
    _, evecs, idx = U.local_frames(pc, k)
    nrm = U.estimate_normal(pc, k)
    assert nrm.shape == (b, 3, n) and nrm.dtype == torch.float32 and not nrm.requires_grad
    assert torch.equal(_bits(nrm), _bits(evecs[:, 0]))
    assert torch.equal(_bits(U.estimate_normal(pc, k, knn_idx=idx)), _bits(nrm))          # a table handed in
    out = U.estimate_normal(pc, k, "outward")                                            # ... and only the sign moves
    assert torch.equal(_bits(out) & 0x7fffffff, _bits(nrm) & 0x7fffffff)


# ------------------------------------------------------------------ accuracy against float64
@pytest.fixture(scope="module")
def accuracy_clouds():
    from geoa3_amd.data import synthetic_cad_clouds, synthetic_clouds
    return {"ellipsoid": synthetic_clouds(3, 1024, seed=5), "cad": synthetic_cad_clouds(3, 1024, seed=5)}


@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("kind", ["ellipsoid", "cad"])
def test_estimate_normal_against_float64(accuracy_clouds, kind, k):
    """1 - |<n_gpu, n_ref>| <= bound at every point with a relative gap (l1 - l0) / l2 >= 0.05, both sides on the
    neighbour table of the GPU search.  The bound, from the arithmetic (u = 2^-24, R = the largest |coordinate|):
      * the kernel forms C in fp32: the mean by k additions (error <= k u R per axis), k centred differences (u each),
        k products (u each) summed by k additions, the factor 1/(k-1) (2 u) and the conversion.  A shift d of the mean
        enters C only through k d d^T / (k-1) (the centred sum is zero), so entrywise
            |dC_ab| <= (k + 5) u sqrt(C_aa C_bb) + 2 (k u R)^2 <= (k + 5) u l2 + 2 (k u R)^2,
        and |dC|_2 <= |dC|_F <= 3 max_ab |dC_ab|;
      * the eigenvector of a simple eigenvalue turns by sin(t) <= 2 |dC|_2 / (l1 - l0) (Davis-Kahan in the form of
        Yu, Wang & Samworth 2015), and 1 - cos(t) <= sin(t)^2;
      * the fp64 Jacobi (6 sweeps, residual ~1e-16) is far below both; rounding the three components to fp32 moves
        the vector by at most u in norm: 2 u covers it with the reference's own 1e-16.
    Points without that gap (or with l2 = 0) are not compared; more than 5 % of them in a case is a failure."""
    from geoa3_amd import ops, utility as U
    pc = accuracy_clouds[kind][0]
    dev = pc.cuda()
    _, idx = ops.knn_planar(dev, dev, k + 1)
    got = U.estimate_normal(dev, k, knn_idx=idx).cpu().double().numpy()
    idx = idx.cpu().numpy()
    radius = float(pc.abs().max())
    excluded, worst = 0, 0.0
    for j in range(pc.shape[0]):
        ref, w = R.estimate_normal(pc[j].numpy(), idx[j])
        l0, l1, l2 = w[:, 0], w[:, 1], w[:, 2]
        keep = (l2 > 0) & ((l1 - l0) >= 0.05 * l2)
        excluded += int((~keep).sum())
        d_c = 3.0 * ((k + 5) * U32 * l2 + 2.0 * (k * U32 * radius) ** 2)
        sin_t = np.minimum(2.0 * d_c / np.where(keep, l1 - l0, 1.0), 1.0)
        bound = sin_t ** 2 + 2.0 * U32
        err = 1.0 - np.abs((got[j] * ref).sum(axis=0))
        ratio = (err / bound)[keep]
        worst = max(worst, float(ratio.max()))
        print("%s k=%d cloud %d: excluded %d, max err %.3e, max err/bound %.3f, bound %.3e..%.3e" % (
            kind, k, j, int((~keep).sum()), err[keep].max(), ratio.max(), bound[keep].min(), bound[keep].max()))
        assert (err[keep] <= bound[keep]).all(), (kind, k, j, float(ratio.max()))
        np.testing.assert_allclose(np.linalg.norm(got[j], axis=0), 1.0, atol=4 * U32)
    assert excluded <= 0.05 * pc.shape[0] * pc.shape[2], (kind, k, excluded)


# ------------------------------------------------------------------ orientation
def test_orientation_on_ellipsoids(accuracy_clouds):
    from geoa3_amd import utility as U
    pc, given = accuracy_clouds["ellipsoid"]
    dev = pc.cuda()
    canon = U.estimate_normal(dev, 16).cpu()
    out = U.estimate_normal(dev, 16, "outward").cpu()
    dots = (out * given).sum(dim=1)
    assert (dots > 0).all(), int((dots <= 0).sum())                  # outward: along the analytic normal everywhere
    lead = torch.gather(canon, 1, canon.abs().argmax(dim=1, keepdim=True))
    assert (lead > 0).all()                                          # canonical: largest-magnitude component positive
    assert torch.equal(out.abs(), canon.abs())                       # a sign apart, nothing else
    assert not torch.equal(out, canon)
    # the float64 restatement picks the same signs (the dot products with p - c are far from 0 on an ellipsoid)
    idx = U.local_frames(dev[:1].contiguous(), 16)[2]
    ref, _ = R.estimate_normal(pc[0].numpy(), idx[0].cpu().numpy(), "outward")
    assert np.array_equal(np.sign((out[0].double().numpy() * ref).sum(axis=0)), np.ones(pc.shape[2]))


# ------------------------------------------------------------------ loud NaN
def test_nan_coordinate_poisons_exactly_the_rows_that_list_it():
    from geoa3_amd import ops, utility as U
    from geoa3_amd.data import synthetic_clouds
    k = 8
    pc = synthetic_clouds(2, 257, seed=21)[0].cuda()
    _, idx = ops.knn_planar(pc, pc, k + 1)                           # the table of the clean cloud, used for both runs
    clean = U.estimate_normal(pc, k, knn_idx=idx)
    assert torch.isfinite(clean).all()
    bad = pc.clone()
    bad[0, 1, 100] = float("nan")
    got = U.estimate_normal(bad, k, knn_idx=idx)
    lists = (idx[0] == 100).any(dim=1)                               # column 0 included: point 100 itself
    assert lists[100] and 2 <= int(lists.sum()) < 257
    isnan = torch.isnan(got)
    assert torch.equal(isnan[0].all(dim=0), lists) and torch.equal(isnan[0].any(dim=0), lists)
    assert not isnan[1].any()
    assert torch.equal(_bits(got[0][:, ~lists]), _bits(clean[0][:, ~lists]))
    assert torch.equal(_bits(got[1]), _bits(clean[1]))
    # outward: the centroid of cloud 0 is not a number, so none of its normals is; cloud 1 is untouched
    out_clean = U.estimate_normal(pc, k, "outward", idx)
    out = U.estimate_normal(bad, k, "outward", idx)
    assert torch.isnan(out[0]).all() and torch.equal(_bits(out[1]), _bits(out_clean[1]))
    inf = pc.clone()
    inf[0, 2, 7] = float("inf")
    got_inf = U.estimate_normal(inf, k, knn_idx=idx)
    lists7 = (idx[0] == 7).any(dim=1)
    assert torch.equal(torch.isnan(got_inf[0]).all(dim=0), lists7) and torch.isfinite(got_inf[0][:, ~lists7]).all()


# ------------------------------------------------------------------ normalisation
@pytest.mark.parametrize("m", [1, 2, 63, 1024, 5000])
def test_normalize_cloud(m):
    """B = 3 clouds off-centre and of different sizes.  Bounds, from the kernel's arithmetic (u = 2^-24, A = the
    largest |input coordinate|, s = the largest centred norm):
      * mean: the sum is formed in fp64 (error <= m 2^-53 A) and rounded to fp32 (<= u A); p - mean is one fp32
        subtraction (<= u |p - mean| <= u s per point); the quotient by s is formed in fp64 and rounded once (<= u |out|
        <= u).  So every coordinate of the float64 mean of the output is within u (A / s + 2) + m 2^-53 A / s of 0;
      * largest norm: the point that attains s is divided by its own norm, which leaves the rounding of its three
        components, u in norm; no other point is longer than 1 + u.  |max norm - 1| <= 2 u.
    m = 1 is the degenerate case the kernel states: the only point is its own mean, the largest norm is 0, the cloud
    comes out NaN."""
    from geoa3_amd import utility as U
    g = torch.Generator().manual_seed(100 + m)
    pts = torch.randn(3, 3, m, generator=g) * torch.tensor([0.5, 2.0, 7.0]).view(3, 1, 1)
    pts = pts + torch.tensor([[3.0, -2.0, 0.5], [0.0, 0.0, 0.0], [-40.0, 10.0, 25.0]]).view(3, 3, 1)
    out, cen, scale = U.normalize_cloud(pts.cuda(), return_stats=True)
    out, cen, scale = out.cpu(), cen.cpu(), scale.cpu()
    assert out.shape == (3, 3, m) and cen.shape == (3, 3) and scale.shape == (3,)
    if m == 1:
        assert torch.isnan(out).all() and torch.isnan(scale).all()
        assert torch.equal(cen, pts[:, :, 0])
        return
    for j in range(3):
        ref, mean, s = R.normalize_cloud(pts[j].numpy())
        a = float(pts[j].abs().max())
        o = out[j].double().numpy()
        mean_bound = U32 * (a / s + 2.0) + m * 2.0 ** -53 * a / s
        got_mean, got_max = np.abs(o.mean(axis=1)).max(), np.linalg.norm(o, axis=0).max()
        print("m=%d cloud %d: |mean| %.3e (bound %.3e), |max norm - 1| %.3e (bound %.3e)" % (
            m, j, got_mean, mean_bound, abs(got_max - 1.0), 2 * U32))
        assert got_mean <= mean_bound
        assert abs(got_max - 1.0) <= 2 * U32
        # the statistics it reports, and the cloud itself against the restatement (u on the mean, on the difference
        # and on the quotient: 4 u (A / s + 1) covers all three)
        np.testing.assert_allclose(cen[j].double().numpy(), mean, rtol=0, atol=U32 * a + m * 2.0 ** -53 * a)
        assert abs(float(scale[j]) - s) <= 4 * U32 * (a + s)
        assert np.abs(o - ref).max() <= 4 * U32 * (a / s + 1.0)
    # in place gives the same bits
    from geoa3_amd import _lib
    buf = pts.cuda().contiguous()
    _lib.check(_lib.load().geoa3_normalize_cloud(buf.data_ptr(), buf.data_ptr(), 3, m, None, None,
                                                 torch.cuda.current_stream().cuda_stream))
    assert torch.equal(_bits(buf), _bits(out))


def test_normalize_cloud_degenerate_instance_is_nan_and_alone():
    from geoa3_amd import utility as U
    g = torch.Generator().manual_seed(7)
    pts = torch.randn(3, 3, 63, generator=g) + 1.5
    want = U.normalize_cloud(pts.cuda()).cpu()
    flat = pts.clone()
    flat[1] = torch.tensor([0.3, -1.25, 2.0]).view(3, 1)              # every point of cloud 1 the same
    got, cen, scale = (t.cpu() for t in U.normalize_cloud(flat.cuda(), return_stats=True))
    assert torch.isnan(got[1]).all() and torch.isnan(scale[1]) and torch.equal(cen[1], flat[1, :, 0])
    assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[2]), _bits(want[2]))
    hole = pts.clone()
    hole[2, 0, 5] = float("inf")                                     # a non-finite largest norm
    got = U.normalize_cloud(hole.cuda()).cpu()
    assert torch.isnan(got[2]).all() and torch.equal(_bits(got[:2]), _bits(want[:2]))


# ------------------------------------------------------------------ re-sampling
@pytest.mark.parametrize("b,n,m", [(2, 300, 64), (1, 10000, 1024)])
def test_resampling_helpers(b, n, m):
    from geoa3_amd import utility as U
    from geoa3_amd.data import synthetic_cad_clouds
    pc, nrm = synthetic_cad_clouds(b, n, seed=31)
    start = torch.randint(n, (b,), generator=torch.Generator().manual_seed(32))
    want_pts, idx = U.fps_indices(pc.cuda(), m, start.cuda())
    sel = idx.cpu().long()
    x, y = pc.clone().cuda().requires_grad_(), nrm.clone().cuda().requires_grad_()
    pts, nm = U.farthest_points_normal_sample(x, y, m, start.cuda())
    assert torch.equal(_bits(pts), _bits(want_pts))                                   # the sampler's own points
    assert torch.equal(_bits(nm), _bits(torch.gather(nrm, 2, sel.unsqueeze(1).expand(b, 3, m))))   # the same columns
    (pts.sum() + 2.0 * nm.sum()).backward()
    ones = torch.zeros(b, n).scatter_add_(1, sel, torch.ones(b, m)).unsqueeze(1).expand(b, 3, n)
    assert torch.equal(x.grad.cpu(), ones) and torch.equal(y.grad.cpu(), 2.0 * ones)
    # ... and the dataset's form: the same selection, the points normalised, the normals as they were
    npts, nnm = U.farthest_points_normalized(pc.cuda(), nrm.cuda(), m, start.cuda())
    assert torch.equal(_bits(nnm), _bits(nm)) and not npts.requires_grad
    assert torch.equal(_bits(npts), _bits(U.normalize_cloud(want_pts)))
    o = npts.cpu().double()
    assert (o.norm(dim=1).max(dim=1)[0] - 1.0).abs().max() <= 2 * U32


# ------------------------------------------------------------------ dataset and command line, end to end
def _bare_mat(path, M, N, seed):
    """A synthetic file in the reference schema with the `normal` array left out."""
    from geoa3_amd.data import TEN_LABEL_INDEXES, synthetic_clouds
    data, normal = synthetic_clouds(M, N, seed=seed)
    labels = np.asarray([TEN_LABEL_INDEXES[i % 10] for i in range(M)], dtype=np.int64).reshape(-1, 1)
    os.makedirs(os.path.dirname(str(path)), exist_ok=True)
    savemat(str(path), {"data": data.numpy(), "label": labels})
    return data, normal


def test_dataset_estimates_then_resamples(tmp_path):
    from geoa3_amd import utility as U
    from geoa3_amd.data import ModelNet40
    data, _ = _bare_mat(tmp_path / "Data" / "bare.mat", 16, 96, seed=41)
    np.random.seed(5)
    ds = ModelNet40(data_mat_file=str(tmp_path / "Data" / "bare.mat"), attack_label="Untarget", resample_num=64,
                    estimate_normal_knn=8, estimate_normal_orient="outward")
    assert ds.data.shape == (16, 3, 64) and ds.normal.shape == (16, 3, 64) and not ds.data.is_cuda
    np.random.seed(5)
    first = torch.as_tensor([np.random.randint(96) for _ in range(16)])               # the reference's draws, in file order
    full = U.estimate_normal(data.cuda(), 8, "outward")                               # on the full cloud first ...
    pts, nrm = U.farthest_points_normalized(data.cuda(), full, 64, first.cuda())      # ... gathered afterwards
    assert torch.equal(ds.data, pts.cpu()) and torch.equal(ds.normal, nrm.cpu())
    item = ds[3]
    assert item[0].shape == (1, 64, 3) and item[1].shape == (1, 64, 3)


def test_resample_data_mat_writes_the_three_arrays(tmp_path):
    """Provider/resample_data_mat.py on an 8-instance file of 96-point clouds without normals -> 32 points."""
    import importlib.util
    from geoa3_amd import utility as U
    spec = importlib.util.spec_from_file_location(
        "resample_data_mat", os.path.join(os.path.dirname(__file__), "..", "Provider", "resample_data_mat.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    data, _ = _bare_mat(tmp_path / "in" / "bare.mat", 8, 96, seed=47)
    out = tool.main(tool.build_parser().parse_args(["--data_mat_file", str(tmp_path / "in" / "bare.mat"), "--out_file",
                                                    str(tmp_path / "out" / "small.mat"), "--resample_num", "32",
                                                    "--estimate_normal_knn", "8", "--seed", "3"]))
    mat = loadmat(out)
    assert sorted(k for k in mat if not k.startswith("__")) == ["data", "label", "normal"]
    assert mat["data"].shape == (8, 3, 32) and mat["normal"].shape == (8, 3, 32) and mat["data"].dtype == np.float32
    assert np.array_equal(mat["label"], loadmat(str(tmp_path / "in" / "bare.mat"))["label"])
    np.random.seed(3)
    first = torch.as_tensor([np.random.randint(96) for _ in range(8)])
    pts, nrm = U.farthest_points_normalized(data.cuda(), U.estimate_normal(data.cuda(), 8), 32, first.cuda())
    assert np.array_equal(mat["data"], pts.cpu().numpy()) and np.array_equal(mat["normal"], nrm.cpu().numpy())
    with pytest.raises(Exception, match="estimate_normal_knn"):      # without the flag the file is refused by name
        tool.main(tool.build_parser().parse_args(["--data_mat_file", str(tmp_path / "in" / "bare.mat"), "--out_file",
                                                  str(tmp_path / "out" / "x.mat"), "--resample_num", "32"]))


def test_command_line_on_a_file_without_normals(tmp_path, monkeypatch):
    """main_attack.py has no batch limit, so the file holds 16 instances (two batches of 8): estimated normals,
    re-sampling to the victim's 64 points, the attack loop, the files it writes and where it writes them."""
    import main_attack
    from geoa3_amd.attack import attack
    monkeypatch.chdir(tmp_path)
    path = tmp_path / "Data" / "bare96.mat"
    _bare_mat(path, 16, 96, seed=43)
    args = ["--attack", "GeoA3", "--attack_label", "Untarget", "-b", "8", "--npoint", "64", "--synthetic",
            "--data_dir_file", str(path), "--resample_num", "64", "--estimate_normal_knn", "8", "--binary_max_steps", "1",
            "--iter_max_steps", "8", "--is_record_loss", "--quiet"]
    cfg = main_attack.build_parser().parse_args(args)
    saved_dir = main_attack.main(cfg)
    assert saved_dir.endswith("_CurLoss1.0_k16_Resample64_EstNormal_k8")
    cfg_out = main_attack.build_parser().parse_args(args + ["--estimate_normal_orient", "outward"])
    assert main_attack.saved_dir_name(cfg_out).endswith("_Resample64_EstNormal_k8_outward")
    loss = loadmat(os.path.join(saved_dir, "Records", "loss_iter.mat"))["loss"]
    assert loss.shape == (8, 16) and np.isfinite(loss).all()
    assert open(os.path.join(saved_dir, "attack_result.txt")).read().startswith("attack success: ")
    for f in os.listdir(os.path.join(saved_dir, "Mat")):
        assert loadmat(os.path.join(saved_dir, "Mat", f))["adversary_point_clouds"].shape == (3, 64)
    # the first batch through attack() itself: the shape of what it returns
    from geoa3_amd.data import ModelNet40, synthetic_state_dict
    from geoa3_amd.pointnet import PointNet
    np.random.seed(0)
    ds = ModelNet40(data_mat_file=str(path), attack_label="Untarget", resample_num=64, estimate_normal_knn=8)
    batch = next(iter(torch.utils.data.DataLoader(ds, batch_size=8, shuffle=False)))
    net = PointNet(40, npoint=64)
    net.load_state_dict(synthetic_state_dict(40, seed=0, device=torch.device("cuda")))
    best, _, success, best_step, all_loss = attack(net.cuda().eval(), batch, cfg, 0, 2, verbose=False)
    assert best.shape == (8, 3, 64) and torch.isfinite(best).all()
    assert np.isfinite(np.asarray(all_loss)).all() and np.asarray(all_loss).shape == (8, 8)


# ------------------------------------------------------------------ the property the design rests on
def test_attack_does_not_read_the_sign_of_a_normal():
    """abs(<v, n>) in the curvature terms, (o.n) n in the projection: a run on the file's normals and a run on the same
    normals under random per-point sign flips must agree bit for bit (b = 4, n = 64, k = 8, 2 x 8 steps,
    --is_pro_grad)."""
    import main_attack
    from geoa3_amd.attack import attack
    from geoa3_amd.data import synthetic_clouds, synthetic_state_dict
    from geoa3_amd.pointnet import PointNet
    cfg = main_attack.build_parser().parse_args(["--attack", "GeoA3", "--attack_label", "Untarget", "--npoint", "64",
                                                 "--curv_loss_knn", "8", "--binary_max_steps", "2", "--iter_max_steps", "8",
                                                 "--is_pro_grad"])
    net = PointNet(40, npoint=64)
    net.load_state_dict(synthetic_state_dict(40, seed=0, device=torch.device("cuda")))
    net = net.cuda().eval()
    ori, nrm = synthetic_clouds(4, 64, seed=51)
    with torch.no_grad():
        gt = net(ori.cuda()).argmax(1).cpu()
    g = torch.Generator().manual_seed(52)
    flip = (torch.randint(2, (4, 1, 64), generator=g) * 2 - 1).float()
    assert (flip < 0).any() and (flip > 0).any()
    inits = [torch.randn(4, 3, 64, generator=g).cuda() * 1e-3 for _ in range(2)]

    def run(normal):
        data = [ori.permute(0, 2, 1).unsqueeze(1).contiguous(), normal.permute(0, 2, 1).unsqueeze(1).contiguous(),
                gt.view(4, 1)]
        best, _, success, best_step, all_loss = attack(net, data, cfg, 0, 1, init_offsets=inits, verbose=False)
        return best.cpu(), torch.as_tensor(np.asarray(all_loss, dtype=np.float64)), list(success), list(best_step)

    a, b = run(nrm), run(nrm * flip)
    assert torch.isfinite(a[1]).all() and a[1].shape == (8, 4)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1])
    assert a[2] == b[2] and a[3] == b[3]
