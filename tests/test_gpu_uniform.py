"""The uniformity term on the GPU (geoa3_uniform_loss / geoa3::uniform_loss / geoa3_amd.loss_utils.uniform_loss and
--uniform_loss_weight in the attack loop) against the reference's own values (tests/golden/geoa3_golden_uniform.npz),
the float64 restatement of tests/_uniform_ref.py and the existing sampler / ball-query entry points.

Bars: value rtol 1e-5 (the reference sums its rows in float32, the kernel in double); gradient within
1e-4 * max|g| (float32 pair terms summed in 2^-32 fixed point against the reference's float32 scatter-adds)."""
import os
import numpy as np
import pytest
import torch

from oracle import geoa3_oracle as O
from tests import _uniform_ref as R
from tests.test_oracle_golden import _traj_close

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = ["n188", "n256", "n1024", "n2048", "dupzero", "custom", "bn3"]
T = torch.from_numpy


@pytest.fixture(scope="module")
def gu():
    return np.load(os.path.join(REPO, "tests", "golden", "geoa3_golden_uniform.npz"), allow_pickle=False)


def _case(gu, tag):
    pre = "uni/%s/" % tag
    return (pre, T(gu[pre + "x"]), [float(p) for p in gu[pre + "percentages"]], float(gu[pre + "radius"]),
            int(gu[pre + "k"]))


@pytest.mark.parametrize("tag", CASES)
def test_op_matches_reference(gu, tag):
    from geoa3_amd import loss_utils as L
    pre, x, pcts, radius, k = _case(gu, tag)
    xg = x.cuda().requires_grad_()
    loss = L.uniform_loss(xg, pcts, radius, k)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (g,) = torch.autograd.grad(loss, xg)
    np.testing.assert_allclose(float(loss.detach()), float(gu[pre + "loss"]), rtol=1e-5)
    ref_g = gu[pre + "grad"]
    assert np.abs(g.cpu().numpy() - ref_g).max() <= 1e-4 * np.abs(ref_g).max()


@pytest.mark.parametrize("tag", CASES)
def test_indices_equal_entry_points(gu, tag):
    from geoa3_amd import ops
    from geoa3_amd.pointnet2 import ext
    pre, x, pcts, radius, k = _case(gu, tag)
    planar = (x.permute(0, 2, 1) if tag == "bn3" else x).contiguous().cuda()
    _, _, fps, rows = ops.uniform_loss(planar, pcts, radius, k, want_idx=True)
    pm = planar.permute(0, 2, 1).contiguous()
    N = pm.shape[1]
    fps_ep = ext.furthest_point_sampling(pm, int(N * 0.05))
    assert torch.equal(fps.cpu(), fps_ep.cpu().int())
    assert np.array_equal(fps.cpu().numpy(), gu[pre + "fps"])
    centres = torch.gather(pm, 1, fps.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    for i, p in enumerate(pcts):
        bq = ext.ball_query(centres, pm, float(np.sqrt(p * 4 * radius)), int(N * (p * 4)))
        assert torch.equal(rows[i].cpu(), bq.cpu().int()), i
        assert np.array_equal(rows[i].cpu().numpy(), gu[pre + "bq%d" % i]), i


@pytest.mark.parametrize("N", [1024, 4096])
def test_op_matches_restatement_b250(N):
    from geoa3_amd import ops
    ori, _ = O.make_synthetic_clouds(250, N, seed=90 + N)
    x = (ori + torch.randn(ori.shape, generator=torch.Generator().manual_seed(N)) * 0.01).contiguous()
    xc = x.cuda()
    loss, g, fps, rows = ops.uniform_loss(xc, want_idx=True)
    ref_loss, ref_g = R.uniform_ref(xc, idx=(fps.long(), [r.long() for r in rows]))
    np.testing.assert_allclose(float(loss), float(ref_loss), rtol=1e-5)
    ref_g = ref_g.float()
    assert float((g - ref_g).abs().max()) <= 1e-4 * float(ref_g.abs().max())
    # the indices of a few instances against the CPU oracle
    f2, r2 = R.indices(x[:3])
    assert torch.equal(fps[:3].cpu().long(), f2)
    for a, b in zip(rows, r2):
        assert torch.equal(a[:3].cpu().long(), b)


def test_repeat_calls_bit_identical():
    from geoa3_amd import ops
    ori, _ = O.make_synthetic_clouds(16, 1024, seed=5)
    x = ori.cuda()
    l1, g1 = ops.uniform_loss(x)
    l2, g2 = ops.uniform_loss(x)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    big, _ = O.make_synthetic_clouds(2, 8192, seed=6)    # gradient sums in the workspace
    l3, g3 = ops.uniform_loss(big.cuda())
    l4, g4 = ops.uniform_loss(big.cuda())
    assert torch.equal(l3, l4) and torch.equal(g3, g4) and torch.isfinite(l3)


def test_compile_fullgraph_with_chamfer():
    from geoa3_amd import loss_utils as L
    ori, _ = O.make_synthetic_clouds(4, 512, seed=8)
    ori = ori.cuda()
    adv = (ori + 0.01 * torch.randn_like(ori)).requires_grad_()

    def f(a, o):
        return L.chamfer_loss(a, o).mean() + 0.5 * L.uniform_loss(a)

    eager = f(adv, ori)
    (ge,) = torch.autograd.grad(eager, adv)
    comp = torch.compile(f, fullgraph=True)(adv, ori)
    (gc,) = torch.autograd.grad(comp, adv)
    assert torch.equal(eager, comp) and torch.equal(ge, gc)


def test_unsupported_sizes_raise():
    from geoa3_amd import _lib, ops
    x = torch.zeros(2, 3, 187, device="cuda")
    with pytest.raises(_lib.Geoa3Error, match="supported range"):
        ops.uniform_loss(x)                              # nsample = int(187 * 0.016) = 2 < k + 1
    with pytest.raises(_lib.Geoa3Error):
        ops.uniform_loss(torch.zeros(1, 3, 9000, device="cuda"))
    with pytest.raises(_lib.Geoa3Error):
        ops.uniform_loss(torch.zeros(1, 3, 1024, device="cuda"), k=9)
    with pytest.raises(_lib.Geoa3Error):
        ops.uniform_loss(torch.zeros(1, 3, 1024, device="cuda"), k=0)
    with pytest.raises(_lib.Geoa3Error):
        ops.uniform_loss(torch.zeros(1, 3, 1024, device="cuda"), percentages=[0.2])   # nsample 819 > 512


def test_nan_input_gives_nan_loss():
    from geoa3_amd import ops
    ori, _ = O.make_synthetic_clouds(3, 256, seed=9)
    x = ori.clone()
    x[1, 2, 17] = float("nan")
    loss, g = ops.uniform_loss(x.cuda())
    assert torch.isnan(loss)
    assert torch.isfinite(g[0]).all() and torch.isnan(g[1]).all()


@pytest.fixture(scope="module")
def net():
    from geoa3_amd.pointnet import PointNet
    n = PointNet(40)
    n.load_state_dict(O.make_pointnet_state_dict(40, seed=0))
    return n.cuda().eval()


UNI_ATK = {"untarget_ce": (dict(uniform_loss_weight=1.0, curv_loss_knn=4, binary_max_steps=2, iter_max_steps=5,
                                lr=0.002), False),
           "target_margin": (dict(uniform_loss_weight=0.5, attack_label="All", cls_loss_type="Margin", curv_loss_knn=4,
                                  binary_max_steps=2, iter_max_steps=5, lr=0.003, initial_const=0.5), True)}


@pytest.mark.parametrize("late", [False, True])
@pytest.mark.parametrize("tag", list(UNI_ATK))
def test_attack_matches_reference_trajectory(net, gu, tag, late):
    from tests.test_gpu_attack import _run
    kw, targeted = UNI_ATK[tag]
    cfg = O.AttackCfg(late_join=late, **kw)
    pre = "atk/%s/" % tag
    ori, nrm, gt, tgt = (T(gu[pre + n]) for n in ("ori", "nrm", "gt", "tgt"))
    inits = [T(a) for a in gu[pre + "inits"]]
    r, (best, target, succ, best_step, all_loss), xs, labels = _run(net, cfg, ori, nrm, gt, tgt, targeted, inits)
    loose = max(2e-3, 2.0 * cfg.lr * cfg.iter_max_steps)
    _traj_close(xs, gu[pre + "tr_x"], loose=loose)
    ref_logits = gu[pre + "tr_logits"]
    ref_labels = ref_logits.argmax(-1)
    top2 = np.sort(ref_logits, axis=-1)[..., -2:]
    near_tie = (top2[..., 1] - top2[..., 0]) < 3e-4
    assert (labels == ref_labels)[~near_tie].all()
    clean = ~((labels != ref_labels).any(axis=0))
    assert clean.mean() >= 0.5
    assert (np.asarray(succ) == gu[pre + "success"])[clean].all()
    assert (np.asarray(best_step) == gu[pre + "best_step"])[clean].all()
    np.testing.assert_allclose(np.asarray(all_loss, dtype=np.float32), gu[pre + "all_loss"], rtol=2e-3, atol=2e-4)


def test_attack_uniform_only_and_cls_none(net):
    """No other geometry term (constrain = w U) and cls_loss_type None (the term's gradient alone drives the update):
    one Adam step moves the cloud along -sign(dU/dx) -- checked against the op itself."""
    from tests.test_gpu_attack import _run
    from geoa3_amd import ops
    cfg = O.AttackCfg(uniform_loss_weight=2.0, dis_loss_type="None", hd_loss_weight=0.0, curv_loss_weight=0.0,
                      cls_loss_type="None", binary_max_steps=1, iter_max_steps=2, lr=0.002)
    ori, nrm = O.make_synthetic_clouds(3, 256, seed=70)
    gt = torch.zeros(3, dtype=torch.int64)
    inits = [torch.zeros(3, 3, 256)]
    r, _, xs, _ = _run(net, cfg, ori, nrm, gt, None, False, inits)
    u, g = ops.uniform_loss(ori.cuda())
    hist = np.asarray(r.t["loss_hist"].cpu())
    np.testing.assert_allclose(hist[0], 10.0 * 2.0 * float(u), rtol=1e-6)   # loss_n = c * w * U (cls 0)
    step = xs[1] - xs[0]
    sel = g.abs().cpu().numpy() > 1e-3 * float(g.abs().max())
    assert (np.sign(step[sel]) == -np.sign(g.cpu().numpy()[sel])).all()


def test_sharded_refusal(net):
    from geoa3_amd.attack import AttackRunner
    cfg = O.AttackCfg(uniform_loss_weight=1.0)
    with pytest.raises(ValueError, match="whole batch"):
        AttackRunner(net, 4, 256, cfg, torch.device("cuda"), global_batch=8)
    AttackRunner(net, 4, 256, cfg, torch.device("cuda"), global_batch=4)


def test_weight_zero_bit_identical(net):
    from tests.test_gpu_attack import _run
    ori, nrm = O.make_synthetic_clouds(3, 256, seed=71)
    gt = torch.zeros(3, dtype=torch.int64)
    inits = [torch.randn(3, 3, 256, generator=torch.Generator().manual_seed(1)) * 1e-3]
    a = _run(net, O.AttackCfg(binary_max_steps=1, iter_max_steps=4, curv_loss_knn=4), ori, nrm, gt, None, False, inits)
    b = _run(net, O.AttackCfg(binary_max_steps=1, iter_max_steps=4, curv_loss_knn=4, uniform_loss_weight=0.0), ori, nrm,
             gt, None, False, inits)
    assert np.array_equal(a[2], b[2])
    assert "uni_loss" not in a[0].t


def test_cli_runs_with_flag(tmp_path, monkeypatch):
    import glob
    import main_attack
    monkeypatch.chdir(tmp_path)
    args = ["--attack", "GeoA3", "--attack_label", "Untarget", "-b", "125", "--npoint", "256", "--synthetic",
            "--data_dir_file", str(tmp_path / "Data" / "syn256.mat"), "--binary_max_steps", "2", "--iter_max_steps",
            "6", "--lr", "0.005", "--curv_loss_knn", "8", "--uniform_loss_weight", "0.5", "--quiet"]
    saved_dir = main_attack.main(main_attack.build_parser().parse_args(args))
    assert saved_dir.endswith("_k8_UniLoss0.5")
    rate = float(open(os.path.join(saved_dir, "attack_result.txt")).read().split(":")[1])
    mats = sorted(glob.glob(os.path.join(saved_dir, "Mat", "adv_*.mat")))
    objs = sorted(glob.glob(os.path.join(saved_dir, "PC", "adv_*.obj")))
    assert len(mats) == len(objs) == round(rate * 250 / 100.0) and len(mats) > 0
