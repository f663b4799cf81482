"""The neighbour-based regularisers on the GPU (csrc/geom_reg.hip: kNN_smoothing_loss / repulsion_loss / displacement_loss,
and corresponding_normal_loss as geoa3_kappa + the dkappa path) through geoa3_amd.loss_utils, the geoa3:: ops and
geoa3_amd.ops, and --is_use_knn_smoothing_loss in the attack loop.

Bar (values and gradients): |GPU - float64| <= 4 * max(e_ref, eps32 * max|float64|), where e_ref is the reference's own
float32-vs-float64 error stored in tests/golden/geoa3_golden_reg.npz (at B = 250: of the float32 restatement of
tests/_reg_ref.py).  4x because the summation order differs from torch's.  The observed ratios are printed."""
import os

import numpy as np
import pytest
import torch

from oracle import geoa3_oracle as O
from tests import _reg_ref as R
from tests.test_reg_ref import NAMES, load_case

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
T = torch.from_numpy
EPS32 = float(np.finfo(np.float32).eps)
CASES = [(f, t) for f, tags in (("kNN_smoothing_loss", ["n64", "n200", "n256", "n1024", "dup256"]),
                                ("repulsion_loss", ["n64", "n200", "n256", "n1024", "dup256"]),
                                ("displacement_loss", ["n64", "n200", "n256", "n1024"]),
                                ("corresponding_normal_loss", ["n64", "n200", "n256", "n1024"])) for t in tags]
DEFAULT_K = {"repulsion_loss": 4, "displacement_loss": 16, "corresponding_normal_loss": 2}


@pytest.fixture(scope="module")
def gr():
    return np.load(os.path.join(REPO, "tests", "golden", "geoa3_golden_reg.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def net():
    from geoa3_amd.pointnet import PointNet
    n = PointNet(40)
    n.load_state_dict(O.make_pointnet_state_dict(40, seed=0))
    return n.cuda().eval()


def test_cases_are_the_fixtures(gr):
    assert CASES == [(f, str(t)) for f in NAMES for t in gr["%s/cases" % f]]


def _within(got, ref64, e_ref, what):
    """the bar of the module docstring; prints error / bound"""
    ref64 = ref64.double()
    bound = 4 * max(float(e_ref), EPS32 * float(ref64.abs().max()))
    err = float((got.detach().cpu().double() - ref64).abs().max())
    print("%-60s err %.3e  bound %.3e  ratio %.3f" % (what, err, bound, err / bound))
    assert err <= bound, (what, err, bound)


def _routes(fname, x, rest, kw, g):
    """(value, gradient) through loss_utils, through the op and through ops"""
    from geoa3_amd import loss_utils as L, ops
    out = {}
    xa = x.clone().requires_grad_()
    v = getattr(L, fname)(xa, *rest, **kw)
    out["loss_utils"] = (v.detach(), torch.autograd.grad(v, xa, g)[0])
    k = kw.get("k", DEFAULT_K.get(fname))
    if fname == "kNN_smoothing_loss":
        coef = kw.get("threshold_coef", 1.05)
        v, _, d, i = torch.ops.geoa3.knn_smoothing_loss(x, k, coef)
        out["op"] = (v, torch.ops.geoa3.knn_smoothing_loss_grad(x, d, i, g, k, coef))
        out["ops"] = (ops.knn_smoothing_loss(x, k, coef), ops.knn_smoothing_loss_grad(x, k, coef, g=g))
    elif fname == "repulsion_loss":
        h = kw.get("h", 0.03)
        v, d, i = torch.ops.geoa3.repulsion_loss(x, k, h)
        out["op"] = (v, torch.ops.geoa3.repulsion_loss_grad(x, d, i, g, k, h))
        out["ops"] = (ops.repulsion_loss(x, k, h), ops.repulsion_loss_grad(x, k, h, g=g))
    elif fname == "displacement_loss":
        v, d, i = torch.ops.geoa3.displacement_loss(x, rest[0], k)
        out["op"] = (v, torch.ops.geoa3.displacement_loss_grad(x, rest[0], d, i, g, k))
        out["ops"] = (ops.displacement_loss(x, rest[0], k), ops.displacement_loss_grad(x, rest[0], k, g=g))
    else:
        v, i = torch.ops.geoa3.corresponding_normal_loss(x, rest[0], k)
        out["op"] = (v, torch.ops.geoa3.corresponding_normal_loss_grad(x, rest[0], i, g))
        v2, i2 = ops.corresponding_normal_loss(x, rest[0], k, want_knn=True)
        out["ops"] = (v2, ops.corresponding_normal_loss_grad(x, rest[0], i2, g))
    return out


@pytest.mark.parametrize("fname,tag", CASES)
def test_matches_reference(gr, fname, tag):
    x, rest, kw, pre = load_case(gr, fname, tag, torch.float32)
    x, rest, g = x.cuda(), tuple(r.cuda() for r in rest), T(gr[pre + "g"]).cuda()
    v64, g64 = T(gr[pre + "value64"]), T(gr[pre + "grad64"])
    for route, (val, grad) in _routes(fname, x, rest, kw, g).items():
        assert val.shape == v64.shape and val.dtype == torch.float32 and grad.shape == x.shape
        _within(val, v64, gr[pre + "e_ref_value"], "%s/%s %s value" % (fname, tag, route))
        _within(grad, g64, gr[pre + "e_ref_grad"], "%s/%s %s grad" % (fname, tag, route))


@pytest.mark.parametrize("fname,tag", CASES)
def test_indices_and_mask_exact(gr, fname, tag):
    x, rest, kw, pre = load_case(gr, fname, tag, torch.float32)
    k = kw.get("k", DEFAULT_K.get(fname))
    if fname == "kNN_smoothing_loss":
        _, cond, _, idx = torch.ops.geoa3.knn_smoothing_loss(x.cuda(), k, kw.get("threshold_coef", 1.05))
        assert np.array_equal(cond.cpu().numpy(), gr[pre + "cond"])
    elif fname == "repulsion_loss":
        idx = torch.ops.geoa3.repulsion_loss(x.cuda(), k, kw.get("h", 0.03))[2]
    elif fname == "displacement_loss":
        idx = torch.ops.geoa3.displacement_loss(x.cuda(), rest[0].cuda(), k)[2]
    else:
        idx = torch.ops.geoa3.corresponding_normal_loss(x.cuda(), rest[0].cuda(), k)[1]
    assert np.array_equal(idx[:, :, 1:].cpu().numpy(), gr[pre + "knn_idx"].astype(np.int32))


def _clouds250(kind):
    from geoa3_amd.data import synthetic_cad_clouds, synthetic_clouds
    ori, _ = (synthetic_clouds if kind == "ellipsoid" else synthetic_cad_clouds)(250, 1024, seed=3)
    return (ori + torch.randn(ori.shape, generator=torch.Generator().manual_seed(7)) * 0.01).contiguous()


@pytest.mark.parametrize("kind", ["ellipsoid", "cad"])
def test_knn_smoothing_b250_matches_restatement(kind):
    """B = 250, N = 1024, k = 5, coef 1.10 against the float64 restatement.  An instance is left out of the mask and value
    comparison only if the float64 restatement has a point within 1e-5 thr of the threshold; at most 5 % may be."""
    from geoa3_amd import ops
    k, coef = 5, 1.10
    x = _clouds250(kind)
    xc = x.cuda()
    loss, cond = ops.knn_smoothing_loss(xc, k, coef, want_cond=True)
    grad = ops.knn_smoothing_loss_grad(xc, k, coef)
    v64, v32, c64, g64, g32, near = [], [], [], [], [], []
    for s in range(0, 250, 10):
        xs = x[s:s + 10]
        sv, thr, c = R.smoothing_parts(xs.double(), k, coef, stable=False)
        near.append(((sv - thr.unsqueeze(1)).abs() <= 1e-5 * thr.unsqueeze(1)).any(1))
        c64.append(c)
        ones = torch.ones(xs.shape[0])
        a, b = R.value_and_grad(R.kNN_smoothing_loss, xs.double(), ones, k, coef, stable=False)
        v64.append(a)
        g64.append(b)
        a, b = R.value_and_grad(R.kNN_smoothing_loss, xs, ones, k, coef, stable=False)
        v32.append(a)
        g32.append(b)
    v64, v32, c64, g64, g32, near = (torch.cat(t) for t in (v64, v32, c64, g64, g32, near))
    keep = ~near
    print("%s: %d of 250 instances within 1e-5 thr of the threshold" % (kind, int(near.sum())))
    assert int(near.sum()) <= 12
    assert torch.equal(cond.cpu().bool()[keep], c64[keep])
    _within(loss.cpu()[keep], v64[keep], float((v32.double() - v64)[keep].abs().max()), "%s b250 value" % kind)
    if kind == "ellipsoid":   # (the CAD clouds repeat points: which of two equal neighbours receives a pull is the tie rule's)
        _within(grad.cpu()[keep], g64[keep], float((g32.double() - g64)[keep].abs().max()), "%s b250 grad" % kind)


def _all_functions(x, ori, nrm, with_normal=True):
    from geoa3_amd import ops
    res = []
    res += [ops.knn_smoothing_loss(x, 5, 1.1), ops.knn_smoothing_loss_grad(x, 5, 1.1)]
    res += [ops.repulsion_loss(x), ops.repulsion_loss_grad(x)]
    res += [ops.displacement_loss(x, ori), ops.displacement_loss_grad(x, ori)]
    if with_normal:
        v, i = ops.corresponding_normal_loss(x, nrm, 2, want_knn=True)
        res += [v, ops.corresponding_normal_loss_grad(x, nrm, i)]
    return res


@pytest.mark.parametrize("N", [256, 1500, 5000])
def test_row_independence_and_repeats(N):
    """Row r of a batch == the same cloud alone, bit for bit; repeated calls are bit identical.  N = 5000: the form with
    the gradient sums in the workspace."""
    ori, nrm = O.make_synthetic_clouds(5, N, seed=33)
    x = (ori + torch.randn(ori.shape, generator=torch.Generator().manual_seed(34)) * 0.01).cuda().contiguous()
    ori, nrm = ori.cuda(), nrm.cuda()
    wn = N <= 4096   # (corresponding_normal_loss's gradient is geoa3_geo_loss_grad's: its own size range)
    full, again = _all_functions(x, ori, nrm, wn), _all_functions(x, ori, nrm, wn)
    one = _all_functions(x[3:4].contiguous(), ori[3:4].contiguous(), nrm[3:4].contiguous(), wn)
    for a, b, c in zip(full, again, one):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)
        assert torch.equal(a[3:4], c)
    # the gradient of the large form against the float64 restatement (one instance)
    if N > 4096:
        g64 = R.value_and_grad(R.repulsion_loss, x[3:4].cpu().double(), torch.ones(1, N), stable=False)[1]
        g32 = R.value_and_grad(R.repulsion_loss, x[3:4].cpu(), torch.ones(1, N), stable=False)[1]
        _within(full[3][3:4], g64, float((g32.double() - g64).abs().max()), "repulsion grad N=%d" % N)


def test_table_argument_and_wider_table():
    """A caller's table (also a wider one: the first k + 1 columns serve) gives the bits of the entry point's own search."""
    from geoa3_amd import ops
    ori, _ = O.make_synthetic_clouds(3, 300, seed=35)
    x = (ori + 0.01 * torch.randn(ori.shape, generator=torch.Generator().manual_seed(36))).cuda().contiguous()
    wide = ops.knn_self_planar(x, 17)
    ws = ops.reg_workspace(3, 300, 5, x.device)
    out = torch.empty(3, device=x.device)
    assert torch.equal(ops.knn_smoothing_loss(x, 5, 1.1), ops.knn_smoothing_loss(x, 5, 1.1, knn=wide, workspace=ws, out=out))
    assert torch.equal(ops.knn_smoothing_loss_grad(x, 5, 1.1), ops.knn_smoothing_loss_grad(x, 5, 1.1, knn=wide))
    assert torch.equal(ops.repulsion_loss_grad(x, 4), ops.repulsion_loss_grad(x, 4, knn=wide))
    ow = ops.knn_self_planar(ori.cuda().contiguous(), 17)
    assert torch.equal(ops.displacement_loss_grad(x, ori.cuda(), 16), ops.displacement_loss_grad(x, ori.cuda(), 16, knn=ow))


def test_nan_input_is_loud():
    ori, nrm = O.make_synthetic_clouds(2, 256, seed=37)
    x = (ori + 0.01 * torch.randn(ori.shape, generator=torch.Generator().manual_seed(38))).contiguous()
    x[1, 0, 5] = float("nan")
    for t in _all_functions(x.cuda(), ori.cuda(), nrm.cuda()):
        assert torch.isfinite(t[0]).all() and torch.isnan(t[1]).all()
    x[1, 0, 5] = float("inf")
    for t in _all_functions(x.cuda(), ori.cuda(), nrm.cuda()):
        assert torch.isfinite(t[0]).all() and torch.isnan(t[1]).all()


def test_out_of_range_sizes_raise():
    from geoa3_amd import loss_utils as L, ops
    from geoa3_amd._lib import Geoa3Error
    x = torch.rand(1, 3, 40, device="cuda")
    big = torch.rand(1, 3, 8200, device="cuda")
    for fn in (lambda c, k: L.kNN_smoothing_loss(c, k), lambda c, k: L.repulsion_loss(c, k),
               lambda c, k: L.displacement_loss(c, c, k), lambda c, k: L.corresponding_normal_loss(c, c, k),
               lambda c, k: ops.knn_smoothing_loss_grad(c, k), lambda c, k: ops.repulsion_loss_grad(c, k),
               lambda c, k: ops.displacement_loss_grad(c, c, k)):
        for cloud, k in ((x, 0), (x, 40), (x, 64), (big, 4)):
            with pytest.raises(Geoa3Error):
                fn(cloud, k)
    with pytest.raises(Geoa3Error):
        ops.repulsion_loss(x, 4, h=0.0)


def test_compile_fullgraph():
    from geoa3_amd import loss_utils as L
    ori, _ = O.make_synthetic_clouds(2, 256, seed=39)
    ori = ori.cuda()
    x = (ori + 0.01 * torch.randn(ori.shape, device="cuda")).contiguous()

    def f(adv, o):
        return L.chamfer_loss(adv, o) + 0.5 * L.kNN_smoothing_loss(adv, 5, 1.1) + L.repulsion_loss(adv).mean(1)

    xa = x.clone().requires_grad_()
    eager = f(xa, ori)
    (ge,) = torch.autograd.grad(eager.sum(), xa)
    xb = x.clone().requires_grad_()
    comp = torch.compile(f, fullgraph=True)(xb, ori)
    (gc,) = torch.autograd.grad(comp.sum(), xb)
    assert torch.allclose(eager, comp, rtol=1e-5, atol=0) and torch.allclose(ge, gc, rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------ the loop
def _inputs(b=3, n=256, seed=41):
    ori, nrm = O.make_synthetic_clouds(b, n, seed=seed)
    gt = torch.zeros(b, dtype=torch.int64)
    inits = [torch.randn(b, 3, n, generator=torch.Generator().manual_seed(seed + 1)) * 1e-3]
    return ori, nrm, gt, inits


def test_loop_opt_in_off_is_bit_identical(net):
    from tests.test_gpu_attack import _run
    ori, nrm, gt, inits = _inputs()
    kw = dict(binary_max_steps=1, iter_max_steps=4, curv_loss_knn=4)
    a = _run(net, O.AttackCfg(**kw), ori, nrm, gt, None, False, inits)
    b = _run(net, O.AttackCfg(knn_smoothing_loss_weight=5.0, knn_smoothing_k=5, knn_threshold_coef=1.10,
                              is_use_knn_smoothing_loss=False, **kw), ori, nrm, gt, None, False, inits)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    for name in ("offset", "m", "v", "x", "loss_hist", "best_attack", "best_loss"):
        assert torch.equal(a[0].t[name], b[0].t[name]), name
    assert "ks_loss" not in b[0].t and "ks_knn" not in b[0].t


def test_loop_term_alone(net):
    """Only this term (no distance / curvature term, no classification loss): constrain = w S(ori), and the first Adam step
    is the one torch computes from g = (c / b) w dS/dx."""
    from tests.test_gpu_attack import _run
    from geoa3_amd import ops
    w, k, coef, lr, c0 = 3.0, 5, 1.10, 0.002, 10.0
    cfg = O.AttackCfg(is_use_knn_smoothing_loss=True, knn_smoothing_loss_weight=w, knn_smoothing_k=k,
                      knn_threshold_coef=coef, dis_loss_type="None", hd_loss_weight=0.0, curv_loss_weight=0.0,
                      cls_loss_type="None", binary_max_steps=1, iter_max_steps=2, lr=lr, initial_const=c0)
    ori, nrm, gt, _ = _inputs()
    b = ori.shape[0]
    r, _, xs, _ = _run(net, cfg, ori, nrm, gt, None, False, [torch.zeros_like(ori)])
    oc = ori.cuda()
    S, dS = ops.knn_smoothing_loss(oc, k, coef), ops.knn_smoothing_loss_grad(oc, k, coef)
    hist = r.t["loss_hist"].cpu().numpy()
    np.testing.assert_allclose(hist[0], (c0 * w * S).cpu().numpy(), rtol=1e-6)      # loss_n = c * constrain (cls 0)
    off = torch.zeros_like(oc).requires_grad_()
    opt = torch.optim.Adam([off], lr=lr)
    off.grad = (c0 / b) * w * dS
    opt.step()
    step = xs[1] - xs[0]
    moved = dS.abs().cpu().numpy() > 1e-3 * float(dS.abs().max())
    assert moved.any()
    np.testing.assert_allclose(step[moved], off.detach().cpu().numpy()[moved], rtol=1e-4, atol=1e-7)
    assert (step[~(dS != 0).cpu().numpy()] == 0).all()


def test_loop_shared_table_is_bit_identical(net):
    from tests.test_gpu_attack import _run
    ori, nrm, gt, inits = _inputs()
    kw = dict(binary_max_steps=1, iter_max_steps=5, curv_loss_knn=8, is_use_knn_smoothing_loss=True,
              knn_smoothing_loss_weight=5.0, knn_smoothing_k=5, knn_threshold_coef=1.10)
    a = _run(net, O.AttackCfg(**kw), ori, nrm, gt, None, False, inits)
    b = _run(net, O.AttackCfg(knn_smoothing_share_table=False, **kw), ori, nrm, gt, None, False, inits)
    assert a[0].knn_share and not b[0].knn_share and "ks_knn" in b[0].t and "ks_knn" not in a[0].t
    assert np.array_equal(a[2], b[2])
    assert torch.equal(a[0].t["loss_hist"], b[0].t["loss_hist"]) and torch.equal(a[0].t["ks_loss"], b[0].t["ks_loss"])
    off = _run(net, O.AttackCfg(binary_max_steps=1, iter_max_steps=5, curv_loss_knn=8), ori, nrm, gt, None, False, inits)
    assert not np.array_equal(a[2], off[2])           # the term moves the iterates


def test_loop_sharded_rows_equal_full_batch(net):
    """The term is per row: the rows of a 2-shard split (global_batch = the full b) equal the full batch's, bit for bit."""
    from tests.test_gpu_attack import _run
    ori, nrm, gt, inits = _inputs(b=4)
    cfg = lambda: O.AttackCfg(binary_max_steps=1, iter_max_steps=4, curv_loss_knn=4, is_use_knn_smoothing_loss=True,
                              knn_smoothing_loss_weight=5.0, knn_smoothing_k=5, knn_threshold_coef=1.10, late_join=False)
    full = _run(net, cfg(), ori, nrm, gt, None, False, inits)
    # (the binary search reads the LAST instance's label: with one binary step it does not reach the iterates)
    for lo, hi in ((0, 2), (2, 4)):
        part = _run(net, cfg(), ori[lo:hi], nrm[lo:hi], gt[lo:hi], None, False, [inits[0][lo:hi]], global_batch=4)
        assert np.array_equal(part[2], full[2][:, lo:hi])
        assert torch.equal(part[0].t["loss_hist"], full[0].t["loss_hist"][:, lo:hi])


def test_info_line_reports_the_term(net):
    from tests.test_gpu_attack import _run
    ori, nrm, gt, inits = _inputs()
    r = _run(net, O.AttackCfg(binary_max_steps=1, iter_max_steps=2, curv_loss_knn=4, is_use_knn_smoothing_loss=True,
                              knn_smoothing_loss_weight=5.0, knn_smoothing_k=5, knn_threshold_coef=1.10), ori, nrm, gt,
             None, False, inits)[0]
    assert "knn_smooth" in r.info_line(0, 1, 0, 1)


def test_cli_runs_with_flag(tmp_path, monkeypatch):
    import glob
    import main_attack
    monkeypatch.chdir(tmp_path)
    args = ["--attack", "GeoA3", "--attack_label", "Untarget", "-b", "125", "--npoint", "256", "--synthetic",
            "--data_dir_file", str(tmp_path / "Data" / "syn256.mat"), "--binary_max_steps", "2", "--iter_max_steps",
            "6", "--lr", "0.005", "--curv_loss_knn", "8", "--is_use_knn_smoothing_loss", "--quiet"]
    saved_dir = main_attack.main(main_attack.build_parser().parse_args(args))
    assert saved_dir.endswith("_k8_kNNSmooth5.0_k5_coef1.1")
    rate = float(open(os.path.join(saved_dir, "attack_result.txt")).read().split(":")[1])
    mats = sorted(glob.glob(os.path.join(saved_dir, "Mat", "adv_*.mat")))
    assert len(mats) == round(rate * 250 / 100.0) and len(mats) > 0
