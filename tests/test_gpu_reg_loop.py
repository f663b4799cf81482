"""--displacement_loss_weight / --repulsion_loss_weight / --corr_normal_loss_weight in the device-resident attack loop, and
geoa3_reg_fold_points (csrc/geom_reg.hip) alone.

Reference: tests/_reg_ref.py in float64 on the float32 iterate ori + offset.  Inputs: O.make_synthetic_clouds(3, 256,
seed=41) with initial offsets randn * 1e-2 (seed 42): at a zero offset the displacement term and its gradient vanish.
Every comparison of a gradient first asserts, from the reference alone, that it exceeds 1e-3 of its maximum on at least
half of the points of every instance.

Weights (2^20, 16, 1) bring the three terms to the same order (0.1, -0.14, 0.17 at these inputs; the reference's figures),
and h = 2^-5 where a float32 `h` must equal the reference's."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import geoa3_oracle as O
from tests import _reg_ref as R

pytestmark = pytest.mark.gpu
U24 = 2.0 ** -24
W = {"disp": 2.0 ** 20, "rep": 16.0, "cn": 1.0}
FLAG = {"disp": "displacement_loss", "rep": "repulsion_loss", "cn": "corr_normal_loss"}
NEW_BUFFERS = ("disp_", "rep_", "cn_", "reg_")


@pytest.fixture(scope="module")
def net():
    from geoa3_amd.pointnet import PointNet
    n = PointNet(40)
    n.load_state_dict(O.make_pointnet_state_dict(40, seed=0))
    return n.cuda().eval()


def _inputs(b=3, n=256, seed=41):
    ori, nrm = O.make_synthetic_clouds(b, n, seed=seed)
    gt = torch.zeros(b, dtype=torch.int64)
    inits = [torch.randn(b, 3, n, generator=torch.Generator().manual_seed(seed + 1)) * 1e-2]
    return ori, nrm, gt, inits


_REF = {}


def _ref(term, n, k, h=0.03, b=3):
    """(mean_i term [b], d mean_i term / dx [b,3,n]) in float64 at x = fl32(ori + offset); computed once per case"""
    key = (term, n, k, h, b)
    if key not in _REF:
        ori, nrm, _, inits = _inputs(b, n)
        x = (ori + inits[0]).double()
        g = torch.full((b, n), 1.0 / n, dtype=torch.float64)
        if term == "disp":
            out, gx = R.value_and_grad(R.displacement_loss, x, g, ori.double(), k=k)
        elif term == "rep":
            out, gx = R.value_and_grad(R.repulsion_loss, x, g, k=k, h=h)
        else:
            out, gx = R.value_and_grad(R.corresponding_normal_loss, x, g, nrm.double(), k=k)
        a = gx.abs().amax(1)
        share = (a > 1e-3 * a.amax(1, keepdim=True)).double().mean(1)
        assert float(share.min()) >= 0.5, (key, share.tolist())      # the gradient is there to be compared
        _REF[key] = (out.mean(1), gx)
    return _REF[key]


def _term_kw(term, w, k=None, h=None):
    kw = {FLAG[term] + "_weight": w}
    if k is not None:
        kw[FLAG[term] + "_knn"] = k
    if h is not None:
        kw["repulsion_loss_h"] = h
    return kw


# ------------------------------------------------------------------------------------------------ 1. the fold alone
FOLD_N = [1, 2, 3, 511, 512, 513, 1025, 4097, 8192]


def _fold(out, grad, w, term=True, constrain=None, g=None):
    """-> (term, constrain, g) after one call; constrain / g given: the _add form on a copy of them"""
    from geoa3_amd import ops
    B, N = out.shape
    t = torch.full((B,), 7.0, device="cuda") if term else None
    c = constrain.clone() if constrain is not None else torch.full((B,), 7.0, device="cuda")
    gg = g.clone() if g is not None else torch.full((B, 3, N), 7.0, device="cuda")
    ops.reg_fold_points(out, grad, w, B, N, term=t, constrain=c, constrain_add=constrain is not None, g=gg,
                        g_add=g is not None)
    return t, c, gg


@pytest.mark.parametrize("N", FOLD_N)
def test_fold_points_alone(N):
    from geoa3_amd import ops
    B, w = 3, -1.75
    gen = torch.Generator().manual_seed(N)
    out, grad = torch.randn(B, N, generator=gen), torch.randn(B, 3, N, generator=gen)       # signed
    c0, g0 = torch.randn(B, generator=gen), torch.randn(B, 3, N, generator=gen)
    mean64 = out.double().mean(1)
    do, dg, dc0, dg0 = out.cuda(), grad.cuda(), c0.cuda(), g0.cuda()
    for add in (False, True):
        t, c, g = _fold(do, dg, w, constrain=dc0 if add else None, g=dg0 if add else None)
        t, c, g = t.cpu().double(), c.cpu().double(), g.cpu().double()
        e = (t - mean64).abs()
        print("N %5d add %d  term err / bound %.3f" % (N, add, float((e / (2 * U24 * out.double().abs().mean(1))).max())))
        assert (e <= 2 * U24 * out.double().abs().mean(1)).all()
        cref = (c0.double() if add else 0.0) + w * mean64
        cmag = (c0.double().abs() if add else 0.0) + (w * mean64).abs()
        assert ((c - cref).abs() <= 4 * U24 * cmag).all(), (N, add)
        gref = (g0.double() if add else 0.0) + (w / N) * grad.double()
        gmag = (g0.double().abs() if add else 0.0) + ((w / N) * grad.double()).abs()
        assert ((g - gref).abs() <= 4 * U24 * gmag).all(), (N, add)
    # the same bits from a second call, and from a row alone
    a, b2 = _fold(do, dg, w, constrain=dc0, g=dg0), _fold(do, dg, w, constrain=dc0, g=dg0)
    assert all(torch.equal(x, y) for x, y in zip(a, b2))
    for r in range(B):
        alone = _fold(do[r:r + 1].contiguous(), dg[r:r + 1].contiguous(), w, constrain=dc0[r:r + 1].contiguous(),
                      g=dg0[r:r + 1].contiguous())
        assert all(torch.equal(x[r:r + 1], y) for x, y in zip(a, alone)), r
    # a NaN row: NaN in its own outputs only
    on, gn = do.clone(), dg.clone()
    on[1, N // 2] = float("nan")
    gn[1, :, N // 2] = float("nan")
    bad = _fold(on, gn, w, constrain=dc0, g=dg0)
    for x, y in zip(bad, a):
        assert torch.isnan(x[1]).all() and torch.equal(x[0], y[0]) and torch.equal(x[2], y[2])
    # NULL outputs are honoured: what is asked for has the same bits, nothing else is written
    t2 = torch.full((B,), 7.0, device="cuda")
    ops.reg_fold_points(do, None, w, B, N, term=t2)
    assert torch.equal(t2, a[0])
    c2 = dc0.clone()
    ops.reg_fold_points(do, None, w, B, N, constrain=c2, constrain_add=True)
    assert torch.equal(c2, a[1])
    g2 = dg0.clone()
    ops.reg_fold_points(None, dg, w, B, N, g=g2, g_add=True)
    assert torch.equal(g2, a[2])
    assert _fold(do, dg, w, term=False, constrain=dc0, g=dg0)[0] is None


# ------------------------------------------------------------------------------------------------ 1b. the normal gradient
@pytest.mark.parametrize("n,k", [(64, 63), (256, 2), (1025, 5)])
def test_corr_normal_loss_grad_alone(n, k):
    """geoa3_corr_normal_loss_grad against float64.  Pair terms and sums are exact to double rounding; what remains is the
    float rounding of the result (2^-24 |value|) and the fixed-point unit, 2^-40 of the instance's largest pair term, on at
    most n + k terms: pair terms are 1 / (k |v|) <= ~10^2 times the largest element here, so 2^-28 max|value| covers it."""
    from geoa3_amd import ops
    ori, nrm = O.make_synthetic_clouds(3, n, seed=41)
    x = (ori + torch.randn(3, 3, n, generator=torch.Generator().manual_seed(42)) * 1e-2).contiguous()
    g = torch.rand(3, n, generator=torch.Generator().manual_seed(43)) - 0.3               # signed upstream gradient
    _, ref = R.value_and_grad(R.corresponding_normal_loss, x.double(), g.double(), nrm.double(), k=k)
    xc, nc, gc = x.cuda(), nrm.cuda(), g.cuda()
    got = ops.corr_normal_loss_grad(xc, nc, k, g=gc)
    err = (got.cpu().double() - ref).abs()
    bound = 2 * U24 * ref.abs() + 2.0 ** -28 * ref.abs().amax((1, 2), keepdim=True)
    print("n %d k %d  err / bound max %.3f" % (n, k, float((err / bound).max())))
    assert (err <= bound).all()
    # the same bits again, from a wider table, and for a row alone; g = None means ones
    wide = ops.knn_self_planar(xc, min(k + 4, n))
    assert torch.equal(got, ops.corr_normal_loss_grad(xc, nc, k, g=gc))
    assert torch.equal(got, ops.corr_normal_loss_grad(xc, nc, k, g=gc, knn=wide))
    assert torch.equal(got[1:2], ops.corr_normal_loss_grad(xc[1:2].contiguous(), nc[1:2].contiguous(), k, g=gc[1:2].contiguous()))
    assert torch.equal(ops.corr_normal_loss_grad(xc, nc, k), ops.corr_normal_loss_grad(xc, nc, k, g=torch.ones_like(gc)))
    # a non-finite coordinate: its row NaN, the others untouched
    bad = xc.clone()
    bad[1, 0, 5] = float("nan")
    gb = ops.corr_normal_loss_grad(bad, nc, k, g=gc)
    assert torch.isnan(gb[1]).all() and torch.equal(gb[0], got[0]) and torch.equal(gb[2], got[2])


# ------------------------------------------------------------------------------------------------ 2. weights zero
def test_loop_weights_zero_is_bit_identical(net):
    from tests.test_gpu_attack import _run
    ori, nrm, gt, inits = _inputs()
    kw = dict(binary_max_steps=1, iter_max_steps=4, curv_loss_knn=4)
    a = _run(net, O.AttackCfg(**kw), ori, nrm, gt, None, False, inits)
    b = _run(net, O.AttackCfg(displacement_loss_weight=0.0, displacement_loss_knn=8, repulsion_loss_weight=0.0,
                              repulsion_loss_knn=6, repulsion_loss_h=0.05, corr_normal_loss_weight=0.0,
                              corr_normal_loss_knn=3, reg_share_table=False, **kw), ori, nrm, gt, None, False, inits)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    for name in ("offset", "m", "v", "x", "loss_hist", "best_attack", "best_loss"):
        assert torch.equal(a[0].t[name], b[0].t[name]), name
    assert not [name for name in b[0].t if name.startswith(NEW_BUFFERS)]
    assert b[0].knn_searches_per_iteration == 1


# ------------------------------------------------------------------------------------------------ 3. each term alone
@pytest.mark.parametrize("term,k", [("disp", 16), ("rep", 4), ("cn", 2)])
def test_loop_term_alone(net, term, k):
    """Only this term (no distance / curvature term, no classification loss): loss_n = c w mean_i(term), and the first Adam
    step is the one torch computes from g = (c / b) w d mean_i(term) / dx."""
    from tests.test_gpu_attack import _run
    w, lr, c0, h = W[term], 0.002, 10.0, 2.0 ** -5
    cfg = O.AttackCfg(dis_loss_type="None", hd_loss_weight=0.0, curv_loss_weight=0.0, cls_loss_type="None",
                      binary_max_steps=1, iter_max_steps=2, lr=lr, initial_const=c0,
                      **_term_kw(term, w, k, h if term == "rep" else None))
    ori, nrm, gt, inits = _inputs()
    b = ori.shape[0]
    S, dS = _ref(term, 256, k, h)
    r, _, xs, _ = _run(net, cfg, ori, nrm, gt, None, False, inits)
    hist = r.t["loss_hist"].cpu().numpy()
    print(term, "loss_hist[0] / (c w mean64) - 1:", (hist[0] / (c0 * w * S).numpy() - 1).tolist())
    np.testing.assert_allclose(hist[0], (c0 * w * S).numpy(), rtol=1e-6)
    off = inits[0].clone().requires_grad_()
    opt = torch.optim.Adam([off], lr=lr)
    off.grad = ((c0 / b) * w * dS).float()
    opt.step()
    step = xs[1] - xs[0]
    ref_step = (off.detach() - inits[0]).numpy()
    moved = (dS.abs() > 1e-3 * dS.abs().max()).numpy()
    assert moved.any()
    np.testing.assert_allclose(step[moved], ref_step[moved], rtol=1e-4, atol=1e-7)


# ------------------------------------------------------------------------------------------------ 4. beside the others
def _objective(net, cfg, ori, nrm, gt, init):
    from geoa3_amd.attack import AttackRunner
    r = AttackRunner(net, ori.shape[0], ori.shape[2], cfg, torch.device("cuda"))
    r.setup(ori, nrm, gt, gt)
    r.begin_search_step(init.cuda())
    g_cls, g_geo = r.objective(0, 0)
    torch.cuda.synchronize()
    r.end_search_step()
    return r, r.geo_out["constrain"].cpu().double(), g_geo.cpu().double()


@pytest.mark.parametrize("n,ks,curv_k", [(256, (16, 4, 2), 16), (256, (8, 12, 3), 8), (64, (63, 63, 63), 8)])
def test_loop_terms_beside_the_others(net, n, ks, curv_k):
    """One objective() on the same x with and without the three terms, beside CD + HD + curvature + kNN smoothing:
    constrain_with = constrain_without + sum_t w_t term_t and g_with = g_without + sum_t (w_t / n) grad_t, each within
    8 * 2^-24 * (the sum of the magnitudes of the summands: the value without the terms and the three terms' shares,
    float64 reference).  The folds round a running float32 sum that starts at the value without the terms, so that value
    is one of the summands.  n = 64 with k + 1 == n: every other point is a neighbour.

    Measured on an MI355X (error / bound, largest element): constrain 0.049 / 0.081 / 0.041 for the three cases, gradient
    0.342 / 0.386 / 0.322; each term's gradient alone against the same bound 0.06-0.12.  All three backward kernels form
    their pair terms in double from the float32 cloud.  With float32 intermediates the bound is out of reach: theta of the
    displacement term in float32 gave 3.2 / 3.2 / 8.7, the table's float32 distances in the repulsion term 0.66 / 0.42 /
    0.08, the float32 dkappa path of geoa3_geo_loss_grad for the normal term 1.18 / 1.03 / 0.27 (torch's float32 autograd
    of tests/_reg_ref.corresponding_normal_loss on the CPU: 5.4 / 1.3 / 9.5)."""
    h = 2.0 ** -5
    ori, nrm, gt, inits = _inputs(n=n)
    base = dict(binary_max_steps=1, iter_max_steps=2, curv_loss_knn=curv_k, is_use_knn_smoothing_loss=True,
                knn_smoothing_loss_weight=5.0, knn_smoothing_k=5, knn_threshold_coef=1.10)
    kw = {}
    for term, k in zip(("disp", "rep", "cn"), ks):
        kw.update(_term_kw(term, W[term], k, h))
    refs = [_ref(term, n, k, h) for term, k in zip(("disp", "rep", "cn"), ks)]
    _, c0, g0 = _objective(net, O.AttackCfg(**base), ori, nrm, gt, inits[0])
    r, c1, g1 = _objective(net, O.AttackCfg(**base, **kw), ori, nrm, gt, inits[0])
    cs = [W[term] * S for term, (S, _) in zip(("disp", "rep", "cn"), refs)]
    gs = [W[term] * dS for term, (_, dS) in zip(("disp", "rep", "cn"), refs)]     # dS is d mean / dx = grad / n already
    cerr, cmag = (c1 - c0 - sum(cs)).abs(), c0.abs() + sum(x.abs() for x in cs)
    gerr, gmag = (g1 - g0 - sum(gs)).abs(), g0.abs() + sum(x.abs() for x in gs)
    print("n %d k %s  constrain err / bound %.3f   gradient err / bound max %.3f  (|without| / sum: constrain %.3f)"
          % (n, ks, float((cerr / (8 * U24 * cmag)).max()), float((gerr / (8 * U24 * gmag)).max()),
             float((c0.abs() / cmag).max())))
    for name, S in zip(("disp_loss", "rep_loss", "cn_loss"), refs):
        np.testing.assert_allclose(r.t[name].cpu().numpy(), S[0].numpy(), rtol=1e-6)
    assert (cerr <= 8 * U24 * cmag).all()
    assert (gerr <= 8 * U24 * gmag).all()


# ------------------------------------------------------------------------------------------------ 5. tables
def test_loop_shared_and_own_tables_are_bit_identical(net):
    from tests.test_gpu_attack import _run
    ori, nrm, gt, inits = _inputs()
    kw = dict(binary_max_steps=1, iter_max_steps=5, curv_loss_knn=8, displacement_loss_weight=W["disp"],
              displacement_loss_knn=8, repulsion_loss_weight=W["rep"], corr_normal_loss_weight=W["cn"])
    a = _run(net, O.AttackCfg(**kw), ori, nrm, gt, None, False, inits)
    b = _run(net, O.AttackCfg(reg_share_table=False, **kw), ori, nrm, gt, None, False, inits)
    assert a[0].reg_share and a[0].disp_share and "reg_knn" not in a[0].t and "disp_knn" not in a[0].t
    assert not b[0].reg_share and len(b[0].t["reg_knn"]) == 2 and b[0].t["reg_knn"][0].shape[2] == 5
    assert a[0].knn_searches_per_iteration == 1 and b[0].knn_searches_per_iteration == 2
    assert np.array_equal(a[2], b[2])
    for name in ("loss_hist", "disp_loss", "rep_loss", "cn_loss"):
        assert torch.equal(a[0].t[name], b[0].t[name]), name
    off = _run(net, O.AttackCfg(binary_max_steps=1, iter_max_steps=5, curv_loss_knn=8), ori, nrm, gt, None, False, inits)
    assert not np.array_equal(a[2], off[2])           # the terms move the iterates


def test_loop_wider_term_takes_one_search_of_its_own(net):
    """k_r > curv_loss_knn: ONE extra search per iteration, of max(k_r, k_n) + 1 columns, for both terms; the displacement
    term's wider table of the clean cloud is built once per batch."""
    from tests.test_gpu_attack import _run
    ori, nrm, gt, inits = _inputs()
    r = _run(net, O.AttackCfg(binary_max_steps=1, iter_max_steps=3, curv_loss_knn=8, displacement_loss_weight=W["disp"],
                              displacement_loss_knn=12, repulsion_loss_weight=W["rep"], repulsion_loss_knn=12,
                              corr_normal_loss_weight=W["cn"], corr_normal_loss_knn=3, is_use_knn_smoothing_loss=True,
                              knn_smoothing_loss_weight=5.0, knn_smoothing_k=5), ori, nrm, gt, None, False, inits)[0]
    assert not r.reg_share and r.knn_share and not r.disp_share
    assert [tuple(x.shape) for x in r.t["reg_knn"]] == [(3, 256, 13)] * 2 and tuple(r.t["cn_knn"].shape) == (3, 256, 4)
    assert tuple(r.t["disp_knn"].shape) == (3, 256, 13)
    assert r.knn_searches_per_iteration == 2
    assert torch.isfinite(r.t["loss_hist"]).all()


# ------------------------------------------------------------------------------------------------ 6. sharding
def test_loop_sharded_rows_equal_full_batch(net):
    from tests.test_gpu_attack import _run
    ori, nrm, gt, inits = _inputs(b=4)
    cfg = lambda: O.AttackCfg(binary_max_steps=1, iter_max_steps=4, curv_loss_knn=4, displacement_loss_weight=W["disp"],
                              displacement_loss_knn=8, repulsion_loss_weight=W["rep"], corr_normal_loss_weight=W["cn"],
                              late_join=False)
    full = _run(net, cfg(), ori, nrm, gt, None, False, inits)
    for lo, hi in ((0, 2), (2, 4)):
        part = _run(net, cfg(), ori[lo:hi], nrm[lo:hi], gt[lo:hi], None, False, [inits[0][lo:hi]], global_batch=4)
        assert np.array_equal(part[2], full[2][:, lo:hi])
        assert torch.equal(part[0].t["loss_hist"], full[0].t["loss_hist"][:, lo:hi])


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_at_construction(net):
    from geoa3_amd.attack import AttackRunner
    dev = torch.device("cuda")
    for term in ("disp", "rep", "cn"):
        for n, k in ((256, 0), (256, 64), (64, 64), (32, 32)):       # 1 <= k, k + 1 <= min(n, 64)
            with pytest.raises(ValueError):
                AttackRunner(net, 2, n, O.AttackCfg(**_term_kw(term, 1.0, k)), dev)
        AttackRunner(net, 2, 64, O.AttackCfg(curv_loss_knn=4, **_term_kw(term, 1.0, 63)), dev)
    for term in ("disp", "cn"):                                     # the sample has no index correspondence
        with pytest.raises(ValueError):
            AttackRunner(net, 2, 256, O.AttackCfg(is_subsample_opt=True, npoint=64, curv_loss_knn=4,
                                                  **_term_kw(term, 1.0)), dev)
        AttackRunner(net, 2, 64, O.AttackCfg(is_subsample_opt=True, npoint=64, curv_loss_knn=4, **_term_kw(term, 1.0)), dev)


def test_repulsion_on_the_dense_subsample_path(net):
    """Nothing but the repulsion term, on the farthest-point sample: the iterates move."""
    from tests.test_gpu_attack import _run
    ori, nrm, gt, inits = _inputs()
    kw = dict(is_subsample_opt=True, npoint=64, eval_num=1, dis_loss_type="None", hd_loss_weight=0.0, curv_loss_weight=0.0,
              cls_loss_type="None", binary_max_steps=1, iter_max_steps=3, lr=0.002)
    moved = _run(net, O.AttackCfg(repulsion_loss_weight=W["rep"], **kw), ori, nrm, gt, None, False, inits)
    assert moved[0].sub and "reg_knn" in moved[0].t
    assert np.isfinite(moved[2]).all() and not np.array_equal(moved[2][-1], moved[2][0])
    assert torch.isfinite(moved[0].t["loss_hist"]).all() and (moved[0].t["loss_hist"] != 0).all()


# ------------------------------------------------------------------------------------------------ 8. info_line, CLI
def test_info_line_reports_the_active_terms(net):
    from tests.test_gpu_attack import _run
    ori, nrm, gt, inits = _inputs()
    kw = dict(binary_max_steps=1, iter_max_steps=2, curv_loss_knn=4)
    r = _run(net, O.AttackCfg(displacement_loss_weight=W["disp"], displacement_loss_knn=4, repulsion_loss_weight=W["rep"],
                              corr_normal_loss_weight=W["cn"], is_use_knn_smoothing_loss=True, knn_smoothing_loss_weight=5.0,
                              **kw), ori, nrm, gt, None, False, inits)[0]
    line = r.info_line(0, 1, 0, 1)
    assert line.index("knn_smooth") < line.index("disp_loss") < line.index("rep_loss") < line.index("cnor_loss")
    vals = {f.split(":")[0].strip(): float(f.split(":")[1]) for f in line.split("\t") if ":" in f}
    assert vals["rep_loss"] == pytest.approx(float(r.t["rep_loss"].mean()), abs=1e-4)
    assert vals["cnor_loss"] == pytest.approx(float(r.t["cn_loss"].mean()), abs=1e-4)
    r = _run(net, O.AttackCfg(repulsion_loss_weight=W["rep"], **kw), ori, nrm, gt, None, False, inits)[0]
    line = r.info_line(0, 1, 0, 1)
    assert "rep_loss" in line and "disp_loss" not in line and "cnor_loss" not in line and "knn_smooth" not in line


def test_cli_runs_with_the_flags(tmp_path, monkeypatch):
    import main_attack
    monkeypatch.chdir(tmp_path)
    args = ["--attack", "GeoA3", "--attack_label", "Untarget", "-b", "125", "--npoint", "256", "--synthetic",
            "--data_dir_file", str(tmp_path / "Data" / "syn256.mat"), "--binary_max_steps", "2", "--iter_max_steps",
            "6", "--lr", "0.005", "--curv_loss_knn", "8", "--displacement_loss_weight", "0.5", "--repulsion_loss_weight",
            "0.25", "--corr_normal_loss_weight", "0.125", "--quiet"]
    saved_dir = main_attack.main(main_attack.build_parser().parse_args(args))
    assert saved_dir.endswith("_k8_Disp0.5_k16_Rep0.25_k4_h0.03_CorrNor0.125_k2")
    rate = float(open(os.path.join(saved_dir, "attack_result.txt")).read().split(":")[1])
    mats = sorted(glob.glob(os.path.join(saved_dir, "Mat", "adv_*.mat")))
    assert len(mats) == round(rate * 250 / 100.0) and len(mats) > 0


# ------------------------------------------------------------------------------------------------ 9. the runner cache key
class _RecordingCfg:
    """cfg, remembering every attribute name asked of it"""

    def __init__(self, cfg):
        self._cfg, self._asked = cfg, set()

    def __getattr__(self, name):
        self._asked.add(name)
        return getattr(self._cfg, name)


@pytest.mark.parametrize("kw", [
    dict(uniform_loss_weight=1.0, is_use_knn_smoothing_loss=True, knn_smoothing_loss_weight=5.0, displacement_loss_weight=1.0,
         repulsion_loss_weight=1.0, corr_normal_loss_weight=1.0, is_pro_grad=True),
    dict(is_subsample_opt=True, npoint=32, eval_num=2, is_pre_jitter_input=True, is_pro_grad=True),
    dict(is_subsample_opt=True, npoint=32, is_pre_jitter_input=True, is_partial_var=True)], ids=["terms", "sample", "partial"])
def test_runner_cache_key_names_every_field_the_constructor_reads(net, kw):
    """attack(..., runner_cache=) keys a runner by RUNNER_CFG_FIELDS: a field AttackRunner.__init__ reads and the tuple
    lacks would hand a stale runner to the next batch."""
    from geoa3_amd.attack import RUNNER_CFG_FIELDS, AttackRunner
    cfg = _RecordingCfg(O.AttackCfg(curv_loss_knn=8, **kw))
    AttackRunner(net, 2, 64, cfg, torch.device("cuda"))
    assert cfg._asked and cfg._asked <= set(RUNNER_CFG_FIELDS), sorted(cfg._asked - set(RUNNER_CFG_FIELDS))
