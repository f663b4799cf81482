"""The geometric objective for clouds of 5840..8192 points (csrc/geom_loss_wide.hip: geo_wide_pair_kernel +
geo_wide_sum_kernel): forced onto smaller clouds against geo_big_kernel, bit for bit; through the public entry against the
float64 table form of the objective (tests/_geo_table_ref.py, pinned to the dense oracle by tests/test_geo_table_ref.py);
its loudness; and the callers that could not run their own loss on a dense cloud.
Runs on the GPU box: python -m pytest tests -m gpu"""
import ctypes
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import geoa3_oracle as O
from tests import _geo_table_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from geoa3_amd import ops as _ops
    assert torch.cuda.is_available(), "needs the MI355X"
    return _ops


def dev(x):
    return x.contiguous().cuda()


def _clouds(B, N, Nr, k, ncoin=0):
    ori, nrm = O.make_synthetic_clouds(B, Nr, seed=N + k)
    g = torch.Generator().manual_seed(N)
    adv = ori[:, :, :N] + 0.02 * torch.randn(B, 3, N, generator=g)
    if ncoin:
        adv[:, :, 100:100 + ncoin] = adv[:, :, 100:101]
    return adv, ori, nrm, g


def _objective_inputs(ops, adv, ori, nrm, k):      # as tests/test_gpu_geometry.py builds them
    advD, oriD, nrmD = dev(adv), dev(ori), dev(nrm)
    d_ao, i_ao, d_oa, i_oa = ops.nn1_pair(advD, oriD)
    _, knn_ori = ops.knn_planar(oriD, oriD, k + 1)
    kap = ops.kappa(oriD, nrmD, knn_ori)
    _, knn_adv = ops.knn_planar(advD, advD, k + 1)
    return dict(normal_ori=nrmD, kappa_ori=kap, d_ao=d_ao, i_ao=i_ao, d_oa=d_oa, i_oa=i_oa, knn_adv=knn_adv, k=k,
                dis_type=1, w_dis=1.0, w_hd=0.1, w_curv=1.0), advD, oriD


LOSSES = ("dis_loss", "hd_loss", "curv_loss", "constrain")


def _fits(ops, B, N, ranges):
    """Whether that many owner ranges fit LDS, from the library itself (a values-only call: ENOSUPPORT or not)."""
    from geoa3_amd import _lib
    z = torch.zeros(B, 3, N, device="cuda")
    try:
        ops.geo_loss_grad(z, z, dis_type=2, want_grad=False, wide_ranges=ranges)
        return True
    except _lib.Geoa3Error as e:
        assert "(%d)" % _lib.ENOSUPPORT in str(e)
        return False


# ---------------------------------------------------------------------------------------------- 1. forced, against geo_big_kernel
@pytest.mark.parametrize("N,Nr,k,ncoin", [(1500, 1500, 16, 0), (2048, 2048, 32, 0), (1500, 3000, 16, 0), (1100, 1100, 40, 0),
                                          (4096, 4096, 32, 130)])
def test_forced_wide_kernels_return_geo_big_kernels_bits(ops, N, Nr, k, ncoin):
    """Both kernels evaluate the same expressions per pair and per point and add the gradient terms as integers, so the
    gradient and kappa_adv agree BIT FOR BIT for 1, 2 and 4 owner ranges, every point included (points 100..229 coincide
    in the last case: zero-length pairs, a hub of the neighbour graph).  The loss values are summed per 1024 points
    instead of per lane stride: rtol 2e-5 against geo_big_kernel, and the same bits for every number of ranges.  The
    same in dkappa mode."""
    B = 3
    adv, ori, nrm, g = _clouds(B, N, Nr, k, ncoin)
    kw, advD, oriD = _objective_inputs(ops, adv, ori, nrm, k)
    big = ops.geo_loss_grad(advD, oriD, deterministic=True, want_kappa=True, scratch=ops.geo_scratch(B, N, "cuda", k), **kw)
    dk = torch.randn(B, N, generator=g).cuda()
    vjp = dict(kw)
    vjp.update(w_dis=0.0, w_hd=0.0, w_curv=0.0, dis_type=0)
    big_vjp = ops.geo_loss_grad(advD, oriD, deterministic=True, dkappa=dk, scratch=ops.geo_scratch(B, N, "cuda", k), **vjp)
    assert torch.isfinite(big["grad"]).all() and torch.isfinite(big_vjp["grad"]).all()
    first, ran = None, []
    for ranges in (1, 2, 4):
        if not _fits(ops, B, N, ranges):
            continue
        ran.append(ranges)
        got = ops.geo_loss_grad(advD, oriD, want_kappa=True, wide_ranges=ranges, **kw)
        print(N, Nr, k, "ranges", ranges, "max |dgrad|", float((got["grad"] - big["grad"]).abs().max()),
              "max |dkappa|", float((got["kappa_adv"] - big["kappa_adv"]).abs().max()),
              "constrain", got["constrain"].tolist(), big["constrain"].tolist())
        assert torch.equal(got["kappa_adv"], big["kappa_adv"]), ranges
        assert torch.equal(got["grad"], big["grad"]), ranges
        for name in LOSSES:
            np.testing.assert_allclose(got[name].cpu().numpy(), big[name].cpu().numpy(), rtol=2e-5,
                                       atol=1e-8 if name == "constrain" else 1e-9)
        if first is None:
            first = {n: got[n].clone() for n in LOSSES}
        for name in LOSSES:
            assert torch.equal(got[name], first[name]), (name, ranges)
        got_vjp = ops.geo_loss_grad(advD, oriD, dkappa=dk, wide_ranges=ranges, **vjp)
        print("   dkappa mode: max |dgrad|", float((got_vjp["grad"] - big_vjp["grad"]).abs().max()))
        assert torch.equal(got_vjp["grad"], big_vjp["grad"]), ranges
    assert 4 in ran and (1 in ran) == (N <= 4096)
    # the dispatcher's own choice, and a values-only call
    auto = ops.geo_loss_grad(advD, oriD, wide_ranges=0, **kw)
    assert torch.equal(auto["grad"], big["grad"])
    vals = ops.geo_loss_grad(advD, oriD, want_grad=False, wide_ranges=0, **kw)
    for name in LOSSES:
        assert torch.equal(vals[name], first[name]), name


# ---------------------------------------------------------------------------------------------- 2. the public path
PUBLIC = [(5840, 5840, 16, {}), (6001, 6001, 20, {}), (8192, 8192, 32, {}), (6144, 8192, 16, {}),
          (8192, 8192, 16, dict(w_curv=0.0, no_table=True)), (8192, 8192, 16, dict(single_side=True)),
          (8192, 8192, 16, dict(dis_type=2))]


def _table_reference(kw, advD, oriD):
    """float64, from the tables the kernel was given; the Hausdorff point from the fp32 d_ao on both sides"""
    return T.objective(advD, oriD, normal_ori=kw.get("normal_ori"), kappa_ori=kw.get("kappa_ori"), i_ao=kw["i_ao"],
                       i_oa=kw.get("i_oa"), knn_adv=kw.get("knn_adv"), hd_arg=kw["d_ao"].cpu().argmax(1),
                       dis_type=kw["dis_type"], single_side=kw.get("single_side", False), w_dis=kw["w_dis"], w_hd=kw["w_hd"],
                       w_curv=kw["w_curv"])


@pytest.mark.parametrize("N,Nr,k,mod", PUBLIC, ids=lambda v: "-".join(sorted(v)) or "full" if isinstance(v, dict) else str(v))
def test_objective_beyond_one_workgroups_lds(ops, N, Nr, k, mod):
    """ops.geo_loss_grad at the sizes the one-workgroup kernel refuses (GEOA3_ENOSUPPORT before the two-pass kernels): the
    first such size, an odd tail, the ceiling, a clean cloud larger than the sample, and at 8192 points Chamfer + Hausdorff
    without a table, the one-sided Chamfer distance and the L2 distance.  Against the float64 table form at the bars the
    smaller sizes are held to the oracle with; three repeats bit for bit; instance 1 alone and inside 19 copies."""
    B = 2
    adv, ori, nrm, _ = _clouds(B, N, Nr, k)
    kw, advD, oriD = _objective_inputs(ops, adv, ori, nrm, k)
    mod = dict(mod)
    if mod.pop("no_table", False):
        for name in ("normal_ori", "kappa_ori", "knn_adv"):
            kw[name] = None
        kw["k"] = 0
    kw.update(mod)
    want_kappa = kw["knn_adv"] is not None
    out = ops.geo_loss_grad(advD, oriD, deterministic=True, want_kappa=want_kappa, **kw)
    con, grad = out["constrain"].clone(), out["grad"].clone()
    ref = _table_reference(kw, advD, oriD)
    scale = max(ref["grad"].abs().max().item(), 1.0)
    print(N, Nr, k, mod, "constrain", con.tolist(), ref["constrain"].tolist(), "max |dgrad|",
          float((grad.cpu().double() - ref["grad"]).abs().max()), "scale", scale)
    np.testing.assert_allclose(con.cpu().numpy(), ref["constrain"].numpy(), rtol=5e-5, atol=1e-7)
    for name in ("dis_loss", "hd_loss", "curv_loss"):
        np.testing.assert_allclose(out[name].cpu().numpy(), ref[name].numpy(), rtol=5e-5, atol=1e-7)
    np.testing.assert_allclose(grad.cpu().numpy(), ref["grad"].numpy(), rtol=2e-4, atol=2e-6 * scale)
    if want_kappa:
        np.testing.assert_allclose(out["kappa_adv"].cpu().numpy(), ref["kappa_adv"].numpy(), rtol=2e-5, atol=2e-6)
    for _ in range(3):
        again = ops.geo_loss_grad(advD, oriD, deterministic=True, **kw)
        assert torch.equal(again["grad"], grad) and torch.equal(again["constrain"], con)
    free = ops.geo_loss_grad(advD, oriD, deterministic=False, **kw)        # the same order-free sums
    assert torch.equal(free["grad"], grad) and torch.equal(free["constrain"], con)
    one = {n: (v[1:2].contiguous() if torch.is_tensor(v) else v) for n, v in kw.items()}
    alone = ops.geo_loss_grad(advD[1:2].contiguous(), oriD[1:2].contiguous(), deterministic=True, **one)
    assert torch.equal(alone["grad"][0], grad[1]) and torch.equal(alone["constrain"][0], con[1])
    many = {n: (v[1:2].expand(19, *v.shape[1:]).contiguous() if torch.is_tensor(v) else v) for n, v in kw.items()}
    big = ops.geo_loss_grad(advD[1:2].expand(19, 3, N).contiguous(), oriD[1:2].expand(19, 3, Nr).contiguous(),
                            deterministic=True, **many)
    assert torch.equal(big["grad"][7], grad[1]) and torch.equal(big["grad"][18], grad[1]) and torch.equal(big["constrain"][18], con[1])


# ---------------------------------------------------------------------------------------------- 3. loudness
def test_wide_objective_is_loud_about_nan_and_huge_terms(ops):
    """As geo_big_kernel (tests/test_gpu_geometry.py): a NaN coordinate, or a pair term beyond the coarse range (dkappa =
    1e30 on a pair 1e-7 apart), gives NaN at the points it reaches, never a finite clamp -- and leaves the other
    instance alone."""
    B, N, k = 2, 6144, 16
    adv, ori, nrm, _ = _clouds(B, N, N, k)
    kw, advD, oriD = _objective_inputs(ops, adv, ori, nrm, k)
    bad = advD.clone()
    bad[0, 1, 77] = float("nan")
    got = ops.geo_loss_grad(bad, oriD, deterministic=True, **kw)["grad"]
    assert torch.isnan(got[0, :, 77]).all() and torch.isfinite(got[1]).all()
    adv2 = adv.clone()
    adv2[:, :, 301] = adv2[:, :, 300] + 1e-7
    kw2, adv2D, _ = _objective_inputs(ops, adv2, ori, nrm, k)
    dk = torch.ones(B, N).cuda()
    dk[0, 300] = 1e30
    vjp = dict(kw2)
    vjp.update(w_dis=0.0, w_hd=0.0, w_curv=0.0, dis_type=0)
    got = ops.geo_loss_grad(adv2D, oriD, deterministic=True, dkappa=dk, **vjp)["grad"]
    assert not torch.isfinite(got[0, :, 301]).all()
    assert torch.isfinite(got[1]).all()


# ---------------------------------------------------------------------------------------------- 4. callers
def test_loss_utils_on_a_dense_cloud():
    """chamfer_loss, hausdorff_loss, curvature_loss and corresponding_normal_loss with autograd at 6144 points (each failed
    with "geoa3_geo_loss_grad failed" there): values and gradients against the float64 table form, at the bars of
    test_loss_utils_unequal_cloud_sizes."""
    from geoa3_amd import loss_utils as LU
    from geoa3_amd import ops
    B, N, k = 2, 6144, 16
    adv, ori, nrm, _ = _clouds(B, N, N, k)
    kw, advD, oriD = _objective_inputs(ops, adv, ori, nrm, k)
    nrmD = kw["normal_ori"]
    common = dict(normal_ori=nrmD, kappa_ori=kw["kappa_ori"], i_ao=kw["i_ao"], i_oa=kw["i_oa"], knn_adv=kw["knn_adv"],
                  hd_arg=kw["d_ao"].cpu().argmax(1))
    for fn, ref in ((LU.chamfer_loss, dict(dis_type=1, w_dis=1.0)), (LU.hausdorff_loss, dict(dis_type=0, w_dis=0.0, w_hd=1.0))):
        a = advD.clone().requires_grad_()
        v = fn(a, oriD)
        v.sum().backward()
        want = T.objective(advD, oriD, **common, **ref)
        np.testing.assert_allclose(v.detach().cpu().numpy(), want["constrain"].numpy(), rtol=2e-5, atol=1e-8)
        np.testing.assert_allclose(a.grad.cpu().numpy(), want["grad"].numpy(), rtol=1e-4, atol=1e-8)
    a = advD.clone().requires_grad_()
    ka, _ = LU._get_kappa_adv(a, oriD, nrmD, k)
    c = LU.curvature_loss(a, oriD, ka, kw["kappa_ori"])
    c.sum().backward()
    want = T.objective(advD, oriD, **common, dis_type=0, w_dis=0.0, w_curv=1.0)
    np.testing.assert_allclose(ka.detach().cpu().numpy(), want["kappa_adv"].numpy(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(c.detach().cpu().numpy(), want["curv_loss"].numpy(), rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(a.grad.cpu().numpy(), want["grad"].numpy(), rtol=2e-3, atol=2e-6)
    # corresponding_normal_loss: the point's own normal (the identity as nearest-point index), upstream gradient w
    w = torch.randn(B, N, generator=torch.Generator().manual_seed(3))
    nadv = dev(nrm[:, :, :N])
    a = advD.clone().requires_grad_()
    v = LU.corresponding_normal_loss(a, nadv, k)
    (v * w.cuda()).sum().backward()
    ident = torch.arange(N).unsqueeze(0).expand(B, N)
    want = T.objective(advD, advD, normal_ori=nadv, i_ao=ident, knn_adv=kw["knn_adv"], dis_type=0, w_dis=0.0, dkappa=w)
    np.testing.assert_allclose(v.detach().cpu().numpy(), want["kappa_adv"].numpy(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(a.grad.cpu().numpy(), want["grad"].numpy(), rtol=2e-3, atol=2e-6)


@pytest.mark.parametrize("kind", ["full", "cd_only"])
def test_attack_on_a_dense_cloud_is_reproducible(kind):
    """attack() at 6144 points (AttackRunner allocates the objective's scratch, with or without the curvature term): 2
    binary steps of 3 iterations, twice from the same offsets -- the same clouds, success mask and loss history bit for bit,
    every loss finite."""
    from geoa3_amd.attack import attack
    from geoa3_amd.data import synthetic_clouds, synthetic_state_dict
    from geoa3_amd.pointnet import PointNet
    b, n = 2, 6144
    net = PointNet(40)
    net.load_state_dict(synthetic_state_dict(40, seed=0))
    net = net.cuda().eval()
    ori, nrm = synthetic_clouds(b, n, seed=7)
    with torch.no_grad():
        gt = net(ori.cuda()).argmax(1).cpu()
    full = kind == "full"
    cfg = Namespace(attack_label="Untarget", binary_max_steps=2, iter_max_steps=3, lr=0.01, initial_const=10.0,
                    optim="adam", cls_loss_type="CE", confidence=0.0, dis_loss_type="CD", dis_loss_weight=1.0,
                    is_cd_single_side=False, hd_loss_weight=0.1 if full else 0.0, curv_loss_weight=1.0 if full else 0.0,
                    curv_loss_knn=16, uniform_loss_weight=0.0, is_use_lr_scheduler=False, cc_linf=0.0, classes=40)
    data = [ori.permute(0, 2, 1).unsqueeze(1).contiguous(), nrm.permute(0, 2, 1).unsqueeze(1).contiguous(), gt.view(b, 1)]
    g = torch.Generator().manual_seed(11)
    init = [(torch.randn(b, 3, n, generator=g) * 1e-3).cuda() for _ in range(2)]
    runs = []
    for _ in range(2):
        best, _, succ, _, all_loss = attack(net, data, cfg, 0, 1, init_offsets=[t.clone() for t in init], verbose=False)
        runs.append((best.clone(), np.asarray(succ).copy(), np.asarray(all_loss, dtype=np.float32)))
    assert runs[0][2].shape == (3, b) and np.isfinite(runs[0][2]).all()
    assert torch.equal(runs[0][0], runs[1][0])
    assert (runs[0][1] == runs[1][1]).all() and (runs[0][2] == runs[1][2]).all()


def test_still_refused(ops):
    from geoa3_amd import _lib
    z = torch.zeros(1, 3, 8193, device="cuda")
    with pytest.raises(_lib.Geoa3Error, match="geoa3_geo_loss_grad failed"):
        ops.geo_loss_grad(z, z, dis_type=2)
    z = torch.zeros(1, 3, 5840, device="cuda")
    out = torch.zeros(1, device="cuda")
    a = _lib.GeoArgs(adv=z.data_ptr(), ori=z.data_ptr(), B=1, N=5840, Nr=5840, dis_type=2, w_dis=1.0, constrain=out.data_ptr(),
                     deterministic=1, scratch=None)
    assert _lib.load().geoa3_geo_loss_grad(ctypes.byref(a), torch.cuda.current_stream().cuda_stream) == _lib.ENOSUPPORT
    torch.cuda.synchronize()
