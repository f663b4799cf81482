"""The feature-propagation operators on the GPU (geoa3_pn2_three_nn / _three_interpolate / _three_interpolate_grad through
geoa3_amd.pointnet2.ext, the autograd Functions and PointnetFPModule) against the numpy restatement tests/_three_ref.py
(bit for bit where the arithmetic is pinned) and the reference's own values (tests/golden/geoa3_golden_fp.npz).

Bars: three_nn and three_interpolate are bit-equal in both roundings.  three_interpolate_grad against the float64 sum:
|got - ref| <= (count + 2) * 2^-24 * sum |g * w| per element, the float32 summation bound (count products each rounded
once, count - 1 additions) -- and bit-equal to the float32 loop in ascending entry number, the order the header
promises (three_interpolate_grad32).  Values that pass through torch on both sides in another order (sqrt, the weights, the MLP):
1e-4 * max |ref|, the bar of tests/test_gpu_uniform.py for float32 results summed in another order."""
import os

import numpy as np
import pytest
import torch

from tests import _three_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
T = torch.from_numpy
FP_CASES = ["gauss", "nofeat", "lattice"]


def _tiles():
    from geoa3_amd.pointnet2 import three_nn_tiles
    return three_nn_tiles()


@pytest.fixture(scope="module")
def gf():
    return np.load(os.path.join(REPO, "tests", "golden", "geoa3_golden_fp.npz"), allow_pickle=False)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------------------------------ three_nn
CONTENTS = ["gauss", "dup", "self", "lattice", "nonfinite"]
M_SPECS = ["1", "2", "3", "4", "T-1", "T", "T+1", "2*T+5"]
_NN_CACHE = {}


def _nn_clouds(content, m, n, seed):
    rng = np.random.default_rng(seed)
    known = rng.standard_normal((3, m, 3)).astype(np.float32)
    unknown = rng.standard_normal((3, n, 3)).astype(np.float32)
    if content == "dup":
        known[:, 1::2] = known[:, 0:m - (m % 2):2]
    elif content == "self":
        unknown = known[:, np.arange(n) % m].copy()
    elif content == "lattice":
        known = (np.round(known * 2) / 2).astype(np.float32)
        unknown = (np.round(unknown * 2) / 2).astype(np.float32)
    elif content == "nonfinite":
        known[0, 0, 1] = np.nan
        known[1, m // 2, 2] = np.inf
        known[2, m - 1, 0] = -np.inf
        unknown[0, n // 2, 0] = np.nan
        unknown[1, 0, 2] = np.inf
    return unknown, known


def _nn_case(content, mspec, contract):
    """clouds [3, U+1 | m, 3] and the restatement's answer, computed once per (content, m, rounding)"""
    key = (content, mspec, contract)
    if key not in _NN_CACHE:
        Tk, U = _tiles()
        m = int(eval(mspec, {"T": Tk}))
        unknown, known = _nn_clouds(content, m, U + 1, seed=1000 + 17 * CONTENTS.index(content) + M_SPECS.index(mspec))
        _NN_CACHE[key] = (unknown, known) + R.three_nn(unknown, known, contract)
    return _NN_CACHE[key]


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("mspec", M_SPECS)
@pytest.mark.parametrize("content", CONTENTS)
def test_three_nn_bit_equal(content, mspec, contract):
    from geoa3_amd.pointnet2 import ext
    unknown, known, d2_ref, idx_ref = _nn_case(content, mspec, contract)
    _, U = _tiles()
    for B in (1, 3):
        for n in (1, 63, 65, U + 1):
            # (every unknown point is searched on its own: the answer for the first n points of the first B instances is
            # a slice of the shared one)
            d2, idx = ext.three_nn(T(unknown[:B, :n].copy()).cuda(), T(known[:B].copy()).cuda(), contract=contract)
            assert d2.shape == (B, n, 3) and d2.dtype == torch.float32 and idx.dtype == torch.int32
            assert np.array_equal(idx.cpu().numpy(), idx_ref[:B, :n]), (B, n)
            assert np.array_equal(_bits(d2.cpu().numpy()), _bits(d2_ref[:B, :n])), (B, n)


def test_three_nn_environment_default_is_unfused():
    from geoa3_amd.pointnet2 import ext, ext_contract_default
    unknown, known, d2_ref, idx_ref = _nn_case("gauss", "T+1", ext_contract_default())
    d2, idx = ext.three_nn(T(unknown).cuda(), T(known).cuda())
    assert np.array_equal(idx.cpu().numpy(), idx_ref) and np.array_equal(_bits(d2.cpu().numpy()), _bits(d2_ref))


# ------------------------------------------------------------------------------------------ three_interpolate
def _interp_inputs(B, C, n, m, seed):
    rng = np.random.default_rng(seed)
    points = rng.standard_normal((B, C, m)).astype(np.float32)
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    idx[:, ::7] = idx[:, ::7, :1]                                   # rows with i1 == i2 == i3
    weight = rng.random((B, n, 3)).astype(np.float32)
    weight /= weight.sum(2, keepdims=True)
    return points, idx, weight


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("m", [3, 130])
@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("C", [1, 3, 65])
def test_three_interpolate_bit_equal(C, n, m, contract):
    from geoa3_amd.pointnet2 import ext
    points, idx, weight = _interp_inputs(2, C, n, m, seed=C * 1000 + n * 10 + m)
    assert (idx[:, 0, 0] == idx[:, 0, 1]).all() and (idx[:, 0, 0] == idx[:, 0, 2]).all()
    ref = R.three_interpolate(points, idx, weight, contract)
    out = ext.three_interpolate(T(points).cuda(), T(idx).cuda(), T(weight).cuda(), contract=contract)
    assert out.shape == (2, C, n) and out.dtype == torch.float32
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ref))


# ------------------------------------------------------------------------------------------ three_interpolate_grad
def _grad_inputs(kind, C, seed):
    """"same3": m = 3, n = 300, every unknown point on the same three destinations (lists of 300 entries);
    "sparse": m = 130, n = 65, only the even destinations are used"""
    rng = np.random.default_rng(seed)
    B = 3
    if kind == "same3":
        n, m = 300, 3
        idx = np.broadcast_to(np.array([2, 0, 1], dtype=np.int32), (B, n, 3)).copy()
    else:
        n, m = 65, 130
        idx = (2 * rng.integers(0, m // 2, (B, n, 3))).astype(np.int32)
    weight = rng.random((B, n, 3)).astype(np.float32)
    weight /= weight.sum(2, keepdims=True)
    g = rng.standard_normal((B, C, n)).astype(np.float32)
    return g, idx, weight, m


@pytest.mark.parametrize("C", [1, 65])
@pytest.mark.parametrize("kind", ["same3", "sparse"])
def test_three_interpolate_grad_within_summation_bound(kind, C):
    from geoa3_amd.pointnet2 import ext
    g, idx, weight, m = _grad_inputs(kind, C, seed=40 + C)
    ref, cnt, mag = R.three_interpolate_grad64(g, idx, weight, m)
    gc, ic, wc = T(g).cuda(), T(idx).cuda(), T(weight).cuda()
    out = ext.three_interpolate_grad(gc, ic, wc, m)
    assert out.shape == (3, C, m) and out.dtype == torch.float32
    got = out.cpu().numpy()
    err, bound = np.abs(got.astype(np.float64) - ref), (cnt + 2) * 2.0 ** -24 * mag
    print("three_interpolate_grad %s C=%d: max err %.3e, max err / bound %.3f" % (
        kind, C, err.max(), (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all()
    unused = np.broadcast_to(cnt == 0, got.shape)
    assert (kind == "sparse") == bool(unused.any())
    assert not _bits(got)[unused].any()                              # exact +0.0 where nobody points
    # the same call again: the same bits
    again = ext.three_interpolate_grad(gc, ic, wc, m)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    # an instance alone: the bits of its row of the batch
    for b in range(3):
        alone = ext.three_interpolate_grad(gc[b:b + 1].contiguous(), ic[b:b + 1].contiguous(), wc[b:b + 1].contiguous(), m)
        assert torch.equal(alone.view(torch.int32)[0], out.view(torch.int32)[b]), b


def _hub_inputs():
    """B = 2, n = 500 (1500 entries), m = 20, C = 3.  Instance 0: every entry on destination 7 (longer than a wavefront,
    longer than one 1024-entry tile of the sort); instance 1: exactly 64 random entries on destination 3, exactly 65 on 11,
    the other 1371 on 7.  Nobody else receives anything."""
    rng = np.random.default_rng(77)
    B, n, m, C = 2, 500, 20, 3
    idx = np.full((B, 3 * n), 7, dtype=np.int32)
    perm = rng.permutation(3 * n)
    idx[1, perm[:64]] = 3
    idx[1, perm[64:129]] = 11
    weight = rng.random((B, n, 3)).astype(np.float32)
    weight /= weight.sum(2, keepdims=True)
    g = rng.standard_normal((B, C, n)).astype(np.float32)
    return g, idx.reshape(B, n, 3), weight, m


def _grad_on_gpu(g, idx, weight, m):
    from geoa3_amd.pointnet2 import ext
    out = ext.three_interpolate_grad(T(g).cuda(), T(idx).cuda(), T(weight).cuda(), m)
    assert out.shape == (g.shape[0], g.shape[1], m) and out.dtype == torch.float32
    return out.cpu().numpy()


@pytest.mark.parametrize("C", [1, 8, 9, 65])
@pytest.mark.parametrize("kind", ["same3", "sparse"])
def test_three_interpolate_grad_bit_equal_to_ascending_float32_loop(kind, C):
    """The promised order, not only the bound: every element has the bits of the float32 loop over e = 3 j + slot ascending
    (tests/test_three_ref.py: the same loop descending changes bits in every one of these cases).  C on both sides of one
    thread's group of 8 channels; "same3": lists of 300 entries (longer than a wavefront), "sparse": lists of 0 to ~10."""
    g, idx, weight, m = _grad_inputs(kind, C, seed=40 + C)
    got = _grad_on_gpu(g, idx, weight, m)
    assert np.array_equal(_bits(got), _bits(R.three_interpolate_grad32(g, idx, weight, m)))


def test_three_interpolate_grad_hub_exact_wavefront_and_untouched_rows():
    """_hub_inputs: lists of 1500 and 1371 entries (more than one tile of the sort), of exactly 64 (the last length one
    wavefront ranks) and exactly 65 (the first the workgroup ranks), and 17 / 19 empty lists per instance, which read +0.0
    with no bit set."""
    g, idx, weight, m = _hub_inputs()
    cnt = np.stack([np.bincount(idx[b].ravel(), minlength=m) for b in range(2)])
    assert cnt[0, 7] == 1500 and (cnt[1, 3], cnt[1, 11], cnt[1, 7]) == (64, 65, 1371) and cnt.sum() == 3000
    got = _grad_on_gpu(g, idx, weight, m)
    assert np.array_equal(_bits(got), _bits(R.three_interpolate_grad32(g, idx, weight, m)))
    quiet = np.broadcast_to((cnt == 0)[:, None, :], got.shape)
    assert quiet.sum() == 3 * (19 + 17) and not _bits(got)[quiet].any()
    assert (got[~quiet] != 0).all()


def test_three_interpolate_grad_drops_indices_out_of_range():
    """An index of -1 and one of m (the caller's error) are in no list: their products are in no sum, every other sum is
    the restatement's, bit for bit."""
    g, idx, weight, m = _grad_inputs("sparse", 9, seed=60)
    idx[0, 3, 1] = -1
    idx[2, 64, 2] = m          # the last entry of the batch
    want = R.three_interpolate_grad32(g, idx, weight, m)
    ok = (idx >= 0) & (idx < m)
    clean = R.three_interpolate_grad32(g, np.where(ok, idx, 0), np.where(ok, weight, np.float32(0)), m)
    assert ok.sum() == idx.size - 2 and np.array_equal(want, clean)   # (g finite: a product with weight 0 adds +-0.0)
    got = _grad_on_gpu(g, idx, weight, m)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("kind", ["same3", "sparse"])
def test_three_interpolate_grad_nan_reaches_its_three_destinations(kind):
    from geoa3_amd.pointnet2 import ext
    g, idx, weight, m = _grad_inputs(kind, 3, seed=50)
    b, c, j = 1, 2, 17
    g[b, c, j] = np.nan
    out = ext.three_interpolate_grad(T(g).cuda(), T(idx).cuda(), T(weight).cuda(), m).cpu().numpy()
    want = np.zeros(out.shape, dtype=bool)
    want[b, c, idx[b, j]] = True
    assert np.array_equal(np.isnan(out), want)
    g[b, c, j] = np.inf
    out = ext.three_interpolate_grad(T(g).cuda(), T(idx).cuda(), T(weight).cuda(), m).cpu().numpy()
    assert np.array_equal(~np.isfinite(out), want)


# ------------------------------------------------------------------------------------------ autograd and the module
def _close(got, ref):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    return np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()


@pytest.mark.parametrize("tag", FP_CASES)
def test_autograd_functions_match_reference(gf, tag):
    from geoa3_amd import pointnet2 as P
    pre = "fp/%s/" % tag
    unknown, known = T(gf[pre + "unknown"]).cuda(), T(gf[pre + "known"]).cuda()
    dist, idx = P.three_nn(unknown, known)
    assert not dist.requires_grad and idx.dtype == torch.int32
    assert np.array_equal(idx.cpu().numpy(), gf[pre + "idx"])
    assert _close(dist, gf[pre + "dist"])
    dist_recip = 1.0 / (dist + 1e-8)
    weight = (dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)).requires_grad_()
    assert _close(weight, gf[pre + "weight"])
    kf = T(gf[pre + "known_feats"]).cuda().requires_grad_()
    interp = P.three_interpolate(kf, idx, weight)
    assert _close(interp, gf[pre + "interp"])
    # a non-contiguous cotangent: backward makes it contiguous as the reference does (pointnet2_utils.py:184-186)
    cot = T(gf[pre + "cot_interp"]).cuda().transpose(1, 2).contiguous().transpose(1, 2)
    g_kf, g_w = torch.autograd.grad(interp, (kf, weight), cot)
    assert _close(g_kf, gf[pre + "interp_grad_feats"])
    assert g_w.shape == weight.shape and not g_w.any() and not gf[pre + "interp_grad_weight"].any()


def _module(gf, pre):
    from geoa3_amd import pointnet2 as P
    names = list(gf[pre + "sd_names"])
    sd = {k: T(gf[pre + "sd/" + k]) for k in names}
    mod = P.PointnetFPModule([sd["mlp.0.weight"].shape[1], 64, 32])
    mod.load_state_dict(sd)
    return mod.cuda()


@pytest.mark.parametrize("tag", FP_CASES)
def test_fp_module_matches_reference(gf, tag):
    pre = "fp/%s/" % tag
    has_uf = (pre + "unknow_feats") in gf.files
    assert has_uf == (tag != "nofeat")                               # "nofeat": unknow_feats=None
    mod = _module(gf, pre).eval()
    unknown, known = T(gf[pre + "unknown"]).cuda(), T(gf[pre + "known"]).cuda()
    kf = T(gf[pre + "known_feats"]).cuda().requires_grad_()
    uf = T(gf[pre + "unknow_feats"]).cuda().requires_grad_() if has_uf else None
    y = mod(unknown, known, uf, kf)
    assert y.shape == gf[pre + "out_eval"].shape and _close(y, gf[pre + "out_eval"])
    grads = torch.autograd.grad(y, (kf, uf) if has_uf else (kf,), T(gf[pre + "cot_out"]).cuda())
    assert _close(grads[0], gf[pre + "grad_known_feats"])
    if has_uf:
        assert _close(grads[1], gf[pre + "grad_unknow_feats"])
    mod.train()
    y = mod(unknown, known, uf, kf)
    assert _close(y, gf[pre + "out_train"])
    # training: the weights take gradients through autograd
    y.square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in mod.parameters())
    assert float(mod.mlp[0].weight.grad.abs().max()) > 0


def test_fp_module_known_none_broadcasts(gf):
    pre = "fp/gauss/"
    mod = _module(gf, pre).eval()
    unknown = T(gf[pre + "unknown"]).cuda()
    uf = T(gf[pre + "unknow_feats"]).cuda()
    glob = T(gf[pre + "known_feats"][:, :, :1].copy()).cuda()          # [B,C2,1]: one feature vector per instance
    with torch.no_grad():
        y = mod(unknown, None, uf, glob)
        want = mod.mlp(torch.cat([glob.expand(-1, -1, unknown.size(1)), uf], dim=1).unsqueeze(-1)).squeeze(-1)
    assert y.shape == (unknown.size(0), 32, unknown.size(1)) and torch.equal(y, want)
