"""knn_gather and the backward passes of knn_gather / knn_points on the device (csrc/geom_knn_ops.hip), BIT FOR BIT against the
float32 loops of tests/_knn_ops_ref.py (pinned to float64 autograd in tests/test_knn_ops_ref.py): every sum sequential, from
+0.0, in ascending entry number.  Every output is pre-filled with NaN before every call; inputs are of order one, so every
term is a normal number or an exact zero."""
import numpy as np
import pytest
import torch

from tests import _knn_ops_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same(got, want):
    """the same bits, element for element (a NaN equals a NaN)"""
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (g.shape, w.shape)
    gn, wn = np.isnan(g.view(np.float32)), np.isnan(w.view(np.float32))
    return bool(np.array_equal(gn, wn) and np.array_equal(g[~gn], w[~wn]))


def _signed(shape, g):
    """magnitudes in [0.5, 1.5), random signs"""
    return ((torch.rand(shape, generator=g) + 0.5) * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)).float()


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda", dtype=torch.float32)


def _guarded(shape, pad=64, fill=-7.5):
    """an output inside a larger buffer: (buffer, the contiguous view of `shape` pre-filled with NaN, check of the guards)"""
    n = int(np.prod(shape))
    buf = torch.full((pad + n + pad,), fill, device="cuda", dtype=torch.float32)
    view = buf[pad:pad + n].view(shape)
    view.fill_(NAN)
    return view, lambda: bool((buf[:pad] == fill).all() and (buf[pad + n:] == fill).all())


@pytest.fixture(scope="module")
def ops():
    from geoa3_amd import ops as _ops
    assert torch.cuda.is_available(), "needs the MI355X"
    return _ops


# ------------------------------------------------------------------------------------------------ gather and its gradient
@pytest.mark.parametrize("M,K,U", [(45, 5, 1), (45, 5, 3), (45, 5, 5), (45, 5, 64), (45, 1, 3), (45, 64, 3),
                                   (18840, 5, 5), (18840, 5, 64)])
def test_gather_and_gradient_random_indices(ops, M, K, U):
    """U on both sides of one thread's group of four components; M = 18840: the tables no longer fit LDS (the form with five
    launches through scratch, see the hub test below)."""
    B, L = 3, 70
    g = torch.Generator().manual_seed(100 * K + U)
    x, go = _signed((B, M, U), g), _signed((B, L, K, U), g)
    idx = torch.randint(0, M, (B, L, K), generator=g)
    out = ops.knn_gather_fwd(x.cuda(), idx.cuda(), out=_nan(B, L, K, U))
    assert _same(out, R.knn_gather(x.numpy(), idx.numpy()))
    want = R.knn_gather_grad(go.numpy(), idx.numpy(), M)
    gx = ops.knn_gather_grad(go.cuda(), idx.cuda(), M, out=_nan(B, M, U))
    assert _same(gx, want)
    # ... and through the operator: the same values forward (torch.gather's), the same bits backward
    xg = x.cuda().requires_grad_()
    o2 = ops.knn_gather(xg, idx.cuda())
    b, l, k = idx.shape
    assert torch.equal(o2.detach(), torch.gather(x.cuda(), 1, idx.cuda().reshape(b, l * k, 1).expand(b, l * k, U)).view(b, l, k, U))
    o2.backward(go.cuda())
    assert _same(xg.grad, want)


@pytest.mark.parametrize("M", [20, 18839, 18840])
def test_gather_gradient_hub_exact_wavefront_and_untouched_rows(ops, M):
    """Instance 0: index 7 receives all 1500 entries (longer than a wavefront, longer than one LDS tile of the sort);
    instance 1: one row receives exactly 64 entries, one exactly 65, index 7 the other 1371; nobody else receives anything
    and reads exactly +0.0.  M = 18839 is the last size whose tables (2 M + 2 E + E / 65 + 2 ints, E = 1500) fit the
    160 KiB - 1 KiB of LDS of the one-launch form, M = 18840 the first that takes the five launches through scratch."""
    B, L, K, U = 2, 300, 5, 3
    g = torch.Generator().manual_seed(7)
    idx = torch.full((B, L * K), 7, dtype=torch.int64)
    perm = torch.randperm(L * K, generator=g)
    idx[1, perm[:64]] = 3
    idx[1, perm[64:129]] = 11
    idx = idx.view(B, L, K)
    go = _signed((B, L, K, U), g)
    want = R.knn_gather_grad(go.numpy(), idx.numpy(), M)
    gx = ops.knn_gather_grad(go.cuda(), idx.cuda(), M, out=_nan(B, M, U))
    assert _same(gx, want)
    quiet = np.ones((B, M), dtype=bool)
    quiet[:, 7] = False
    quiet[1, 3] = quiet[1, 11] = False
    assert (_bits(gx)[quiet] == 0).all()          # +0.0: not a bit set
    x = _signed((B, M, U), g)
    assert _same(ops.knn_gather_fwd(x.cuda(), idx.cuda(), out=_nan(B, L, K, U)), R.knn_gather(x.numpy(), idx.numpy()))


# ------------------------------------------------------------------------------------------------ knn_points' gradient
def _clouds(b, n1, n2, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(b, n1, 3, generator=g) * 2 - 1).float(), (torch.rand(b, n2, 3, generator=g) * 2 - 1).float(), g


@pytest.fixture(scope="module")
def search_case(ops):
    """B=3, n1=70, n2=45, K=5 through the real search, with its reference: shared by the tests below, never modified."""
    p1, p2, g = _clouds(3, 70, 45, 21)
    w = (torch.rand(3, 70, 5, generator=g) + 0.5).float()
    idx = ops.knn_points(p1.cuda(), p2.cuda(), K=5).idx
    g1, g2 = R.knn_points_grad(p1.numpy(), p2.numpy(), idx.cpu().numpy(), w.numpy())
    return p1.cuda(), p2.cuda(), idx, w.cuda(), g1, g2


@pytest.mark.parametrize("b,n1,n2,K", [(3, 70, 45, 1), (3, 70, 45, 5), (3, 64, 64, 17), (1, 2048, 2048, 17)])
def test_points_gradient_through_the_search(ops, b, n1, n2, K):
    p1, p2, g = _clouds(b, n1, n2, 1000 + n1 + K)
    w = (torch.rand(b, n1, K, generator=g) + 0.5).float()
    a, r = p1.cuda().requires_grad_(), p2.cuda().requires_grad_()
    res = ops.knn_points(a, r, K=K)
    (res.dists * w.cuda()).sum().backward()
    g1, g2 = R.knn_points_grad(p1.numpy(), p2.numpy(), res.idx.cpu().numpy(), w.numpy())
    assert _same(a.grad, g1) and _same(r.grad, g2)
    # the C entry itself, outputs pre-filled with NaN
    o1, o2 = ops.knn_points_grad(p1.cuda(), p2.cuda(), res.idx, w.cuda(), out=(_nan(b, n1, 3), _nan(b, n2, 3)))
    assert _same(o1, g1) and _same(o2, g2)


def test_points_gradient_self_case_adds_both_halves(ops):
    p, _, g = _clouds(2, 64, 1, 5)
    w = (torch.rand(2, 64, 17, generator=g) + 0.5).float()
    x = p.cuda().requires_grad_()
    res = ops.knn_points(x, x, K=17)
    (res.dists * w.cuda()).sum().backward()
    g1, g2 = R.knn_points_grad(p.numpy(), p.numpy(), res.idx.cpu().numpy(), w.numpy())
    assert _same(x.grad, g1 + g2)


def test_points_gradient_hub_by_construction(ops):
    """1500 queries within 1e-3 of p2[7], every other point of p2 further than 1 away, K=1: every entry lands on index 7."""
    g = torch.Generator().manual_seed(9)
    p2 = (torch.rand(1, 20, 3, generator=g) * 0.4 - 0.2 + torch.tensor([3.0, 0.0, 0.0])).float()
    p2[0, 7] = torch.tensor([0.25, -0.5, 0.75])
    p1 = (p2[:, 7:8] + (torch.rand(1, 1500, 3, generator=g) * 2 - 1) * 5e-4).float()
    w = (torch.rand(1, 1500, 1, generator=g) + 0.5).float()
    a, r = p1.cuda().requires_grad_(), p2.cuda().requires_grad_()
    res = ops.knn_points(a, r, K=1)
    assert bool((res.idx == 7).all())
    (res.dists * w.cuda()).sum().backward()
    g1, g2 = R.knn_points_grad(p1.numpy(), p2.numpy(), res.idx.cpu().numpy(), w.numpy())
    assert _same(a.grad, g1) and _same(r.grad, g2)
    assert (np.delete(_bits(r.grad)[0], 7, 0) == 0).all()


def test_points_gradient_one_output_only(ops, search_case):
    p1, p2, idx, w, g1, g2 = search_case
    o1, none2 = ops.knn_points_grad(p1, p2, idx, w, want2=False, out=(_nan(3, 70, 3), None))
    none1, o2 = ops.knn_points_grad(p1, p2, idx, w, want1=False, out=(None, _nan(3, 45, 3)))
    assert none1 is None and none2 is None and _same(o1, g1) and _same(o2, g2)


# ------------------------------------------------------------------------------------------------ reproducibility
def test_backward_passes_repeat_and_do_not_depend_on_the_batch(ops, search_case):
    p1, p2, idx, w, g1, g2 = search_case
    g = torch.Generator().manual_seed(2)
    go = _signed((3, 70, 5, 3), g).cuda()
    gx_ref = R.knn_gather_grad(go.cpu().numpy(), idx.cpu().numpy(), 45)
    for _ in range(5):
        o1, o2 = ops.knn_points_grad(p1, p2, idx, w, out=(_nan(3, 70, 3), _nan(3, 45, 3)))
        assert _same(o1, g1) and _same(o2, g2)
        assert _same(ops.knn_gather_grad(go, idx, 45, out=_nan(3, 45, 3)), gx_ref)
    one = lambda t: t[1:2].contiguous()
    five = lambda t: t[1:2].expand(5, *t.shape[1:]).contiguous()
    for sel, rows in ((one, (0,)), (five, (2, 4))):
        o1, o2 = ops.knn_points_grad(sel(p1), sel(p2), sel(idx), sel(w), out=(_nan(len(sel(p1)), 70, 3), _nan(len(sel(p1)), 45, 3)))
        ox = ops.knn_gather_grad(sel(go), sel(idx), 45, out=_nan(len(sel(p1)), 45, 3))
        for row in rows:     # (beside two unrelated clouds: instance 1 of the batch of three above)
            assert _same(o1[row], g1[1]) and _same(o2[row], g2[1]) and _same(ox[row], gx_ref[1])


# ------------------------------------------------------------------------------------------------ wrapper and errors
def test_return_nn_is_the_gather_and_carries_the_gradient(ops, search_case):
    p1, p2, idx, w, _, _ = search_case
    r = p2.clone().requires_grad_()
    res = ops.knn_points(p1, r, K=5, return_nn=True)
    assert res.knn.shape == (3, 70, 5, 3) and torch.equal(res.idx, idx)
    assert torch.equal(res.knn.detach(), ops.knn_gather(p2, idx))
    go = _signed((3, 70, 5, 3), torch.Generator().manual_seed(4))
    res.knn.backward(go.cuda())
    assert _same(r.grad, R.knn_gather_grad(go.numpy(), idx.cpu().numpy(), 45))
    assert ops.knn_points(p1, p2, K=5).knn is None
    full = torch.full((3,), 45, device="cuda")
    assert torch.equal(ops.knn_points(p1, p2, K=5, lengths1=None, lengths2=full).idx, idx)


def test_ragged_lengths_are_refused(ops, search_case):
    from geoa3_amd._lib import Geoa3Error
    p1, p2 = search_case[0], search_case[1]
    with pytest.raises(Geoa3Error, match="lengths2"):
        ops.knn_points(p1, p2, K=5, lengths2=torch.tensor([45, 44, 45], device="cuda"))
    with pytest.raises(Geoa3Error, match="lengths1"):
        ops.knn_points(p1, p2, K=5, lengths1=[70, 70, 12])


def test_index_out_of_range_is_nan_forward_and_dropped_backward(ops):
    """An index equal to M (and a negative one) is never dereferenced: NaN in that element of the gather, no term in the
    sums; the neighbouring elements and the memory around the outputs (and the scratch) stay as they were."""
    B, M, L, K, U = 2, 45, 70, 5, 3
    g = torch.Generator().manual_seed(31)
    x, go = _signed((B, M, U), g), _signed((B, L, K, U), g)
    idx = torch.randint(0, M, (B, L, K), generator=g)
    idx[1, 69, 4] = M          # the last entry of the batch: a wrapped read would leave the buffer
    idx[0, 3, 2] = -1
    idx[0, 0, 0] = 1 << 40
    out, out_ok = _guarded((B, L, K, U))
    ops.knn_gather_fwd(x.cuda(), idx.cuda(), out=out)
    want = R.knn_gather(x.numpy(), idx.numpy())
    assert np.isnan(want).sum() == 3 * U and _same(out, want) and out_ok()
    gx, gx_ok = _guarded((B, M, U))
    nbytes = ops.knn_scatter_scratch(B, L * K, M, "cuda").numel()
    sbuf = torch.full((256 + nbytes + 256,), 0x5A, device="cuda", dtype=torch.uint8)
    ops.knn_gather_grad(go.cuda(), idx.cuda(), M, scratch=sbuf[256:256 + nbytes], out=gx)
    assert _same(gx, R.knn_gather_grad(go.numpy(), idx.numpy(), M)) and gx_ok()
    assert bool((sbuf[:256] == 0x5A).all() and (sbuf[256 + nbytes:] == 0x5A).all())
    # knn_points' gradient with the same table: the three terms are in neither sum
    p1, p2 = _signed((B, L, 3), g), _signed((B, M, 3), g)
    w = (torch.rand(B, L, K, generator=g) + 0.5).float()
    o1, ok1 = _guarded((B, L, 3))
    o2, ok2 = _guarded((B, M, 3))
    sbuf.fill_(0x5A)
    ops.knn_points_grad(p1.cuda(), p2.cuda(), idx.cuda(), w.cuda(), scratch=sbuf[256:256 + nbytes], out=(o1, o2))
    g1, g2 = R.knn_points_grad(p1.numpy(), p2.numpy(), idx.numpy(), w.numpy())
    assert _same(o1, g1) and _same(o2, g2) and ok1() and ok2()
    assert bool((sbuf[:256] == 0x5A).all() and (sbuf[256 + nbytes:] == 0x5A).all())


def test_sizes_out_of_range_are_refused(ops):
    from geoa3_amd import _lib
    lib = _lib.load()
    assert lib.geoa3_knn_scatter_scratch_bytes(1 << 16, 1 << 15, 8) < 0      # B E = 2^31
    assert lib.geoa3_knn_scatter_scratch_bytes(0, 8, 8) < 0 and lib.geoa3_knn_scatter_scratch_bytes(2, 0, 8) < 0
    assert lib.geoa3_knn_scatter_scratch_bytes(250, 1024 * 17, 1024) == 4 * 250 * (1025 + 1024 + 2 * 1024 * 17)
    x = torch.zeros(1, 4, 3, device="cuda")
    idx = torch.zeros(1, 4, 2, device="cuda", dtype=torch.int64)
    out = torch.zeros(1, 4, 2, 3, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert lib.geoa3_knn_gather(x.data_ptr(), idx.data_ptr(), 1, 4, 4, 0, 3, out.data_ptr(), s) == -1            # K = 0
    assert lib.geoa3_knn_gather(x.data_ptr(), idx.data_ptr(), 1, 4, 4, 2, 0, out.data_ptr(), s) == -1            # U = 0
    assert lib.geoa3_knn_gather(x.data_ptr(), idx.data_ptr(), 1 << 16, 4, 1 << 14, 2, 3, out.data_ptr(), s) == _lib.ENOSUPPORT
    assert lib.geoa3_knn_points_grad(x.data_ptr(), x.data_ptr(), idx.data_ptr(), out.data_ptr(), 1, 4, 4, 2, None, None,
                                     None, s) == -1                                                              # no output


def test_other_tensors_keep_the_torch_expression(ops):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 9, 4, generator=g, dtype=torch.float64)
    idx = torch.randint(0, 9, (2, 5, 3), generator=g)
    want = torch.gather(x, 1, idx.reshape(2, 15, 1).expand(2, 15, 4)).view(2, 5, 3, 4)
    assert torch.equal(ops.knn_gather(x, idx), want)                                   # CPU float64
    got = ops.knn_gather(x.cuda(), idx.cuda())                                          # device float64
    assert got.dtype == torch.float64 and torch.equal(got.cpu(), want)


def test_second_derivative_raises(ops, search_case):
    p1, p2, idx, w, _, _ = search_case
    a = p1.clone().requires_grad_()
    (g,) = torch.autograd.grad((ops.knn_points(a, p2, K=5).dists * w).sum(), a, create_graph=True)
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="no derivative of its own"):
        torch.autograd.grad(g.sum(), a)
    x = p2.clone().requires_grad_()
    (g,) = torch.autograd.grad((ops.knn_gather(x, idx) ** 2).sum(), x, create_graph=True)
    assert g.requires_grad
    with pytest.raises(RuntimeError, match="no derivative of its own"):
        torch.autograd.grad(g.sum(), x)


# ------------------------------------------------------------------------------------------------ torch.compile
def test_kappa_adv_composition_compiles_whole_and_equals_eager(ops):
    """The reference's _get_kappa_adv (Lib/loss_utils.py:64-82) written on the two operators, and a term through `dists`:
    torch.compile(fullgraph=True) == eager bit for bit, values and gradient."""
    from oracle import geoa3_oracle as O
    ori, nrm = O.make_synthetic_clouds(3, 96, 5)
    adv0 = (ori + 0.01 * torch.randn(3, 3, 96, generator=torch.Generator().manual_seed(6))).cuda()
    ori, nrm = ori.cuda(), nrm.cuda()

    def kappa_adv(adv, k=4):
        pts = adv.permute(0, 2, 1)
        near = ops.knn_points(pts, ori.permute(0, 2, 1), K=1)
        normal = ops.knn_gather(nrm.permute(0, 2, 1), near.idx).permute(0, 3, 1, 2).squeeze(3).contiguous()
        own = ops.knn_points(pts, pts, K=k + 1)
        nn_pts = ops.knn_gather(pts, own.idx).permute(0, 3, 1, 2)[:, :, :, 1:].contiguous()
        v = nn_pts - adv.unsqueeze(3)
        v = v / v.norm(2, 1, keepdim=True).clamp(min=1e-12)
        return torch.abs((v * normal.unsqueeze(3)).sum(1)).mean(2), near.dists.sum((1, 2)) + own.dists.sum((1, 2))

    res = []
    for fn in (kappa_adv, torch.compile(kappa_adv, fullgraph=True, backend="aot_eager")):
        adv = adv0.clone().requires_grad_()
        kap, dsum = fn(adv)
        (gk,) = torch.autograd.grad(kap.sum(), adv, retain_graph=True)
        (gd,) = torch.autograd.grad(dsum.sum(), adv)
        res.append((kap.detach(), dsum.detach(), gk, gd))
    for e, c in zip(*res):
        assert _same(e, c)
    assert bool(res[0][2].abs().sum() > 0) and bool(res[0][3].abs().sum() > 0)
    want, _ = O.get_kappa_adv(adv0.cpu(), ori.cpu(), nrm.cpu(), 4)
    np.testing.assert_allclose(res[0][0].cpu().numpy(), want.numpy(), rtol=2e-5, atol=1e-6)
