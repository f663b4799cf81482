"""CPU-only.  (1) The float32 restatement of the knn_gather / knn_points backward formulas (tests/_knn_ops_ref.py, what
tests/test_gpu_knn_ops.py holds the kernels to bit for bit) against float64 autograd through the oracle's knn_points /
knn_gather on the same indices.  The bound is derived, not tuned: a term t = fl(fl(2 gd) fl(p1 - p2)) carries at most three
roundings, a sequential sum of c terms c - 1 more, so with u = 2^-24

    |ref32 - ref64| <= ((1 + u)^(c + 2) - 1) sum|t| <= (c + 3) u sum|t|        (c + 2 <= 4096)

per output element, sum|t| the float64 sum of the absolute values of the c terms behind it; the pure gather gradient has
no rounding inside a term: c u sum|g|.  One dropped term must move its element by more than that bound, or the pin would
see nothing.  (2) The registered ops trace: knn_points(return_nn=True) + knn_gather and their gradient are ONE FX graph
under FakeTensorMode with geoa3::knn_gather, geoa3::knn_gather_grad and geoa3::knn_points_grad as nodes."""
import numpy as np
import pytest
import torch

from oracle import geoa3_oracle as O
from tests import _knn_ops_ref as R

U24 = 2.0 ** -24


def _points_case(seed, b, n1, n2, K, hub=False):
    g = torch.Generator().manual_seed(seed)
    p2 = torch.rand(b, n2, 3, generator=g) * 2 - 1
    if hub:        # every query within 1e-3 of p2[:, 7], every other point of p2 further than 1 away
        p2 = p2 * 0.2 + torch.tensor([3.0, 0.0, 0.0])
        p2[:, 7] = torch.tensor([0.25, -0.5, 0.75])
        p1 = p2[:, 7:8] + (torch.rand(b, n1, 3, generator=g) * 2 - 1) * 5e-4
    else:
        p1 = torch.rand(b, n1, 3, generator=g) * 2 - 1
    gd = torch.rand(b, n1, K, generator=g) + 0.5
    return p1.float(), p2.float(), gd.float()


def _points_64(p1, p2, gd, K):
    """float64 autograd through the oracle's search: the indices, d p1, d p2 and, per output element, the number of terms
    and the float64 sum of their absolute values."""
    a, r = p1.double().requires_grad_(), p2.double().requires_grad_()
    d, idx = O.knn_points(a, r, K)
    g1, g2 = torch.autograd.grad((d * gd.double()).sum(), (a, r))
    nb = O.knn_gather(r.detach(), idx)                                        # [b,n1,K,3]
    t = (2.0 * gd.double()).unsqueeze(-1) * (a.detach().unsqueeze(2) - nb)    # the terms in float64
    b, n1, _ = idx.shape
    n2 = p2.shape[1]
    flat = idx.reshape(b, n1 * K, 1).expand(b, n1 * K, 3)
    abs1, cnt1 = t.abs().sum(2), torch.full((b, n1, 3), float(K), dtype=torch.float64)
    abs2 = torch.zeros(b, n2, 3, dtype=torch.float64).scatter_add(1, flat, t.abs().reshape(b, n1 * K, 3))
    cnt2 = torch.zeros(b, n2, 3, dtype=torch.float64).scatter_add(1, flat, torch.ones(b, n1 * K, 3, dtype=torch.float64))
    return idx, (g1.numpy(), g2.numpy()), ((cnt1 + 3) * U24 * abs1).numpy(), ((cnt2 + 3) * U24 * abs2).numpy(), t.numpy()


@pytest.mark.parametrize("shape", [(2, 40, 25, 4), (2, 33, 33, 1), (1, 150, 20, 1, True)], ids=["k4", "k1", "hub"])
def test_points_grad_restatement_against_float64_autograd(shape):
    b, n1, n2, K = shape[:4]
    hub = len(shape) > 4
    p1, p2, gd = _points_case(17 + K, b, n1, n2, K, hub)
    idx, (g1_64, g2_64), bound1, bound2, t64 = _points_64(p1, p2, gd, K)
    idx = idx.numpy()
    if hub:
        assert (idx == 7).all()
    g1, g2 = R.knn_points_grad(p1.numpy(), p2.numpy(), idx, gd.numpy())
    assert g1.dtype == np.float32 and g2.dtype == np.float32
    e1, e2 = np.abs(g1.astype(np.float64) - g1_64), np.abs(g2.astype(np.float64) - g2_64)
    print("points grad %s: max err/bound g1 %.3f g2 %.3f" % (shape, (e1 / np.maximum(bound1, 1e-300)).max(),
                                                              (e2 / np.maximum(bound2, 1e-300)).max()))
    assert (e1 <= bound1).all() and (e2 <= bound2).all()
    # a destination nobody points at is exactly +0.0
    nobody = np.ones((b, n2), dtype=bool)
    nobody[np.arange(b)[:, None], idx.reshape(b, -1)] = False
    assert nobody.any() and not g2[nobody].any() and not np.signbit(g2[nobody]).any()
    # one dropped term is seen: a row's last k (g1), the first and the last entry of the longest segment (g2)
    counts = np.bincount(idx[0].reshape(-1), minlength=n2)
    j = int(counts.argmax())
    entries = np.nonzero(idx[0].reshape(-1) == j)[0]
    assert len(entries) >= 2
    for e in (int(entries[0]), int(entries[-1])):
        d1, d2 = R.knn_points_grad(p1.numpy(), p2.numpy(), idx, gd.numpy(), drop={(0, e)})
        assert (np.abs(d2[0, j].astype(np.float64) - g2_64[0, j]) > bound2[0, j]).any()
        assert np.array_equal(np.delete(d2[0], j, 0), np.delete(g2[0], j, 0))       # ... and only there
    i = n1 - 1
    d1, _ = R.knn_points_grad(p1.numpy(), p2.numpy(), idx, gd.numpy(), drop={(0, i * K + K - 1)})
    assert (np.abs(d1[0, i].astype(np.float64) - g1_64[0, i]) > bound1[0, i]).any()
    assert np.array_equal(d1[0, :i], g1[0, :i])


def test_gather_grad_restatement_against_float64_autograd():
    b, m, l, K, u = 2, 30, 50, 4, 5
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, m, (b, l, K), generator=g)
    idx[0, :40] = 7                      # a hub: 160 entries; destination 8 gets none
    idx[idx == 8] = 9
    x = (torch.rand(b, m, u, generator=g) * 2 - 1).float()
    go = (torch.rand(b, l, K, u, generator=g) + 0.5).float() * torch.where(torch.rand(b, l, K, u, generator=g) < 0.5, -1.0, 1.0)
    out = R.knn_gather(x.numpy(), idx.numpy())
    assert np.array_equal(out, O.knn_gather(x, idx).numpy())
    x64 = x.double().requires_grad_()
    (g64,) = torch.autograd.grad((O.knn_gather(x64, idx) * go.double()).sum(), x64)
    flat = idx.reshape(b, l * K, 1).expand(b, l * K, u)
    sabs = torch.zeros(b, m, u, dtype=torch.float64).scatter_add(1, flat, go.double().abs().reshape(b, l * K, u))
    cnt = torch.zeros(b, m, u, dtype=torch.float64).scatter_add(1, flat, torch.ones(b, l * K, u, dtype=torch.float64))
    bound = (cnt * U24 * sabs).numpy()
    gx = R.knn_gather_grad(go.numpy(), idx.numpy(), m)
    err = np.abs(gx.astype(np.float64) - g64.numpy())
    print("gather grad: max err/bound %.3f" % (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all()
    assert not gx[:, 8].any() and not np.signbit(gx[:, 8]).any()
    entries = np.nonzero(idx[0].reshape(-1).numpy() == 7)[0]
    assert len(entries) >= 160
    for e in (int(entries[0]), int(entries[-1])):      # the first entry of the segment, the hub's last entry
        dx = R.knn_gather_grad(go.numpy(), idx.numpy(), m, drop={(0, e)})
        assert (np.abs(dx[0, 7].astype(np.float64) - g64.numpy()[0, 7]) > bound[0, 7]).all()
        assert np.array_equal(np.delete(dx[0], 7, 0), np.delete(gx[0], 7, 0))
    # an index outside [0, m): NaN in the gather, no term in the sum
    bad = idx.clone()
    bad[1, 3, 2] = m
    bad[1, 4, 0] = -1
    ob = R.knn_gather(x.numpy(), bad.numpy())
    assert np.isnan(ob[1, 3, 2]).all() and np.isnan(ob[1, 4, 0]).all() and np.isnan(ob).sum() == 2 * u
    assert np.array_equal(R.knn_gather_grad(go.numpy(), bad.numpy(), m),
                          R.knn_gather_grad(go.numpy(), idx.numpy(), m, drop={(1, 3 * K + 2), (1, 4 * K)}))


def test_operators_and_their_gradient_trace_as_one_graph():
    """FakeTensorMode + make_fx of knn_points(return_nn=True), knn_gather and the gradient of both.  The fake tensors are
    CPU ones: without a device the autograd engine refuses to run a backward over device tensors, fake or not (with a
    device: torch.compile(fullgraph=True) in tests/test_gpu_knn_ops.py).  knn_points and its `.knn` are the library's ops
    on fake tensors of any device; the bare knn_gather wrapper keeps torch.gather for whatever is not a device tensor, so
    that call shows as aten.gather in the same graph."""
    from torch._subclasses import FakeTensorMode
    from torch.fx.experimental.proxy_tensor import make_fx
    from geoa3_amd import library, ops  # noqa: F401

    for name in ("knn_gather", "knn_gather_grad", "knn_points_grad"):
        assert str(getattr(torch.ops.geoa3, name).default._schema).startswith("geoa3::" + name + "(")

    def f(p1, p2, feat):
        r = ops.knn_points(p1, p2, K=3, return_nn=True)
        nb = torch.ops.geoa3.knn_gather(feat, r.idx)
        nb2 = ops.knn_gather(feat, r.idx)
        loss = (r.dists * 0.5).sum() + (r.knn ** 2).sum() + (nb ** 2).sum() + nb2.sum()
        return (r.knn, nb) + torch.autograd.grad(loss, (p1, p2, feat))

    with FakeTensorMode():
        p1 = torch.empty(2, 50, 3, requires_grad=True)
        p2 = torch.empty(2, 40, 3, requires_grad=True)
        feat = torch.empty(2, 40, 7, requires_grad=True)
        gm = make_fx(f, tracing_mode="real")(p1, p2, feat)
        knn, nb, g1, g2, gf = f(p1, p2, feat)
    assert knn.shape == (2, 50, 3, 3) and nb.shape == (2, 50, 3, 7) and knn.dtype == torch.float32
    assert g1.shape == (2, 50, 3) and g2.shape == (2, 40, 3) and gf.shape == (2, 40, 7) and gf.dtype == torch.float32
    nodes = {}
    for n in gm.graph.nodes:
        if n.op == "call_function" and "geoa3" in str(n.target):
            nodes.setdefault(str(n.target).split(".")[1], []).append(n)
    assert set(nodes) == {"knn_points", "knn_gather", "knn_gather_grad", "knn_points_grad"}, sorted(nodes)
    assert len(nodes["knn_gather"]) == 2 and len(nodes["knn_gather_grad"]) == 2 and len(nodes["knn_points_grad"]) == 1
    assert any("aten.gather" in str(n.target) for n in gm.graph.nodes)
    shapes = lambda n: [(tuple(v.shape), v.dtype) for v in (n.meta["val"] if isinstance(n.meta["val"], (tuple, list))
                                                            else [n.meta["val"]])]
    f32 = torch.float32
    assert sorted(shapes(n)[0] for n in nodes["knn_gather"]) == [((2, 50, 3, 3), f32), ((2, 50, 3, 7), f32)]
    assert sorted(shapes(n)[0] for n in nodes["knn_gather_grad"]) == [((2, 40, 3), f32), ((2, 40, 7), f32)]
    assert shapes(nodes["knn_points_grad"][0]) == [((2, 50, 3), f32), ((2, 40, 3), f32)]
    assert shapes(nodes["knn_points"][0]) == [((2, 50, 3), f32), ((2, 50, 3), torch.int64)]


def test_wrapper_keeps_the_torch_expression_off_the_device_and_refuses_lengths():
    from geoa3_amd import ops
    from geoa3_amd._lib import Geoa3Error
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 9, 4, generator=g, dtype=torch.float64, requires_grad=True)
    idx = torch.randint(0, 9, (2, 5, 3), generator=g)
    out = ops.knn_gather(x, idx)
    assert out.dtype == torch.float64 and torch.equal(out, O.knn_gather(x, idx))
    (gx,) = torch.autograd.grad(out.sum(), x)
    assert gx.shape == x.shape
    with pytest.raises(Geoa3Error, match="lengths2"):
        ops.knn_points(torch.zeros(2, 6, 3), torch.zeros(2, 9, 3), K=1, lengths2=torch.tensor([9, 4]))
    with pytest.raises(Geoa3Error, match="lengths1"):
        ops.knn_points(torch.zeros(2, 6, 3), torch.zeros(2, 9, 3), K=1, lengths1=torch.tensor([5, 6]))


def test_second_derivative_raises_instead_of_returning_zeros():
    """The two gradient ops have no derivative of their own: differentiating the result of a create_graph=True backward
    raises (fake tensors: the formula is registered for every device, nothing runs)."""
    from torch._subclasses import FakeTensorMode
    from geoa3_amd import library, ops  # noqa: F401
    with FakeTensorMode():
        a = torch.empty(2, 10, 3, requires_grad=True)
        r = torch.empty(2, 8, 3, requires_grad=True)
        res = ops.knn_points(a, r, K=2, return_nn=True)
        (g,) = torch.autograd.grad(res.dists.sum(), a, create_graph=True)
        assert g.requires_grad
        with pytest.raises(RuntimeError, match="knn_points_grad.*no derivative of its own"):
            torch.autograd.grad(g.sum(), a)
        (g,) = torch.autograd.grad((res.knn ** 2).sum(), r, create_graph=True)
        assert g.requires_grad
        with pytest.raises(RuntimeError, match="knn_gather_grad.*no derivative of its own"):
            torch.autograd.grad(g.sum(), r)
