"""What of the DGCNN victim can be checked without a GPU: the command lines accept it, the module has the public model's
state_dict and refuses what it does not implement, the new operators trace on fake tensors, and the checkers of
tests/_knn_nd_ref.py / tests/_dgcnn_ref.py agree with themselves (float32 loops against float64 on data where float32 is
exact)."""
import numpy as np
import pytest
import torch

from tests import _dgcnn_ref as D
from tests import _knn_nd_ref as K


# state_dict() of the public classification model, in its order, written out: bn1..bn5 are registered at top level AND
# inside conv1..conv5 (as conv<i>.1), so they appear twice; linear1 has no bias; dp1 / dp2 hold nothing
PUBLIC_STATE_KEYS = [
    "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked",
    "bn2.weight", "bn2.bias", "bn2.running_mean", "bn2.running_var", "bn2.num_batches_tracked",
    "bn3.weight", "bn3.bias", "bn3.running_mean", "bn3.running_var", "bn3.num_batches_tracked",
    "bn4.weight", "bn4.bias", "bn4.running_mean", "bn4.running_var", "bn4.num_batches_tracked",
    "bn5.weight", "bn5.bias", "bn5.running_mean", "bn5.running_var", "bn5.num_batches_tracked",
    "conv1.0.weight",
    "conv1.1.weight", "conv1.1.bias", "conv1.1.running_mean", "conv1.1.running_var", "conv1.1.num_batches_tracked",
    "conv2.0.weight",
    "conv2.1.weight", "conv2.1.bias", "conv2.1.running_mean", "conv2.1.running_var", "conv2.1.num_batches_tracked",
    "conv3.0.weight",
    "conv3.1.weight", "conv3.1.bias", "conv3.1.running_mean", "conv3.1.running_var", "conv3.1.num_batches_tracked",
    "conv4.0.weight",
    "conv4.1.weight", "conv4.1.bias", "conv4.1.running_mean", "conv4.1.running_var", "conv4.1.num_batches_tracked",
    "conv5.0.weight",
    "conv5.1.weight", "conv5.1.bias", "conv5.1.running_mean", "conv5.1.running_var", "conv5.1.num_batches_tracked",
    "linear1.weight",
    "bn6.weight", "bn6.bias", "bn6.running_mean", "bn6.running_var", "bn6.num_batches_tracked",
    "linear2.weight", "linear2.bias",
    "bn7.weight", "bn7.bias", "bn7.running_mean", "bn7.running_var", "bn7.num_batches_tracked",
    "linear3.weight", "linear3.bias",
]


@pytest.mark.parametrize("script", ["main_attack", "defense"])
def test_parsers_accept_arch_dgcnn(script):
    import importlib
    mod = importlib.import_module(script)
    cfg = mod.build_parser().parse_args(["--arch", "DGCNN"])
    assert cfg.arch == "DGCNN"
    import main_attack
    from geoa3_amd.dgcnn import DGCNN
    assert "DGCNN" in main_attack.ARCHS
    net = main_attack.make_victim(cfg)
    assert isinstance(net, DGCNN) and net.classes == cfg.classes and net.k == 20
    cfg.arch = "PointNet3"
    with pytest.raises(AssertionError, match="Not support such arch"):
        main_attack.make_victim(cfg)


def test_module_has_the_public_state_dict_and_refuses_training_and_cpu():
    from geoa3_amd.dgcnn import DGCNN, checkpoint_state_dict
    net = DGCNN(emb_dims=64, output_channels=10)
    assert list(net.state_dict().keys()) == PUBLIC_STATE_KEYS
    assert net.conv1[1] is net.bn1 and net.conv5[1] is net.bn5          # registered twice, one module
    assert tuple(net.conv4[0].weight.shape) == (256, 256, 1, 1) and tuple(net.linear1.weight.shape) == (512, 128)
    sd = net.state_dict()
    for wrapped in ({"state_dict": sd}, {"model_state_dict": sd, "epoch": 3}, sd, {"module." + k: v for k, v in sd.items()},
                    {"state_dict": {"module." + k: v for k, v in sd.items()}}):
        assert list(checkpoint_state_dict(wrapped).keys()) == PUBLIC_STATE_KEYS
    with pytest.raises(NotImplementedError):
        net.train()(torch.zeros(1, 3, 32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.eval()(torch.zeros(1, 3, 32))


@pytest.mark.parametrize("layout", ["state_dict", "model_state_dict", "bare", "module_prefix"])
def test_load_checkpoint_reads_every_layout_of_a_dgcnn_file(tmp_path, layout):
    import main_attack
    from geoa3_amd.dgcnn import DGCNN
    torch.manual_seed(1)
    sd = DGCNN(emb_dims=64).state_dict()
    obj = {"state_dict": {"state_dict": sd}, "model_state_dict": {"model_state_dict": sd, "epoch": 3}, "bare": sd,
           "module_prefix": {"state_dict": {"module." + k: v for k, v in sd.items()}}}[layout]
    path = str(tmp_path / "model_best.pth.tar")
    torch.save(obj, path)
    cfg = main_attack.build_parser().parse_args(["--arch", "DGCNN"])
    torch.manual_seed(2)
    net = DGCNN(emb_dims=64)
    main_attack.load_checkpoint(net, cfg, path)
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())


def test_new_operators_trace_on_fake_tensors():
    from torch._subclasses import FakeTensorMode
    from geoa3_amd import library, ops  # noqa: F401
    with FakeTensorMode():
        p = torch.empty(2, 50, 64)
        out = ops.knn_points(p, p, K=20, return_nn=True)
        assert tuple(out.dists.shape) == (2, 50, 20) and out.idx.dtype == torch.int64 and tuple(out.knn.shape) == (2, 50, 20, 64)
        y, arg = torch.ops.geoa3.edge_max(torch.empty(2, 50, 65), torch.empty(2, 50, 65), torch.empty(65), out.idx)
        assert tuple(y.shape) == (2, 65, 50) and tuple(arg.shape) == (2, 50, 65) and arg.dtype == torch.int32
        dU, dV = torch.ops.geoa3.edge_max_grad(y, y, arg, out.idx)
        assert tuple(dU.shape) == tuple(dV.shape) == (2, 50, 65)


# ------------------------------------------------------------------------------------------------ the checkers themselves
def test_knn_checker_float32_loop_equals_float64_on_integers():
    rng = np.random.default_rng(0)
    q = rng.integers(-3, 4, (2, 9, 5)).astype(np.float32)
    r = rng.integers(-3, 4, (2, 12, 5)).astype(np.float32)
    d32, i32 = K.knn_nd(q, r, 7)
    d64, i64 = K.knn_nd_f64(q, r, 7)
    assert np.array_equal(i32, i64) and np.array_equal(d32.astype(np.float64), d64)
    assert (np.diff(d32, axis=2) >= 0).all()
    tied = np.diff(d32, axis=2) == 0
    assert tied.any() and (np.diff(i32, axis=2)[tied] > 0).all()          # equal distances: ascending index


def test_knn_checker_orders_nan_as_inf_and_gradient_equals_autograd():
    q = np.array([[[0.0, 0.0], [np.nan, 1.0]]], np.float32)
    r = np.array([[[1.0, 0.0], [np.inf, 0.0], [0.0, 0.5]]], np.float32)
    d, i = K.knn_nd(q, r, 3)
    assert i.tolist() == [[[2, 0, 1], [0, 1, 2]]] and d[0, 0].tolist() == [0.25, 1.0, np.inf] and np.isinf(d[0, 1]).all()
    rng = np.random.default_rng(1)
    p1 = rng.integers(-2, 3, (1, 6, 4)).astype(np.float32)
    p2 = rng.integers(-2, 3, (1, 5, 4)).astype(np.float32)
    _, idx = K.knn_nd(p1, p2, 3)
    gd = rng.integers(1, 3, (1, 6, 3)).astype(np.float32)
    g1, g2 = K.knn_points_grad(p1, p2, idx, gd)
    a, b = torch.tensor(p1, dtype=torch.float64, requires_grad=True), torch.tensor(p2, dtype=torch.float64, requires_grad=True)
    nb = torch.gather(b, 1, torch.tensor(idx).reshape(1, -1, 1).expand(1, 18, 4)).view(1, 6, 3, 4)
    ((a.unsqueeze(2) - nb) ** 2).sum(-1).backward(torch.tensor(gd, dtype=torch.float64))
    assert np.array_equal(g1.astype(np.float64), a.grad.numpy()) and np.array_equal(g2.astype(np.float64), b.grad.numpy())


def test_edgeconv_checkers_agree_on_integers():
    """the float32 loops of edge_max / edge_max_grad on integer data (BatchNorm the identity, so every value is an exact
    small integer or a fifth of one) against the float64 standard formulation and its autograd"""
    g = torch.Generator().manual_seed(2)
    B, C, N, k, Co = 2, 3, 9, 4, 5
    x = torch.randint(-3, 4, (B, C, N), generator=g).double()
    w = torch.randint(-2, 3, (Co, 2 * C), generator=g).double()
    idx = torch.randint(0, N, (B, N, k), generator=g)
    one, zero = torch.ones(Co, dtype=torch.float64), torch.zeros(Co, dtype=torch.float64)
    eps = 2.0 ** -20                                                      # running_var + eps == 1 exactly
    ref = D.edgeconv_f64(x, idx, w, one, zero, zero, one - eps, eps=eps)
    xt = x.transpose(1, 2)
    U, V = xt @ w[:, :C].t(), xt @ (w[:, C:] - w[:, :C]).t()
    y, arg = D.edge_max(U.numpy(), V.numpy(), np.zeros(Co), idx.numpy())
    assert np.allclose(y.astype(np.float64), ref["y"].numpy(), rtol=2e-7, atol=0)
    sure = (ref["gap"] > 0).numpy()                                       # a unique best neighbour
    assert sure.mean() > 0.5 and np.array_equal(arg[sure], ref["arg"].numpy()[sure])
    go = torch.randint(1, 4, (B, Co, N), generator=g).double()
    dU, dV = D.edge_max_grad(go.numpy(), y, arg, idx.numpy())
    slope = np.where(y > 0, 1.0, 0.2)
    assert np.allclose(dV.astype(np.float64), (go.numpy() * slope).transpose(0, 2, 1), rtol=2e-7)
    # dU scattered to the chosen neighbour, dV kept at the point: together they are the gradient through U + V
    j = np.take_along_axis(idx.numpy(), arg.astype(np.int64), 2)          # [B,N,Co] the chosen point
    want = np.zeros_like(dU, dtype=np.float64)
    for b in range(B):
        for i in range(N):
            for c in range(Co):
                want[b, j[b, i, c], c] += dV[b, i, c]
    assert np.allclose(dU, want, rtol=1e-6)


def test_edge_max_checker_invalid_index_and_nan():
    U = np.array([[[1.0], [np.nan], [3.0]]], np.float32)
    V, t = np.zeros((1, 3, 1), np.float32), np.zeros(1, np.float32)
    idx = np.array([[[0, 2, 2], [0, 1, 2], [2, 3, 0]]])
    y, arg = D.edge_max(U, V, t, idx)
    assert arg[0, :, 0].tolist() == [1, 1, 1]               # first maximum; the NaN, once met, stays; the bad slot
    assert y[0, 0, 0] == 3.0 and np.isnan(y[0, 0, 1]) and np.isnan(y[0, 0, 2])
    dU, dV = D.edge_max_grad(np.ones((1, 1, 3), np.float32), y, arg, idx)
    assert dV[0, :, 0].tolist() == [1.0, np.float32(0.2), np.float32(0.2)]
    assert dU[0, :, 0].tolist() == [0.0, np.float32(0.2), 1.0]
