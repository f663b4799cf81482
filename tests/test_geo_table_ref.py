"""CPU-only: the float64 table form of the objective (tests/_geo_table_ref.py), which the GPU tests of clouds beyond 4096
points are held to, against the oracle's dense formulation (oracle/geoa3_oracle.py: N x N distance matrices, autograd)
with the oracle's own tables.  Inputs and bars as tests/test_gpu_geometry.py holds the kernels to the oracle."""
import numpy as np
import pytest
import torch

from oracle import geoa3_oracle as O

from tests import _geo_table_ref as T


@pytest.mark.parametrize("B,N,Nr,k", [(2, 600, 600, 16), (2, 500, 900, 32)])
def test_table_form_matches_the_dense_oracle(B, N, Nr, k):
    ori, nrm = O.make_synthetic_clouds(B, Nr, seed=N + k)
    g = torch.Generator().manual_seed(N)
    adv = ori[:, :, :N] + 0.02 * torch.randn(B, 3, N, generator=g)
    # the dense side
    a = adv.clone().requires_grad_()
    ka, _ = O.get_kappa_adv(a, ori, nrm, k)
    kori = O.get_kappa_ori(ori, nrm, k)
    con = O.chamfer_loss(a, ori) + 0.1 * O.hausdorff_loss(a, ori) + O.curvature_loss(a, ori, ka, kori)
    (want_g,) = torch.autograd.grad(con.sum(), a)
    # the tables, as the oracle's searches return them
    ap, op = adv.permute(0, 2, 1), ori.permute(0, 2, 1)
    d_ao, i_ao = O.knn_points(ap, op, 1)
    _, i_oa = O.knn_points(op, ap, 1)
    _, knn_adv = O.knn_points(ap, ap, k + 1)
    got = T.objective(adv, ori, normal_ori=nrm, kappa_ori=kori, i_ao=i_ao[:, :, 0], i_oa=i_oa[:, :, 0], knn_adv=knn_adv,
                      hd_arg=d_ao[:, :, 0].argmax(1), w_dis=1.0, w_hd=0.1, w_curv=1.0)
    print("constrain", got["constrain"].tolist(), con.tolist(), "max |dg|", float((got["grad"] - want_g.double()).abs().max()))
    np.testing.assert_allclose(got["constrain"].numpy(), con.detach().numpy(), rtol=5e-5, atol=1e-7)
    scale = max(want_g.abs().max().item(), 1.0)
    np.testing.assert_allclose(got["grad"].numpy(), want_g.numpy(), rtol=2e-4, atol=2e-6 * scale)
    np.testing.assert_allclose(got["kappa_adv"].numpy(), ka.detach().numpy(), rtol=2e-5, atol=2e-6)


def test_table_form_is_cheap_at_the_ceiling():
    """8192 points, k = 32: the shape the dense oracle cannot serve.  Random tables: only the cost and the shapes."""
    B, N, k = 1, 8192, 32
    g = torch.Generator().manual_seed(0)
    adv, ori, nrm = (torch.randn(B, 3, N, generator=g) for _ in range(3))
    ri = lambda *s: torch.randint(0, N, s, generator=g)
    got = T.objective(adv, ori, normal_ori=nrm, kappa_ori=torch.rand(B, N, generator=g), i_ao=ri(B, N), i_oa=ri(B, N),
                      knn_adv=ri(B, N, k + 1), hd_arg=ri(B), w_hd=0.1, w_curv=1.0)
    assert got["grad"].shape == (B, 3, N) and got["kappa_adv"].shape == (B, N) and torch.isfinite(got["grad"]).all()
