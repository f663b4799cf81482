"""The geometric objective (Lib/loss_utils.py:25-97 as combined by Attacker/geoA3_attack.py:131-166) restated in float64
FROM THE TABLES the kernels consume -- i_ao, i_oa (nearest points), knn_adv (self K-NN of the iterate) -- with torch
autograd for the gradient: O(N k) instead of the oracle's dense N x N distance matrices, which take minutes at 4096
points and cannot serve at 8192.  tests/test_geo_table_ref.py pins it to the oracle's dense formulation."""
import torch


def _take(x, idx):
    """x [B,C,M], idx [B,L] -> [B,C,L]"""
    return torch.gather(x, 2, idx.long().unsqueeze(1).expand(-1, x.shape[1], -1))


def kappa_adv(a, nrm, i_ao, knn_adv):
    """_get_kappa_adv from the tables: a [B,3,N] float64, nrm [B,3,Nr], i_ao [B,N], knn_adv [B,N,k+1] (column 0 dropped)."""
    B, _, N = a.shape
    nb = knn_adv[:, :, 1:]
    k = nb.shape[2]
    q = _take(a, nb.reshape(B, N * k)).view(B, 3, N, k)
    v = q - a.unsqueeze(3)
    u = v / v.norm(2, 1, keepdim=True).clamp(min=1e-12)
    n = _take(nrm, i_ao)
    return (u * n.unsqueeze(3)).sum(1).abs().mean(2)


def objective(adv, ori, *, normal_ori=None, kappa_ori=None, i_ao=None, i_oa=None, knn_adv=None, hd_arg=None, dis_type=1,
              single_side=False, w_dis=1.0, w_hd=0.0, w_curv=0.0, dkappa=None):
    """-> dict of float64 CPU tensors: dis_loss, hd_loss, curv_loss, constrain [B], kappa_adv [B,N] (with a table) and grad
    [B,3,N] = d constrain / d adv (with dkappa: d (sum dkappa . kappa_adv) / d adv added, as geoa3_geo_args.dkappa).
    hd_arg [B]: the point whose d_ao is the Hausdorff distance -- taken by the caller from the fp32 distances, so that
    both sides differentiate the same point."""
    f = lambda t: None if t is None else t.detach().cpu().double()
    ix = lambda t: None if t is None else t.detach().cpu().long()
    a = f(adv).clone().requires_grad_()
    o, nrm, kori = f(ori), f(normal_ori), f(kappa_ori)
    i_ao, i_oa, knn_adv, hd_arg = ix(i_ao), ix(i_oa), ix(knn_adv), ix(hd_arg)
    B = a.shape[0]
    zero = torch.zeros(B, dtype=torch.float64)
    out = {}
    d_ao = ((a - _take(o, i_ao)) ** 2).sum(1) if i_ao is not None else None
    dis = zero
    if dis_type == 1:
        dis = d_ao.mean(1)
        if not single_side:
            dis = dis + ((o - _take(a, i_oa)) ** 2).sum(1).mean(1)
    elif dis_type == 2:
        dis = ((a - o) ** 2).sum(1).sum(1)
    hd = d_ao.gather(1, hd_arg.view(B, 1))[:, 0] if w_hd != 0.0 else zero
    curv, extra = zero, 0.0
    if knn_adv is not None and (w_curv != 0.0 or dkappa is not None):
        kap = kappa_adv(a, nrm, i_ao, knn_adv)
        out["kappa_adv"] = kap.detach()
        if dkappa is not None:
            extra = (f(dkappa) * kap).sum()
        else:
            curv = ((kap - kori.gather(1, i_ao)) ** 2).mean(1)
    con = (w_dis * dis if dis_type != 0 else zero) + w_hd * hd + w_curv * curv
    (g,) = torch.autograd.grad(con.sum() + extra, a)
    out.update(dis_loss=dis.detach(), hd_loss=hd.detach(), curv_loss=curv.detach(), constrain=con.detach(), grad=g)
    return out
