"""`torch.library` registration of the operator boundary (north_star "PyTorch-ROCm custom ops").

Every op of the `geoa3::` namespace has a schema, a CUDA(HIP) implementation that calls the C ABI through
`geoa3_amd.ops` (ctypes: the transport stays what it is), a fake (meta) kernel so that FakeTensor tracing --
`torch.compile`, `torch.export`, `make_fx` -- sees shapes and dtypes without running anything, and, where the reference
differentiates through it, a registered autograd formula.  `geoa3_amd.ops.knn_points` and the loss functions of
`geoa3_amd.loss_utils` are built on these ops, so a caller that keeps the reference's `_forward_step` composition
(Attacker/geoA3_attack.py:131-166) can put it under `torch.compile(fullgraph=True)` without a graph break.

    geoa3::nn1_pair        knn_points(K=1) both directions            Lib/loss_utils.py:32-33,41,48,70,92
    geoa3::knn             knn_points(K)                              Lib/loss_utils.py:57,77
    geoa3::knn_points      the pytorch3d operator itself ([b,n,D] arguments, 1 <= D <= 128, int64 idx, differentiable dists)
    geoa3::edge_max / _grad     the neighbour half of a fused eval-mode EdgeConv layer and its ordered backward (DGCNN)
    geoa3::knn_points_grad its backward, every point's terms in a fixed order      (pytorch3d knn backward)
    geoa3::knn_gather / _grad   pytorch3d.ops.knn_gather and its ordered backward  Lib/loss_utils.py:58,71,78
    geoa3::kappa           _get_kappa_ori / the forward of _get_kappa_adv   Lib/loss_utils.py:52-82
    geoa3::geo_loss_grad   CD / HD / L2 / curvature values and d constrain / d adv   Attacker/geoA3_attack.py:131-166
    geoa3::point_loss      chamfer / pseudo-chamfer / hausdorff / l2 with autograd    Lib/loss_utils.py:25-50
    geoa3::kappa_adv       _get_kappa_adv with autograd                               Lib/loss_utils.py:64-82
    geoa3::uniform_loss    uniform_loss (one scalar for the batch) with autograd      Lib/loss_utils.py:151-189
    geoa3::knn_smoothing_loss / repulsion_loss / displacement_loss / corresponding_normal_loss  with autograd  Lib/loss_utils.py:99-149
    geoa3::mesh_surface_points / _grad   pytorch3d's sample_points_from_meshes at a fixed draw and its ordered pullback
    geoa3::mesh_reg / _grad   pytorch3d's mesh_laplacian_smoothing(method="uniform") and mesh_edge_loss per mesh   main_attack.py:283-293
    geoa3::pointnet_forward / _backward   PointNet.forward (eval) and its input gradient   Model/PointNet.py:132-160
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch.library import custom_op

from . import ops

Tensor = torch.Tensor
_f32 = torch.float32
_i32 = torch.int32


def _planar(x: Tensor) -> Tensor:
    return x.detach().contiguous().float()


# ------------------------------------------------------------------------------------------------ searches
@custom_op("geoa3::nn1_pair", mutates_args=(), device_types="cuda")
def nn1_pair(a: Tensor, r: Tensor, both: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """a [B,3,Na], r [B,3,Nr] planar -> d_ar [B,Na], i_ar int32, d_ra [B,Nr], i_ra (empty [B,0] when not both)."""
    d_ar, i_ar, d_ra, i_ra = ops.nn1_pair(_planar(a), _planar(r), both=both, method="auto")
    if not both:
        d_ra, i_ra = a.new_empty(a.shape[0], 0, dtype=_f32), a.new_empty(a.shape[0], 0, dtype=_i32)
    return d_ar, i_ar, d_ra, i_ra


@nn1_pair.register_fake
def _(a, r, both):
    B, Na, Nr = a.shape[0], a.shape[2], (r.shape[2] if both else 0)
    return (a.new_empty(B, Na, dtype=_f32), a.new_empty(B, Na, dtype=_i32), a.new_empty(B, Nr, dtype=_f32),
            a.new_empty(B, Nr, dtype=_i32))


@custom_op("geoa3::knn", mutates_args=(), device_types="cuda")
def knn(q: Tensor, r: Tensor, K: int) -> Tuple[Tensor, Tensor]:
    """q [B,3,Nq], r [B,3,Nr] planar -> dists [B,Nq,K] ascending, idx int32 [B,Nq,K]."""
    return ops.knn_planar(_planar(q), _planar(r), K)


@knn.register_fake
def _(q, r, K):
    B, Nq = q.shape[0], q.shape[2]
    return q.new_empty(B, Nq, K, dtype=_f32), q.new_empty(B, Nq, K, dtype=_i32)


@custom_op("geoa3::kappa", mutates_args=(), device_types="cuda")
def kappa(pc: Tensor, normal: Tensor, knn_idx: Tensor, nn_idx: Optional[Tensor]) -> Tensor:
    return ops.kappa(_planar(pc), _planar(normal), knn_idx.contiguous(), None if nn_idx is None else nn_idx.contiguous())


@kappa.register_fake
def _(pc, normal, knn_idx, nn_idx):
    return pc.new_empty(pc.shape[0], pc.shape[2], dtype=_f32)


# ------------------------------------------------------------------------------------------------ the fused objective
@custom_op("geoa3::geo_loss_grad", mutates_args=(), device_types="cuda")
def geo_loss_grad(adv: Tensor, ori: Tensor, normal_ori: Optional[Tensor], kappa_ori: Optional[Tensor],
                  d_ao: Optional[Tensor], i_ao: Optional[Tensor], d_oa: Optional[Tensor], i_oa: Optional[Tensor],
                  knn_adv: Optional[Tensor], dkappa: Optional[Tensor], k: int, dis_type: int, single_side: bool,
                  w_dis: float, w_hd: float, w_curv: float, deterministic: bool
                  ) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """-> (dis_loss [B], hd_loss [B], curv_loss [B], constrain [B], d constrain / d adv [B,3,N])."""
    c = lambda t: None if t is None else t.contiguous()
    o = ops.geo_loss_grad(_planar(adv), _planar(ori), normal_ori=c(normal_ori), kappa_ori=c(kappa_ori), d_ao=c(d_ao),
                          i_ao=c(i_ao), d_oa=c(d_oa), i_oa=c(i_oa), knn_adv=c(knn_adv), dkappa=c(dkappa), k=k,
                          dis_type=dis_type, single_side=single_side, w_dis=w_dis, w_hd=w_hd, w_curv=w_curv,
                          deterministic=deterministic)
    return o["dis_loss"], o["hd_loss"], o["curv_loss"], o["constrain"], o["grad"]


@geo_loss_grad.register_fake
def _(adv, ori, normal_ori, kappa_ori, d_ao, i_ao, d_oa, i_oa, knn_adv, dkappa, k, dis_type, single_side, w_dis, w_hd,
      w_curv, deterministic):
    B = adv.shape[0]
    v = lambda: adv.new_empty(B, dtype=_f32)
    return v(), v(), v(), v(), adv.new_empty(B, 3, adv.shape[2], dtype=_f32)


# ------------------------------------------------------------------------------------------------ pytorch3d.ops.knn_points
@custom_op("geoa3::knn_points", mutates_args=(), device_types="cuda")
def knn_points_op(p1: Tensor, p2: Tensor, K: int) -> Tuple[Tensor, Tensor]:
    """p1 [b,n1,D], p2 [b,n2,D] -> dists [b,n1,K] (squared, ascending), idx int64 [b,n1,K].  D == 3: the planar searches;
    any other D: geoa3_knn_nd on the arguments as they are (point-major)."""
    if p1.shape[2] != 3:
        d, i = ops.knn_nd(p1.detach().contiguous().float(), p2.detach().contiguous().float(), K)
        return d, i.long()
    q = p1.detach().permute(0, 2, 1).contiguous().float()
    r = p2.detach().permute(0, 2, 1).contiguous().float()
    if K == 1:
        d, i, _, _ = ops.nn1_pair(q, r, both=False, method="auto")
        d, i = d.unsqueeze(-1), i.unsqueeze(-1)
    else:
        d, i = ops.knn_planar(q, r, K)
    return d, i.long()


@knn_points_op.register_fake
def _(p1, p2, K):
    b, n1 = p1.shape[0], p1.shape[1]
    return p1.new_empty(b, n1, K, dtype=_f32), p1.new_empty(b, n1, K, dtype=torch.int64)


def _knn_points_setup(ctx, inputs, output):
    p1, p2, _K = inputs
    ctx.save_for_backward(p1, p2, output[1])


def _knn_points_backward(ctx, gd, _gi):
    # pytorch3d's knn backward: dp1 += 2 g (p1 - p2[idx]);  dp2[idx] -= the same, every point's terms in a fixed order
    p1, p2, idx = ctx.saved_tensors
    if p1.shape[2] != 3:
        # the autograd of ((p1.unsqueeze(2) - knn_gather(p2, idx))**2).sum(-1), its two sums through the ordered gather
        # backward: p2's rows by idx, p1's by a table that sends every entry of a query to the query itself
        b, n1, K = idx.shape
        t = (2.0 * gd.float()).unsqueeze(-1) * (p1.float().unsqueeze(2) - torch.ops.geoa3.knn_gather(p2.float(), idx))
        own = torch.arange(n1, device=idx.device, dtype=torch.int64).view(1, n1, 1).expand(b, n1, K).contiguous()
        g1 = torch.ops.geoa3.knn_gather_grad(t, own, n1)
        g2 = torch.ops.geoa3.knn_gather_grad(-t, idx, p2.shape[1])
        return g1.to(p1.dtype), g2.to(p2.dtype), None
    g1, g2 = torch.ops.geoa3.knn_points_grad(p1, p2, idx, gd)
    return g1, g2, None


knn_points_op.register_autograd(_knn_points_backward, setup_context=_knn_points_setup)

def _no_second_derivative(name):
    def backward(ctx, *grads):
        raise RuntimeError("geoa3::%s is a first derivative and has no derivative of its own: nothing in the package or the "
                           "reference differentiates twice through knn_points / knn_gather (create_graph=True)" % name)
    return backward


@custom_op("geoa3::knn_points_grad", mutates_args=(), device_types="cuda")
def knn_points_grad(p1: Tensor, p2: Tensor, idx: Tensor, gd: Tensor) -> Tuple[Tensor, Tensor]:
    """The backward of geoa3::knn_points through dists: p1 [b,n1,3], p2 [b,n2,3], idx int64 / gd [b,n1,K] ->
    (d p1 [b,n1,3], d p2 [b,n2,3]), each point's terms added in ascending (query, neighbour) order."""
    g1, g2 = ops.knn_points_grad(p1.detach().contiguous().float(), p2.detach().contiguous().float(),
                                 idx.contiguous().long(), gd.detach().contiguous().float())
    return g1.to(p1.dtype), g2.to(p2.dtype)


@knn_points_grad.register_fake
def _(p1, p2, idx, gd):
    return p1.new_empty(p1.shape), p2.new_empty(p2.shape)


knn_points_grad.register_autograd(_no_second_derivative("knn_points_grad"))


# ------------------------------------------------------------------------------------------------ pytorch3d.ops.knn_gather
@custom_op("geoa3::knn_gather", mutates_args=(), device_types="cuda")
def knn_gather_op(x: Tensor, idx: Tensor) -> Tensor:
    """x [b,m,u] float32, idx int64 [b,l,k] -> [b,l,k,u]."""
    return ops.knn_gather_fwd(x.detach().contiguous(), idx.contiguous())


@knn_gather_op.register_fake
def _(x, idx):
    return x.new_empty(idx.shape[0], idx.shape[1], idx.shape[2], x.shape[2], dtype=_f32)


@custom_op("geoa3::knn_gather_grad", mutates_args=(), device_types="cuda")
def knn_gather_grad(g: Tensor, idx: Tensor, m: int) -> Tensor:
    """The backward of geoa3::knn_gather: g [b,l,k,u], idx int64 [b,l,k] -> d x [b,m,u], row j the sum of the g[b,l,k,:]
    with idx[b,l,k] == j in ascending (l, k) order."""
    return ops.knn_gather_grad(g.detach().contiguous().float(), idx.contiguous(), int(m))


@knn_gather_grad.register_fake
def _(g, idx, m):
    return g.new_empty(g.shape[0], m, g.shape[3], dtype=_f32)


knn_gather_grad.register_autograd(_no_second_derivative("knn_gather_grad"))


def _knn_gather_setup(ctx, inputs, output):
    x, idx = inputs
    ctx.save_for_backward(idx)
    ctx.m = x.shape[1]


def _knn_gather_backward(ctx, g):
    (idx,) = ctx.saved_tensors
    return torch.ops.geoa3.knn_gather_grad(g, idx, ctx.m), None


knn_gather_op.register_autograd(_knn_gather_backward, setup_context=_knn_gather_setup)

# ------------------------------------------------------------------------------------------------ fused EdgeConv (DGCNN)
@custom_op("geoa3::edge_max", mutates_args=(), device_types="cuda")
def edge_max_op(U: Tensor, V: Tensor, t: Tensor, idx: Tensor) -> Tuple[Tensor, Tensor]:
    """U, V [b,n,c] float32, t [c], idx int64 [b,n,k] -> (y [b,c,n] = max over the neighbours of lrelu_0.2(U[j] + V[i] + t),
    arg int32 [b,n,c], the neighbour slot that reaches it).  No gradient flows through idx."""
    return ops.edge_max(U.detach().contiguous().float(), V.detach().contiguous().float(), t.detach().contiguous().float(),
                        idx.contiguous())


@edge_max_op.register_fake
def _(U, V, t, idx):
    b, n, c = U.shape
    return U.new_empty(b, c, n, dtype=_f32), U.new_empty(b, n, c, dtype=_i32)


@custom_op("geoa3::edge_max_grad", mutates_args=(), device_types="cuda")
def edge_max_grad_op(g: Tensor, y: Tensor, arg: Tensor, idx: Tensor) -> Tuple[Tensor, Tensor]:
    """The backward of geoa3::edge_max: g, y [b,c,n], arg int32 [b,n,c], idx int64 [b,n,k] -> (d U, d V) [b,n,c], every row
    of d U summed in ascending (point, slot) order."""
    return ops.edge_max_grad(g.detach().contiguous().float(), y.contiguous(), arg.contiguous(), idx.contiguous())


@edge_max_grad_op.register_fake
def _(g, y, arg, idx):
    b, c, n = g.shape
    return g.new_empty(b, n, c, dtype=_f32), g.new_empty(b, n, c, dtype=_f32)


edge_max_grad_op.register_autograd(_no_second_derivative("edge_max_grad"))


def _edge_max_setup(ctx, inputs, output):
    ctx.save_for_backward(output[0], output[1], inputs[3])


def _edge_max_backward(ctx, g, _ga):
    y, arg, idx = ctx.saved_tensors
    dU, dV = torch.ops.geoa3.edge_max_grad(g, y, arg, idx)
    dt = dV.sum((0, 1)) if ctx.needs_input_grad[2] else None
    return dU, dV, dt, None


edge_max_op.register_autograd(_edge_max_backward, setup_context=_edge_max_setup)

# ------------------------------------------------------------------------------------------------ Lib/loss_utils.py
_KINDS = {"cd": 0, "pcd": 1, "hd": 2, "l2": 3}


@custom_op("geoa3::point_loss", mutates_args=(), device_types="cuda")
def point_loss(adv_pc: Tensor, ori_pc: Tensor, kind: int) -> Tuple[Tensor, Tensor]:
    """One of chamfer (0) / pseudo-chamfer (1) / hausdorff (2) / l2 (3): -> (loss [b], d loss / d adv [b,3,n])."""
    adv, ori = _planar(adv_pc), _planar(ori_pc)
    kw = dict(dis_type=0, w_dis=0.0, w_hd=0.0)
    if kind in (0, 1, 2):
        d_ao, i_ao, d_oa, i_oa = ops.nn1_pair(adv, ori, both=(kind == 0), method="auto")
        kw.update(d_ao=d_ao, i_ao=i_ao, d_oa=d_oa, i_oa=i_oa)
    if kind == 0:
        kw.update(dis_type=1, w_dis=1.0)
    elif kind == 1:
        kw.update(dis_type=1, w_dis=1.0, single_side=True)
    elif kind == 2:
        kw.update(w_hd=1.0)
    else:
        kw.update(dis_type=2, w_dis=1.0)
    out = ops.geo_loss_grad(adv, ori, **kw)
    return (out["hd_loss"] if kind == 2 else out["dis_loss"]).clone(), out["grad"]


@point_loss.register_fake
def _(adv_pc, ori_pc, kind):
    return adv_pc.new_empty(adv_pc.shape[0], dtype=_f32), adv_pc.new_empty(adv_pc.shape, dtype=_f32)


def _point_loss_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _point_loss_backward(ctx, g, _gg):
    (grad,) = ctx.saved_tensors
    return grad * g.view(-1, 1, 1), None, None


point_loss.register_autograd(_point_loss_backward, setup_context=_point_loss_setup)


@custom_op("geoa3::kappa_adv", mutates_args=(), device_types="cuda")
def kappa_adv(adv_pc: Tensor, ori_pc: Tensor, ori_normal: Tensor, k: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """_get_kappa_adv: -> (kappa_adv [b,n], normal [b,3,n], i_ao int32 [b,n], knn_adv int32 [b,n,k+1])."""
    adv, ori, nrm = _planar(adv_pc), _planar(ori_pc), _planar(ori_normal)
    _, i_ao, _, _ = ops.nn1_pair(adv, ori, both=False, method="auto")
    _, knn_adv = ops.knn_planar(adv, adv, k + 1)
    kap = ops.kappa(adv, nrm, knn_adv, i_ao)
    b, _, n = adv.shape
    normal = torch.gather(nrm, 2, i_ao.long().unsqueeze(1).expand(b, 3, n)).contiguous()
    return kap, normal, i_ao, knn_adv


@kappa_adv.register_fake
def _(adv_pc, ori_pc, ori_normal, k):
    b, _, n = adv_pc.shape
    return (adv_pc.new_empty(b, n, dtype=_f32), adv_pc.new_empty(b, 3, n, dtype=_f32), adv_pc.new_empty(b, n, dtype=_i32),
            adv_pc.new_empty(b, n, k + 1, dtype=_i32))


def _kappa_adv_setup(ctx, inputs, output):
    adv_pc, ori_pc, ori_normal, k = inputs
    ctx.save_for_backward(adv_pc, ori_pc, ori_normal, output[2], output[3])
    ctx.k = k


def _kappa_adv_backward(ctx, gk, _gn, _gi, _gt):
    adv, ori, nrm, i_ao, knn_adv = ctx.saved_tensors
    out = torch.ops.geoa3.geo_loss_grad(adv, ori, nrm, None, None, i_ao, None, None, knn_adv, gk.contiguous().float(),
                                        ctx.k, 0, False, 0.0, 0.0, 0.0, True)
    return out[4], None, None, None


kappa_adv.register_autograd(_kappa_adv_backward, setup_context=_kappa_adv_setup)

@custom_op("geoa3::uniform_loss", mutates_args=(), device_types="cuda")
def uniform_loss(adv_pc: Tensor, percentages: List[float], radius: float, k: int, contract: int) -> Tuple[Tensor, Tensor]:
    """uniform_loss on adv_pc [b,3,n] planar -> (U [] float32, dU / d adv [b,3,n]).  contract: -1 = the choice of
    geoa3_amd.pointnet2.ext_contract_default, 0 / 1 = GEOA3_PN2_CONTRACT off / on."""
    return ops.uniform_loss(_planar(adv_pc), percentages, radius, k, contract=None if contract < 0 else bool(contract))


@uniform_loss.register_fake
def _(adv_pc, percentages, radius, k, contract):
    return adv_pc.new_empty((), dtype=_f32), adv_pc.new_empty(adv_pc.shape, dtype=_f32)


def _uniform_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])


def _uniform_backward(ctx, g, _gg):
    (grad,) = ctx.saved_tensors
    return grad * g, None, None, None, None


uniform_loss.register_autograd(_uniform_backward, setup_context=_uniform_setup)

# ------------------------------------------------------------------------------------------------ neighbour regularisers
# Each forward returns the K-NN table it used beside the value, so that the registered backward (itself an op: a traced
# backward graph holds it) differentiates THAT selection, as autograd does through the reference's topk / knn_points.
@custom_op("geoa3::knn_smoothing_loss", mutates_args=(), device_types="cuda")
def knn_smoothing_loss(adv_pc: Tensor, k: int, threshold_coef: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """kNN_smoothing_loss on adv_pc [b,3,n] -> (loss [b], mask [b,n] uint8, knn dists [b,n,k+1], knn idx int32)."""
    x = _planar(adv_pc)
    d, i = ops.knn_self_planar(x, k + 1)
    loss, cond = ops.knn_smoothing_loss(x, k, threshold_coef, knn=(d, i), want_cond=True)
    return loss, cond, d, i


@knn_smoothing_loss.register_fake
def _(adv_pc, k, threshold_coef):
    b, _, n = adv_pc.shape
    return (adv_pc.new_empty(b, dtype=_f32), adv_pc.new_empty(b, n, dtype=torch.uint8),
            adv_pc.new_empty(b, n, k + 1, dtype=_f32), adv_pc.new_empty(b, n, k + 1, dtype=_i32))


@custom_op("geoa3::knn_smoothing_loss_grad", mutates_args=(), device_types="cuda")
def knn_smoothing_loss_grad(adv_pc: Tensor, knn_d: Tensor, knn_i: Tensor, g: Tensor, k: int, threshold_coef: float) -> Tensor:
    return ops.knn_smoothing_loss_grad(_planar(adv_pc), k, threshold_coef, g=g.contiguous().float(),
                                       knn=(knn_d.contiguous(), knn_i.contiguous()))


@knn_smoothing_loss_grad.register_fake
def _(adv_pc, knn_d, knn_i, g, k, threshold_coef):
    return adv_pc.new_empty(adv_pc.shape, dtype=_f32)


def _smooth_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], output[2], output[3])
    ctx.k, ctx.coef = inputs[1], inputs[2]


def _smooth_backward(ctx, g, _gc, _gd, _gi):
    x, d, i = ctx.saved_tensors
    return torch.ops.geoa3.knn_smoothing_loss_grad(x, d, i, g, ctx.k, ctx.coef), None, None


knn_smoothing_loss.register_autograd(_smooth_backward, setup_context=_smooth_setup)


@custom_op("geoa3::repulsion_loss", mutates_args=(), device_types="cuda")
def repulsion_loss(pc: Tensor, k: int, h: float) -> Tuple[Tensor, Tensor, Tensor]:
    """repulsion_loss on pc [b,3,n] -> (out [b,n], knn dists [b,n,k+1], knn idx int32)."""
    x = _planar(pc)
    d, i = ops.knn_self_planar(x, k + 1)
    return ops.repulsion_loss(x, k, h, knn=(d, i)), d, i


@repulsion_loss.register_fake
def _(pc, k, h):
    b, _, n = pc.shape
    return (pc.new_empty(b, n, dtype=_f32), pc.new_empty(b, n, k + 1, dtype=_f32), pc.new_empty(b, n, k + 1, dtype=_i32))


@custom_op("geoa3::repulsion_loss_grad", mutates_args=(), device_types="cuda")
def repulsion_loss_grad(pc: Tensor, knn_d: Tensor, knn_i: Tensor, g: Tensor, k: int, h: float) -> Tensor:
    return ops.repulsion_loss_grad(_planar(pc), k, h, g=g.contiguous().float(), knn=(knn_d.contiguous(), knn_i.contiguous()))


@repulsion_loss_grad.register_fake
def _(pc, knn_d, knn_i, g, k, h):
    return pc.new_empty(pc.shape, dtype=_f32)


def _repulse_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], output[1], output[2])
    ctx.k, ctx.h = inputs[1], inputs[2]


def _repulse_backward(ctx, g, _gd, _gi):
    x, d, i = ctx.saved_tensors
    return torch.ops.geoa3.repulsion_loss_grad(x, d, i, g, ctx.k, ctx.h), None, None


repulsion_loss.register_autograd(_repulse_backward, setup_context=_repulse_setup)


@custom_op("geoa3::displacement_loss", mutates_args=(), device_types="cuda")
def displacement_loss(adv_pc: Tensor, ori_pc: Tensor, k: int) -> Tuple[Tensor, Tensor, Tensor]:
    """displacement_loss on adv_pc, ori_pc [b,3,n] -> (out [b,n], knn dists / idx [b,n,k+1] of ORI)."""
    adv, ori = _planar(adv_pc), _planar(ori_pc)
    d, i = ops.knn_self_planar(ori, k + 1)
    return ops.displacement_loss(adv, ori, k, knn=(d, i)), d, i


@displacement_loss.register_fake
def _(adv_pc, ori_pc, k):
    b, _, n = adv_pc.shape
    return (adv_pc.new_empty(b, n, dtype=_f32), adv_pc.new_empty(b, n, k + 1, dtype=_f32),
            adv_pc.new_empty(b, n, k + 1, dtype=_i32))


@custom_op("geoa3::displacement_loss_grad", mutates_args=(), device_types="cuda")
def displacement_loss_grad(adv_pc: Tensor, ori_pc: Tensor, knn_d: Tensor, knn_i: Tensor, g: Tensor, k: int) -> Tensor:
    return ops.displacement_loss_grad(_planar(adv_pc), _planar(ori_pc), k, g=g.contiguous().float(),
                                      knn=(knn_d.contiguous(), knn_i.contiguous()))


@displacement_loss_grad.register_fake
def _(adv_pc, ori_pc, knn_d, knn_i, g, k):
    return adv_pc.new_empty(adv_pc.shape, dtype=_f32)


def _displace_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], output[1], output[2])
    ctx.k = inputs[2]


def _displace_backward(ctx, g, _gd, _gi):
    adv, ori, d, i = ctx.saved_tensors
    return torch.ops.geoa3.displacement_loss_grad(adv, ori, d, i, g, ctx.k), None, None


displacement_loss.register_autograd(_displace_backward, setup_context=_displace_setup)


@custom_op("geoa3::corresponding_normal_loss", mutates_args=(), device_types="cuda")
def corresponding_normal_loss(adv_pc: Tensor, normal: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """corresponding_normal_loss on adv_pc, normal [b,3,n] -> (out [b,n], knn idx int32 [b,n,k+1] of adv)."""
    return ops.corresponding_normal_loss(_planar(adv_pc), _planar(normal), k, want_knn=True)


@corresponding_normal_loss.register_fake
def _(adv_pc, normal, k):
    b, _, n = adv_pc.shape
    return adv_pc.new_empty(b, n, dtype=_f32), adv_pc.new_empty(b, n, k + 1, dtype=_i32)


@custom_op("geoa3::corresponding_normal_loss_grad", mutates_args=(), device_types="cuda")
def corresponding_normal_loss_grad(adv_pc: Tensor, normal: Tensor, knn_i: Tensor, g: Tensor) -> Tensor:
    return ops.corresponding_normal_loss_grad(_planar(adv_pc), _planar(normal), knn_i.contiguous(), g.contiguous().float())


@corresponding_normal_loss_grad.register_fake
def _(adv_pc, normal, knn_i, g):
    return adv_pc.new_empty(adv_pc.shape, dtype=_f32)


def _cnl_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1], output[1])


def _cnl_backward(ctx, g, _gi):
    adv, nrm, i = ctx.saved_tensors
    return torch.ops.geoa3.corresponding_normal_loss_grad(adv, nrm, i, g), None, None


corresponding_normal_loss.register_autograd(_cnl_backward, setup_context=_cnl_setup)


# ------------------------------------------------------------------------------------------------ the mesh attack
# pytorch3d's sample_points_from_meshes at a fixed draw, mesh_laplacian_smoothing(method="uniform") and mesh_edge_loss on
# planar padded vertices [B,3,Vp] (geoa3_amd.mesh: surface_points, mesh_laplacian_smoothing, mesh_edge_loss)
@custom_op("geoa3::mesh_surface_points", mutates_args=(), device_types="cuda")
def mesh_surface_points(verts: Tensor, nv: Tensor, faces: Tensor, face_off: Tensor, face_idx: Tensor, u: Tensor,
                        lists: Optional[Tensor]) -> Tensor:
    """verts [B,3,Vp], nv i32 [B], faces i32 [sumF,3], face_off i64 [B+1], face_idx i32 [B,S], u [B,S,3] -> pts [B,3,S].
    lists: mesh_point_lists of the draw for the backward (None: it sorts the draw itself)."""
    from . import mesh
    return mesh.mesh_points_forward(verts, nv, faces, face_off, face_idx, u)


@mesh_surface_points.register_fake
def _(verts, nv, faces, face_off, face_idx, u, lists):
    return verts.new_empty(verts.shape[0], 3, face_idx.shape[1], dtype=_f32)


@custom_op("geoa3::mesh_surface_points_grad", mutates_args=(), device_types="cuda")
def mesh_surface_points_grad(g: Tensor, nv: Tensor, faces: Tensor, face_off: Tensor, face_idx: Tensor, u: Tensor,
                             lists: Optional[Tensor], vp: int) -> Tensor:
    """The pullback of geoa3::mesh_surface_points: g [B,3,S] -> d verts [B,3,vp], every vertex's terms in ascending
    (sample, corner) order."""
    from . import mesh
    if lists is None:
        lists = mesh.mesh_point_lists(nv, faces, face_off, face_idx, vp)
    return mesh.mesh_points_backward(g, u, lists, vp)


@mesh_surface_points_grad.register_fake
def _(g, nv, faces, face_off, face_idx, u, lists, vp):
    return g.new_empty(g.shape[0], 3, vp, dtype=_f32)


mesh_surface_points_grad.register_autograd(_no_second_derivative("mesh_surface_points_grad"))


def _mesh_points_setup(ctx, inputs, output):
    verts, nv, faces, face_off, face_idx, u, lists = inputs
    ctx.save_for_backward(nv, faces, face_off, face_idx, u)
    ctx.lists, ctx.vp, ctx.dtype = lists, verts.shape[2], verts.dtype


def _mesh_points_backward(ctx, g):
    nv, faces, face_off, face_idx, u = ctx.saved_tensors
    gv = torch.ops.geoa3.mesh_surface_points_grad(g, nv, faces, face_off, face_idx, u, ctx.lists, ctx.vp)
    return gv.to(ctx.dtype), None, None, None, None, None, None


mesh_surface_points.register_autograd(_mesh_points_backward, setup_context=_mesh_points_setup)


@custom_op("geoa3::mesh_reg", mutates_args=(), device_types="cuda")
def mesh_reg(verts: Tensor, nv: Tensor, row_off: Tensor, col: Tensor, ne: Tensor, target: Optional[Tensor],
             target_scalar: float) -> Tuple[Tensor, Tensor, Tensor]:
    """verts [B,3,Vp] and the CSR of a MeshTopology -> (Lap_b [B], Edge_b [B], unit [B,4,Vp] = (u_i, |delta_i|) for the
    gradient).  target: one length per CSR entry, or None for target_scalar."""
    from . import mesh
    return mesh.mesh_reg_forward(verts, nv, row_off, col, ne, target, target_scalar)


@mesh_reg.register_fake
def _(verts, nv, row_off, col, ne, target, target_scalar):
    b = verts.shape[0]
    return (verts.new_empty(b, dtype=_f32), verts.new_empty(b, dtype=_f32), verts.new_empty(b, 4, verts.shape[2], dtype=_f32))


@custom_op("geoa3::mesh_reg_grad", mutates_args=(), device_types="cuda")
def mesh_reg_grad(verts: Tensor, nv: Tensor, row_off: Tensor, col: Tensor, ne: Tensor, target: Optional[Tensor],
                  target_scalar: float, unit: Tensor, g_lap: Optional[Tensor], g_edge: Optional[Tensor]) -> Tensor:
    """d (g_lap . Lap + g_edge . Edge) / d verts [B,3,Vp] in one gather over the CSR; a term whose g is None is skipped."""
    from . import mesh
    return mesh.mesh_reg_backward(verts, nv, row_off, col, ne, target, target_scalar, unit, g_lap, g_edge,
                                  w_lap=0.0 if g_lap is None else 1.0, w_edge=0.0 if g_edge is None else 1.0)


@mesh_reg_grad.register_fake
def _(verts, nv, row_off, col, ne, target, target_scalar, unit, g_lap, g_edge):
    return verts.new_empty(verts.shape, dtype=_f32)


mesh_reg_grad.register_autograd(_no_second_derivative("mesh_reg_grad"))


def _mesh_reg_setup(ctx, inputs, output):
    verts, nv, row_off, col, ne, target, target_scalar = inputs
    ctx.save_for_backward(verts, nv, row_off, col, ne, output[2])
    ctx.target, ctx.target_scalar = target, target_scalar
    ctx.set_materialize_grads(False)   # a term nobody reads arrives as None and is skipped, not multiplied by 0


def _mesh_reg_backward(ctx, g_lap, g_edge, _g_unit):
    verts, nv, row_off, col, ne, unit = ctx.saved_tensors
    if g_lap is None and g_edge is None:
        return (None,) * 7
    gv = torch.ops.geoa3.mesh_reg_grad(verts, nv, row_off, col, ne, ctx.target, ctx.target_scalar, unit, g_lap, g_edge)
    return gv.to(verts.dtype), None, None, None, None, None, None


mesh_reg.register_autograd(_mesh_reg_backward, setup_context=_mesh_reg_setup)

# ------------------------------------------------------------------------------------------------ the victim
import weakref

_NETS = weakref.WeakValueDictionary()   # handle -> geoa3_amd.pointnet.PointNet (custom ops take tensors and scalars only)


import itertools

_NEXT_HANDLE = itertools.count(1)


def register_net(net) -> int:
    """A handle for `net` (a geoa3_amd.pointnet.PointNet in eval mode) to pass to geoa3::pointnet_forward.  Handles
    come from a counter (never reused); a copy of a module (copy.deepcopy / pickle) registers itself again in
    PointNet.__setstate__."""
    h = next(_NEXT_HANDLE)
    _NETS[h] = net
    return h


def net_handle(net) -> int:
    """The handle under which `net` itself is registered (re-registered if the stored one belongs to another module).
    Eager callers; a traced forward reads net._handle, which PointNet.__setstate__ keeps its own for copies."""
    h = getattr(net, "_handle", None)
    if h is None or _NETS.get(h) is not net:
        h = net._handle = register_net(net)
    return h


@custom_op("geoa3::pointnet_forward", mutates_args=(), device_types="cuda")
def pointnet_forward(x: Tensor, handle: int) -> Tensor:
    """Eval-mode PointNet.forward on x [b,3,n] -> logits [b,classes] (the library's forward; activations stay in the
    net's workspace for a backward of the SAME input)."""
    from .pointnet import pointnet_forward_raw
    return pointnet_forward_raw(_NETS[handle], x)


@pointnet_forward.register_fake
def _(x, handle):
    return x.new_empty(x.shape[0], int(_NETS[handle].classes), dtype=_f32)


@custom_op("geoa3::pointnet_backward", mutates_args=(), device_types="cuda")
def pointnet_backward(x: Tensor, dlogits: Tensor, handle: int) -> Tensor:
    """d (logits . dlogits) / d x [b,3,n]: recomputes the forward of x into the workspace, then the input gradient."""
    from .pointnet import pointnet_backward_raw
    return pointnet_backward_raw(_NETS[handle], x, dlogits)


@pointnet_backward.register_fake
def _(x, dlogits, handle):
    return x.new_empty(x.shape, dtype=_f32)


def _pn_setup(ctx, inputs, output):
    x, handle = inputs
    ctx.save_for_backward(x)
    ctx.handle = handle


def _pn_backward(ctx, g):
    (x,) = ctx.saved_tensors
    return torch.ops.geoa3.pointnet_backward(x, g.contiguous(), ctx.handle), None


pointnet_forward.register_autograd(_pn_backward, setup_context=_pn_setup)
