"""Tensor-level entry points over the C ABI (include/geoa3_hip.h): device memory and streams are
PyTorch-ROCm's, the arithmetic is the HIP library's.  No CPU fallback: CPU tensors are rejected.

Planar layout: clouds are fp32 [B,3,N] contiguous (the reference's logical layout)."""
from __future__ import annotations

import collections
import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import GeoArgs, check

Tensor = torch.Tensor


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[Tensor], dtype=None) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.Geoa3Error("geoa3_amd ops need device (cuda/HIP) tensors; there is no CPU path")
    if not t.is_contiguous():
        raise _lib.Geoa3Error("tensor must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise _lib.Geoa3Error("expected dtype %s, got %s" % (dtype, t.dtype))
    return t.data_ptr()


def nn1_pair(a: Tensor, r: Tensor, both: bool = True, method: str = "brute", prior=None, policy=None):
    """a [B,3,Na], r [B,3,Nr] -> (d_ar [B,Na], i_ar int32 [B,Na], d_ra [B,Nr] | None, i_ra | None).
    method: "brute" (all pairs, geoa3_nn1_pair), "grid" (geoa3_grid_nn1_pair: the pruned searches -- matrix-core filter /
    grid walk -- same bits; prior = (i_ar, i_ra) of a previous call seeds its radii; policy = (brute_frac, filter) of
    geoa3_debug_grid_nn1_pair for tests / tools) or "auto" (the pruned search whenever both clouds hold >= 32 points)."""
    B, _, Na = a.shape
    Nr = r.shape[2]
    d_ar = torch.empty(B, Na, device=a.device, dtype=torch.float32)
    i_ar = torch.empty(B, Na, device=a.device, dtype=torch.int32)
    d_ra = i_ra = None
    if both:
        d_ra = torch.empty(B, Nr, device=a.device, dtype=torch.float32)
        i_ra = torch.empty(B, Nr, device=a.device, dtype=torch.int32)
    if method == "auto":
        method = "grid" if min(Na, Nr) >= 32 else "brute"
    if method == "grid":
        p_ar, p_ra = prior if prior is not None else (None, None)
        if policy is not None:
            check(_lib.load().geoa3_debug_grid_nn1_pair(_p(a, torch.float32), _p(r, torch.float32), B, Na, Nr,
                                                        _p(p_ar, torch.int32) if p_ar is not None else None,
                                                        _p(p_ra, torch.int32) if p_ra is not None and both else None,
                                                        _p(d_ar), _p(i_ar), _p(d_ra), _p(i_ra), float(policy[0]),
                                                        int(policy[1]), _stream()), "geoa3_debug_grid_nn1_pair")
            return d_ar, i_ar, d_ra, i_ra
        check(_lib.load().geoa3_grid_nn1_pair(_p(a, torch.float32), _p(r, torch.float32), B, Na, Nr,
                                              _p(p_ar, torch.int32) if p_ar is not None else None,
                                              _p(p_ra, torch.int32) if p_ra is not None and both else None,
                                              _p(d_ar), _p(i_ar), _p(d_ra), _p(i_ra), _stream()), "geoa3_grid_nn1_pair")
    else:
        check(_lib.load().geoa3_nn1_pair(_p(a, torch.float32), _p(r, torch.float32), B, Na, Nr, _p(d_ar), _p(i_ar),
                                         _p(d_ra), _p(i_ra), _stream()), "geoa3_nn1_pair")
    return d_ar, i_ar, d_ra, i_ra


def knn_planar(q: Tensor, r: Tensor, K: int, prior: Optional[Tensor] = None, out=None) -> Tuple[Tensor, Tensor]:
    """q [B,3,Nq], r [B,3,Nr] -> (dists [B,Nq,K] ascending, idx int32 [B,Nq,K])."""
    B, _, Nq = q.shape
    Nr = r.shape[2]
    if out is None:
        d = torch.empty(B, Nq, K, device=q.device, dtype=torch.float32)
        i = torch.empty(B, Nq, K, device=q.device, dtype=torch.int32)
    else:
        d, i = out
    check(_lib.load().geoa3_knn(_p(q, torch.float32), _p(r, torch.float32), B, Nq, Nr, K, _p(prior, torch.int32),
                                _p(d), _p(i), _stream()), "geoa3_knn")
    return d, i


def knn_nd(q: Tensor, r: Tensor, K: int, out=None) -> Tuple[Tensor, Tensor]:
    """geoa3_knn_nd: q [B,Nq,D], r [B,Nr,D] point-major float32, 1 <= D <= 128 -> (dists [B,Nq,K] ascending by (distance,
    index), idx int32 [B,Nq,K]); the distance is the sequential float32 sum over d, a NaN distance counts as +inf."""
    B, Nq, D = q.shape
    Nr = r.shape[1]
    if r.shape[0] != B or r.shape[2] != D:
        raise _lib.Geoa3Error("knn_nd: q %s and r %s differ in batch or dimension" % (tuple(q.shape), tuple(r.shape)))
    if out is None:
        d = torch.empty(B, Nq, K, device=q.device, dtype=torch.float32)
        i = torch.empty(B, Nq, K, device=q.device, dtype=torch.int32)
    else:
        d, i = out
    check(_lib.load().geoa3_knn_nd(_p(q, torch.float32), _p(r, torch.float32), B, Nq, Nr, D, int(K), _p(d, torch.float32),
                                   _p(i, torch.int32), _stream()), "geoa3_knn_nd")
    return d, i


def edge_max(U: Tensor, V: Tensor, t: Tensor, idx: Tensor, out=None) -> Tuple[Tensor, Tensor]:
    """geoa3_edge_max: U, V [B,N,C] float32, t [C], idx int64 [B,N,k] -> (y [B,C,N], arg int32 [B,N,C]):
    y = lrelu_0.2(U[idx[i, arg]] + V[i] + t), arg the first slot that maximises U[idx[i, .], c]."""
    B, N, Cc = U.shape
    K = idx.shape[2]
    if tuple(V.shape) != (B, N, Cc) or tuple(t.shape) != (Cc,) or tuple(idx.shape[:2]) != (B, N):
        raise _lib.Geoa3Error("edge_max: U %s, V %s, t %s, idx %s do not fit" % (tuple(U.shape), tuple(V.shape),
                                                                                tuple(t.shape), tuple(idx.shape)))
    if out is None:
        y = torch.empty(B, Cc, N, device=U.device, dtype=torch.float32)
        arg = torch.empty(B, N, Cc, device=U.device, dtype=torch.int32)
    else:
        y, arg = out
    check(_lib.load().geoa3_edge_max(_p(U, torch.float32), _p(V, torch.float32), _p(t, torch.float32), _p(idx, torch.int64),
                                     B, N, Cc, K, _p(y, torch.float32), _p(arg, torch.int32), _stream()), "geoa3_edge_max")
    return y, arg


def edge_max_scratch(B: int, N: int, K: int, device) -> Tensor:
    """Scratch of edge_max_grad for B clouds of N points with K neighbours each."""
    nbytes = int(_lib.load().geoa3_edge_max_scratch_bytes(B, N, K))
    if nbytes < 0:
        raise _lib.Geoa3Error("edge_max_grad: sizes out of range (B=%d, N=%d, K=%d)" % (B, N, K))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def edge_max_grad(g: Tensor, y: Tensor, arg: Tensor, idx: Tensor, scratch: Optional[Tensor] = None, out=None):
    """geoa3_edge_max_grad: g, y [B,C,N] float32, arg int32 [B,N,C], idx int64 [B,N,k] -> (dU, dV) [B,N,C]: dV = g times the
    LeakyReLU slope from the sign of y, dU[j] the sum of the dV[i] whose arg-max neighbour is j, in ascending (i, slot)."""
    B, Cc, N = g.shape
    K = idx.shape[2]
    if tuple(y.shape) != (B, Cc, N) or tuple(arg.shape) != (B, N, Cc) or tuple(idx.shape[:2]) != (B, N):
        raise _lib.Geoa3Error("edge_max_grad: g %s, y %s, arg %s, idx %s do not fit" % (tuple(g.shape), tuple(y.shape),
                                                                                       tuple(arg.shape), tuple(idx.shape)))
    if out is None:
        dU = torch.empty(B, N, Cc, device=g.device, dtype=torch.float32)
        dV = torch.empty(B, N, Cc, device=g.device, dtype=torch.float32)
    else:
        dU, dV = out
    if scratch is None:
        scratch = edge_max_scratch(B, N, K, g.device)
    check(_lib.load().geoa3_edge_max_grad(_p(g, torch.float32), _p(y, torch.float32), _p(arg, torch.int32),
                                          _p(idx, torch.int64), B, N, Cc, K, _p(dU, torch.float32), _p(dV, torch.float32),
                                          _p(scratch), _stream()), "geoa3_edge_max_grad")
    return dU, dV


def edge_train_workspace(B: int, N: int, C_: int, K: int, device) -> Tensor:
    """Workspace of edge_train / edge_train_grad (geoa3_edge_train_workspace_bytes); the library's refusal raises."""
    nbytes = int(_lib.load().geoa3_edge_train_workspace_bytes(B, N, C_, K))
    if nbytes < 0:
        check(nbytes, "geoa3_edge_train_workspace_bytes")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def edge_train(U0: Tensor, V0: Tensor, idx: Tensor, gamma: Tensor, beta: Tensor, eps: float, workspace: Optional[Tensor] = None):
    """geoa3_edge_train_forward: U0, V0 [B,N,C] float32, idx int64 [B,N,k], gamma, beta [C] -> (y [B,C,N], arg int32 [B,N,C],
    S1 [B,N,C], mean [C], var [C] (biased), stats float64 [3,C] = mean | var | 1/sqrt(var + eps)): the neighbour half of a
    training-mode EdgeConv layer, y = lrelu_0.2(gamma r (U0[idx[i, arg]] + V0[i] - mean) + beta)."""
    B, N, Cc = U0.shape
    K = idx.shape[2]
    if tuple(V0.shape) != (B, N, Cc) or tuple(gamma.shape) != (Cc,) or tuple(beta.shape) != (Cc,) or tuple(idx.shape[:2]) != (B, N):
        raise _lib.Geoa3Error("edge_train: U0 %s, V0 %s, gamma %s, beta %s, idx %s do not fit" % (
            tuple(U0.shape), tuple(V0.shape), tuple(gamma.shape), tuple(beta.shape), tuple(idx.shape)))
    if workspace is None:
        workspace = edge_train_workspace(B, N, Cc, K, U0.device)
    dev = U0.device
    y = torch.empty(B, Cc, N, device=dev, dtype=torch.float32)
    arg = torch.empty(B, N, Cc, device=dev, dtype=torch.int32)
    S1 = torch.empty(B, N, Cc, device=dev, dtype=torch.float32)
    mean = torch.empty(Cc, device=dev, dtype=torch.float32)
    var = torch.empty(Cc, device=dev, dtype=torch.float32)
    stats = torch.empty(3, Cc, device=dev, dtype=torch.float64)
    check(_lib.load().geoa3_edge_train_forward(
        _p(U0, torch.float32), _p(V0, torch.float32), _p(idx, torch.int64), _p(gamma, torch.float32), _p(beta, torch.float32),
        float(eps), B, N, Cc, K, _p(y), _p(arg), _p(S1), _p(mean), _p(var), _p(stats), _p(workspace), _stream()),
        "geoa3_edge_train_forward")
    return y, arg, S1, mean, var, stats


def edge_train_grad(g: Tensor, y: Tensor, U0: Tensor, V0: Tensor, arg: Tensor, S1: Tensor, idx: Tensor, gamma: Tensor,
                    stats: Tensor, workspace: Optional[Tensor] = None):
    """geoa3_edge_train_grad: g, y [B,C,N]; the forward's inputs and arg, S1, stats -> (dU0, dV0 [B,N,C], dgamma, dbeta [C])."""
    B, N, Cc = U0.shape
    K = idx.shape[2]
    if (tuple(g.shape) != (B, Cc, N) or tuple(y.shape) != (B, Cc, N) or tuple(V0.shape) != (B, N, Cc)
            or tuple(arg.shape) != (B, N, Cc) or tuple(S1.shape) != (B, N, Cc) or tuple(idx.shape[:2]) != (B, N)
            or tuple(gamma.shape) != (Cc,) or tuple(stats.shape) != (3, Cc)):
        raise _lib.Geoa3Error("edge_train_grad: g %s, y %s, U0 %s, V0 %s, arg %s, S1 %s, idx %s, gamma %s, stats %s do not fit" % (
            tuple(g.shape), tuple(y.shape), tuple(U0.shape), tuple(V0.shape), tuple(arg.shape), tuple(S1.shape),
            tuple(idx.shape), tuple(gamma.shape), tuple(stats.shape)))
    if workspace is None:
        workspace = edge_train_workspace(B, N, Cc, K, U0.device)
    dev = U0.device
    dU0 = torch.empty(B, N, Cc, device=dev, dtype=torch.float32)
    dV0 = torch.empty(B, N, Cc, device=dev, dtype=torch.float32)
    dgamma = torch.empty(Cc, device=dev, dtype=torch.float32)
    dbeta = torch.empty(Cc, device=dev, dtype=torch.float32)
    check(_lib.load().geoa3_edge_train_grad(
        _p(g, torch.float32), _p(y, torch.float32), _p(U0, torch.float32), _p(V0, torch.float32), _p(arg, torch.int32),
        _p(S1, torch.float32), _p(idx, torch.int64), _p(gamma, torch.float32), _p(stats, torch.float64), B, N, Cc, K,
        _p(dU0), _p(dV0), _p(dgamma), _p(dbeta), _p(workspace), _stream()), "geoa3_edge_train_grad")
    return dU0, dV0, dgamma, dbeta


def knn_self_scratch(B: int, N: int, device) -> Tensor:
    """Scratch buffer of geoa3_knn_self for [B,3,N] clouds."""
    return torch.empty(int(_lib.load().geoa3_knn_self_scratch_bytes(B, N)), dtype=torch.uint8, device=device)


def knn_self_planar(pc: Tensor, K: int, prior: Optional[Tensor] = None, scratch: Optional[Tensor] = None,
                    out=None, method: int = 0) -> Tuple[Tensor, Tensor]:
    """== knn_planar(pc, pc, K, prior) bit for bit; pruned when prior and scratch (knn_self_scratch) are given, N <= 8192
    and K <= N.  method (GEOA3_KNN_SELF_* of geoa3_hip.h) 0: the cell grid for K > 20 or N >= 2048, else the slab search;
    1: slab along the longest axis (position lists for launches of more than 512 workgroups, else (distance, index) lists);
    2: cell grid with one wavefront per query; 3 / 4: slab with (distance, index) / position lists whatever the launch size.
    _lib.load().geoa3_debug_knn_self_route names the kernel a call takes."""
    B, _, N = pc.shape
    if out is None:
        d = torch.empty(B, N, K, device=pc.device, dtype=torch.float32)
        i = torch.empty(B, N, K, device=pc.device, dtype=torch.int32)
    else:
        d, i = out
    check(_lib.load().geoa3_knn_self(_p(pc, torch.float32), B, N, K, _p(prior, torch.int32), _p(d), _p(i),
                                     _p(scratch), int(method), _stream()), "geoa3_knn_self")
    return d, i


def kappa(pc: Tensor, normal: Tensor, knn_idx: Tensor, nn_idx: Optional[Tensor] = None) -> Tensor:
    """pc/normal [B,3,N], knn_idx int32 [B,N,k+1] -> kappa [B,N] (Lib/loss_utils.py:52-62)."""
    B, _, N = pc.shape
    k = knn_idx.shape[2] - 1
    out = torch.empty(B, N, device=pc.device, dtype=torch.float32)
    check(_lib.load().geoa3_kappa(_p(pc, torch.float32), _p(normal, torch.float32), _p(knn_idx, torch.int32),
                                  _p(nn_idx, torch.int32), B, N, int(normal.shape[2]), k, _p(out), _stream()),
          "geoa3_kappa")
    return out


GEO_WIDE_MIN_N = 5840   # the first cloud no single workgroup holds: geoa3_geo_loss_grad needs a scratch buffer from here on


def geo_scratch(B: int, N: int, device, k: int = 0) -> Tensor:
    """geoa3_geo_args.scratch for B clouds of N points (geoa3_geo_scratch_bytes: 16 bytes per point up to 4096 points)."""
    return torch.empty(int(_lib.load().geoa3_geo_scratch_bytes(B, N, k)), dtype=torch.uint8, device=device)


def geo_loss_grad(adv: Tensor, ori: Tensor, *, normal_ori=None, kappa_ori=None, d_ao=None, i_ao=None, d_oa=None,
                  i_oa=None, knn_adv=None, dkappa=None, k: int = 0, dis_type: int = 1, single_side: bool = False,
                  w_dis: float = 1.0, w_hd: float = 0.0, w_curv: float = 0.0, want_grad: bool = True,
                  want_kappa: bool = False, out: Optional[dict] = None, deterministic: bool = True,
                  scratch: Optional[Tensor] = None, wide_ranges: Optional[int] = None) -> dict:
    """The fused geometric objective (Attacker/geoA3_attack.py:131-166) and d constrain / d adv.
    deterministic (default): every point's gradient is summed by its owner in a fixed order -- bit-for-bit reproducible
    and independent of the rest of the batch; False: LDS float atomics (free summation order).  Clouds of up to 8192
    points; from 5840 points on the sums are order-free whatever `deterministic` says.
    wide_ranges (tests, tools): the two-pass kernels of those sizes on this cloud, 64..8192 points, with that many owner
    ranges per instance (geoa3_debug_geo_wide; 0 = the dispatcher's choice)."""
    B, _, N = adv.shape
    dev = adv.device
    o = out if out is not None else {}
    for name in ("dis_loss", "hd_loss", "curv_loss", "constrain"):
        if name not in o:
            o[name] = torch.empty(B, device=dev, dtype=torch.float32)
    if want_grad and "grad" not in o:
        o["grad"] = torch.empty(B, 3, N, device=dev, dtype=torch.float32)
    if want_kappa and "kappa_adv" not in o:
        o["kappa_adv"] = torch.empty(B, N, device=dev, dtype=torch.float32)
    if wide_ranges is not None:
        scratch = torch.empty(int(_lib.load().geoa3_debug_geo_wide_scratch_bytes(B, N)), dtype=torch.uint8, device=dev)
    elif scratch is None and (deterministic or not want_grad) and (1024 < N or k > 32) and N <= 4096 and knn_adv is not None:
        scratch = geo_scratch(B, N, dev, k)   # (callers in a loop hand over their own: AttackRunner)
    elif scratch is None and GEO_WIDE_MIN_N <= N <= 8192:   # the two-pass kernels, with or without the curvature term
        scratch = geo_scratch(B, N, dev, k)
    elif scratch is False:                    # tests: the one-workgroup kernel
        scratch = None
    a = GeoArgs(adv=_p(adv, torch.float32), ori=_p(ori, torch.float32), normal_ori=_p(normal_ori),
                kappa_ori=_p(kappa_ori), d_ao=_p(d_ao), i_ao=_p(i_ao, torch.int32) if i_ao is not None else None,
                d_oa=_p(d_oa), i_oa=_p(i_oa, torch.int32) if i_oa is not None else None,
                knn_adv=_p(knn_adv, torch.int32) if knn_adv is not None else None, dkappa=_p(dkappa),
                B=B, N=N, k=k, Nr=int(ori.shape[2]), dis_type=dis_type, single_side=int(single_side), w_dis=w_dis, w_hd=w_hd,
                w_curv=w_curv, dis_loss=_p(o["dis_loss"]), hd_loss=_p(o["hd_loss"]), curv_loss=_p(o["curv_loss"]),
                constrain=_p(o["constrain"]), kappa_adv=_p(o.get("kappa_adv")) if want_kappa else None,
                grad=_p(o["grad"]) if want_grad else None, deterministic=int(bool(deterministic)),
                scratch=_p(scratch))
    if wide_ranges is not None:
        check(_lib.load().geoa3_debug_geo_wide(C.byref(a), int(wide_ranges), _stream()), "geoa3_debug_geo_wide")
    else:
        check(_lib.load().geoa3_geo_loss_grad(C.byref(a), _stream()), "geoa3_geo_loss_grad")
    return o


UNIFORM_PERCENTAGES = (0.004, 0.006, 0.008, 0.010, 0.012)   # uniform_loss's defaults, Lib/loss_utils.py:151


def uniform_workspace(B: int, N: int, device) -> Tensor:
    """Workspace of geoa3_uniform_loss for [B,3,N] clouds."""
    return torch.empty(int(_lib.load().geoa3_uniform_loss_workspace_bytes(B, N)), dtype=torch.uint8, device=device)


def uniform_loss(pc: Tensor, percentages=UNIFORM_PERCENTAGES, radius: float = 1.0, k: int = 2,
                 contract: Optional[bool] = None, workspace: Optional[Tensor] = None, out=None, want_idx: bool = False):
    """The uniformity term of Lib/loss_utils.py:151-189 on pc [B,3,N] (planar) -> (U [] float32 -- one scalar for the
    batch --, dU/dpc [B,3,N]); with want_idx also the sampler's indices [B,npoint] and the ball-query rows (a list of
    [B,npoint,nsample_p], one per percentage).  contract: the sampler's and the ball queries' distances as
    GEOA3_PN2_CONTRACT (None = the choice of geoa3_amd.pointnet2.ext_contract_default)."""
    from .pointnet2 import _ext_flags
    B, _, N = pc.shape
    pcts = [float(p) for p in percentages]
    if out is None:
        out = (torch.empty((), device=pc.device, dtype=torch.float32),
               torch.empty(B, 3, N, device=pc.device, dtype=torch.float32))
    loss, grad = out
    if workspace is None:
        workspace = uniform_workspace(B, N, pc.device)
    fps_idx = group_idx = None
    npoint = int(N * 0.05)
    ns = [int(N * (p * 4)) for p in pcts]
    if want_idx:
        fps_idx = torch.empty(B, max(npoint, 1), device=pc.device, dtype=torch.int32)
        group_idx = torch.empty(B * max(npoint, 1) * max(sum(ns), 1), device=pc.device, dtype=torch.int32)
    arr = (C.c_double * max(len(pcts), 1))(*pcts)
    check(_lib.load().geoa3_uniform_loss(_p(pc, torch.float32), B, N, arr, len(pcts), float(radius), int(k),
                                         _ext_flags(contract), _p(loss), _p(grad), _p(fps_idx), _p(group_idx),
                                         _p(workspace), _stream()), "geoa3_uniform_loss")
    if not want_idx:
        return loss, grad
    rows, o = [], 0
    for n in ns:
        rows.append(group_idx[o:o + B * npoint * n].view(B, npoint, n))
        o += B * npoint * n
    return loss, grad, fps_idx, rows


def uniform_fold(loss: Tensor, grad: Optional[Tensor], scale_const: Optional[Tensor], w: float, B: int, N: int,
                 constrain: Optional[Tensor] = None, constrain_add: bool = False, g: Optional[Tensor] = None,
                 g_add: bool = False, stream: Optional[int] = None) -> None:
    """geoa3_uniform_fold: constrain (+)= w U; g (+)= w (sum_b scale_const[b] / B) dU (geoA3_attack.py:171,176-178)."""
    check(_lib.load().geoa3_uniform_fold(_p(loss), _p(grad), _p(scale_const), float(w), B, N, _p(constrain),
                                         int(constrain_add), _p(g), int(g_add),
                                         _stream() if stream is None else stream), "geoa3_uniform_fold")


# ---------------------------------------------------------------------------------------------
# Neighbour-based regularisers (csrc/geom_reg.hip): kNN_smoothing_loss / repulsion_loss / displacement_loss /
# corresponding_normal_loss of Lib/loss_utils.py:99-149.  `knn` = (dists, idx) [B,N,K >= k+1] of geoa3_knn_self on the
# cloud the table belongs to (displacement_loss: ori); None: the entry point computes it into `workspace`.
# ---------------------------------------------------------------------------------------------
def reg_workspace(B: int, N: int, k: int, device) -> Tensor:
    """Workspace of the geoa3_*_loss(_grad) entry points of csrc/geom_reg.hip for [B,3,N] clouds."""
    return torch.empty(max(int(_lib.load().geoa3_reg_workspace_bytes(B, N, int(k))), 256), dtype=torch.uint8, device=device)


def _reg_table(knn, B: int, N: int, k: int):
    if knn is None:
        return None, None, 0
    d, i = knn
    if d.dim() != 3 or tuple(d.shape) != tuple(i.shape) or d.shape[0] != B or d.shape[1] != N or d.shape[2] < k + 1:
        raise _lib.Geoa3Error("knn must be (dists, idx) of shape [%d,%d,K >= %d]" % (B, N, k + 1))
    return _p(d, torch.float32), _p(i, torch.int32), int(d.shape[2])


def _reg_ws(workspace, B, N, k, device):
    return workspace if workspace is not None else reg_workspace(B, N, k, device)


def knn_smoothing_loss(pc: Tensor, k: int, threshold_coef: float = 1.05, knn=None, workspace: Optional[Tensor] = None,
                       out=None, want_cond: bool = False):
    """kNN_smoothing_loss (Lib/loss_utils.py:135-149) on pc [B,3,N] -> loss [B] (with want_cond: also the mask [B,N] uint8)."""
    B, _, N = pc.shape
    loss = out if out is not None else torch.empty(B, device=pc.device, dtype=torch.float32)
    cond = torch.empty(B, N, device=pc.device, dtype=torch.uint8) if want_cond else None
    d, i, ld = _reg_table(knn, B, N, int(k))
    check(_lib.load().geoa3_knn_smoothing_loss(_p(pc, torch.float32), B, N, int(k), float(threshold_coef), d, i, ld,
                                               _p(loss, torch.float32), _p(cond), _p(_reg_ws(workspace, B, N, k, pc.device)),
                                               _stream()), "geoa3_knn_smoothing_loss")
    return (loss, cond) if want_cond else loss


def knn_smoothing_loss_grad(pc: Tensor, k: int, threshold_coef: float = 1.05, g: Optional[Tensor] = None, knn=None,
                            workspace: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """d (sum_b g_b loss_b) / d pc [B,3,N] (g [B]; None = ones)."""
    B, _, N = pc.shape
    grad = out if out is not None else torch.empty(B, 3, N, device=pc.device, dtype=torch.float32)
    d, i, ld = _reg_table(knn, B, N, int(k))
    check(_lib.load().geoa3_knn_smoothing_loss_grad(_p(pc, torch.float32), B, N, int(k), float(threshold_coef), d, i, ld,
                                                    _p(g, torch.float32), _p(grad, torch.float32),
                                                    _p(_reg_ws(workspace, B, N, k, pc.device)), _stream()),
          "geoa3_knn_smoothing_loss_grad")
    return grad


def repulsion_loss(pc: Tensor, k: int = 4, h: float = 0.03, knn=None, workspace: Optional[Tensor] = None,
                   out: Optional[Tensor] = None) -> Tensor:
    """repulsion_loss (Lib/loss_utils.py:119-123) on pc [B,3,N] -> [B,N]."""
    B, _, N = pc.shape
    o = out if out is not None else torch.empty(B, N, device=pc.device, dtype=torch.float32)
    d, i, ld = _reg_table(knn, B, N, int(k))
    check(_lib.load().geoa3_repulsion_loss(_p(pc, torch.float32), B, N, int(k), float(h), d, i, ld, _p(o, torch.float32),
                                           _p(_reg_ws(workspace, B, N, k, pc.device)), _stream()), "geoa3_repulsion_loss")
    return o


def repulsion_loss_grad(pc: Tensor, k: int = 4, h: float = 0.03, g: Optional[Tensor] = None, knn=None,
                        workspace: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """d (sum g . out) / d pc [B,3,N] (g [B,N]; None = ones)."""
    B, _, N = pc.shape
    grad = out if out is not None else torch.empty(B, 3, N, device=pc.device, dtype=torch.float32)
    d, i, ld = _reg_table(knn, B, N, int(k))
    check(_lib.load().geoa3_repulsion_loss_grad(_p(pc, torch.float32), B, N, int(k), float(h), d, i, ld,
                                                _p(g, torch.float32), _p(grad, torch.float32),
                                                _p(_reg_ws(workspace, B, N, k, pc.device)), _stream()),
          "geoa3_repulsion_loss_grad")
    return grad


def displacement_loss(adv: Tensor, ori: Tensor, k: int = 16, knn=None, workspace: Optional[Tensor] = None,
                      out: Optional[Tensor] = None) -> Tensor:
    """displacement_loss (Lib/loss_utils.py:99-107) on adv, ori [B,3,N] -> [B,N]; knn: the table of ORI."""
    B, _, N = adv.shape
    if tuple(ori.shape) != (B, 3, N):
        raise _lib.Geoa3Error("displacement_loss: adv and ori must have the same shape")
    o = out if out is not None else torch.empty(B, N, device=adv.device, dtype=torch.float32)
    d, i, ld = _reg_table(knn, B, N, int(k))
    check(_lib.load().geoa3_displacement_loss(_p(adv, torch.float32), _p(ori, torch.float32), B, N, int(k), d, i, ld,
                                              _p(o, torch.float32), _p(_reg_ws(workspace, B, N, k, adv.device)), _stream()),
          "geoa3_displacement_loss")
    return o


def displacement_loss_grad(adv: Tensor, ori: Tensor, k: int = 16, g: Optional[Tensor] = None, knn=None,
                           workspace: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """d (sum g . out) / d adv [B,3,N] (g [B,N]; None = ones)."""
    B, _, N = adv.shape
    if tuple(ori.shape) != (B, 3, N):
        raise _lib.Geoa3Error("displacement_loss: adv and ori must have the same shape")
    grad = out if out is not None else torch.empty(B, 3, N, device=adv.device, dtype=torch.float32)
    d, i, ld = _reg_table(knn, B, N, int(k))
    check(_lib.load().geoa3_displacement_loss_grad(_p(adv, torch.float32), _p(ori, torch.float32), B, N, int(k), d, i, ld,
                                                   _p(g, torch.float32), _p(grad, torch.float32),
                                                   _p(_reg_ws(workspace, B, N, k, adv.device)), _stream()),
          "geoa3_displacement_loss_grad")
    return grad


def _reg_check(B: int, N: int, k: int) -> None:
    if k < 1 or N < k + 1:
        raise _lib.Geoa3Error("corresponding_normal_loss failed: invalid argument (k = %d, N = %d)" % (k, N))
    if k + 1 > 64 or N > 8192:
        raise _lib.Geoa3Error("corresponding_normal_loss failed: not supported (k + 1 <= 64, N <= 8192)")


def _instance_bad(pc: Tensor) -> Tensor:
    return ~torch.isfinite(pc).flatten(1).all(1)


def corresponding_normal_loss(adv: Tensor, normal: Tensor, k: int = 2, knn=None, want_knn: bool = False):
    """corresponding_normal_loss (Lib/loss_utils.py:109-117) on adv, normal [B,3,N] -> [B,N]: geoa3_kappa on adv's own
    K-NN with the point's own normal.  want_knn: also the index table [B,N,k+1] the backward needs."""
    B, _, N = adv.shape
    _reg_check(B, N, int(k))
    idx = knn[1][:, :, :k + 1].contiguous() if knn is not None else knn_self_planar(adv, int(k) + 1)[1]
    # a point with a non-finite coordinate has no neighbours (index -1, which geoa3_kappa does not follow: that point's
    # value is NaN): the whole instance is NaN, as in the kernels of csrc/geom_reg.hip
    out = kappa(adv, normal, idx)
    out = torch.where(_instance_bad(adv).view(B, 1), out.new_full((), float("nan")), out)
    return (out, idx) if want_knn else out


def corresponding_normal_loss_grad(adv: Tensor, normal: Tensor, knn_idx: Tensor, g: Optional[Tensor] = None) -> Tensor:
    """d (sum g . out) / d adv [B,3,N]: the dkappa path of geoa3_geo_loss_grad with the identity as nearest-point index."""
    B, _, N = adv.shape
    k = int(knn_idx.shape[2]) - 1
    _reg_check(B, N, k)
    ident = torch.arange(N, device=adv.device, dtype=torch.int32).unsqueeze(0).expand(B, N).contiguous()
    if g is None:
        g = torch.ones(B, N, device=adv.device, dtype=torch.float32)
    o = geo_loss_grad(adv, adv, normal_ori=normal, i_ao=ident, knn_adv=knn_idx, dkappa=g.contiguous(), k=k, dis_type=0,
                      w_dis=0.0, w_hd=0.0, w_curv=0.0, deterministic=True)
    return torch.where(_instance_bad(adv).view(B, 1, 1), o["grad"].new_full((), float("nan")), o["grad"])


def corr_normal_loss_grad(pc: Tensor, normal: Tensor, k: int = 2, g: Optional[Tensor] = None, knn=None,
                          workspace: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """geoa3_corr_normal_loss_grad: d (sum g . corresponding_normal_loss) / d pc [B,3,N] with every pair term formed in
    double (g [B,N]; None = ones); the attack loop's gradient of the term."""
    B, _, N = pc.shape
    if tuple(normal.shape) != (B, 3, N):
        raise _lib.Geoa3Error("corr_normal_loss_grad: pc and normal must have the same shape")
    grad = out if out is not None else torch.empty(B, 3, N, device=pc.device, dtype=torch.float32)
    d, i, ld = _reg_table(knn, B, N, int(k))
    check(_lib.load().geoa3_corr_normal_loss_grad(_p(pc, torch.float32), _p(normal, torch.float32), B, N, int(k), d, i, ld,
                                                  _p(g, torch.float32), _p(grad, torch.float32),
                                                  _p(_reg_ws(workspace, B, N, k, pc.device)), _stream()),
          "geoa3_corr_normal_loss_grad")
    return grad


def reg_fold(loss: Optional[Tensor], grad: Optional[Tensor], w: float, B: int, N: int, constrain: Optional[Tensor] = None,
             constrain_add: bool = False, g: Optional[Tensor] = None, g_add: bool = False,
             stream: Optional[int] = None) -> None:
    """geoa3_reg_fold: constrain (+)= w loss [B]; g (+)= w grad [B,3,N]."""
    check(_lib.load().geoa3_reg_fold(_p(loss), _p(grad), float(w), B, N, _p(constrain), int(constrain_add), _p(g),
                                     int(g_add), _stream() if stream is None else stream), "geoa3_reg_fold")


def reg_fold_points(out: Optional[Tensor], grad: Optional[Tensor], w: float, B: int, N: int, term: Optional[Tensor] = None,
                    constrain: Optional[Tensor] = None, constrain_add: bool = False, g: Optional[Tensor] = None,
                    g_add: bool = False, stream: Optional[int] = None) -> None:
    """geoa3_reg_fold_points: term [B] = mean_i out [B,N]; constrain (+)= w term; g (+)= (w / N) grad [B,3,N], grad being
    d (sum_i out) / d cloud (the *_grad entry points with g = None)."""
    for name, x, numel in (("out", out, B * N), ("grad", grad, B * 3 * N), ("term", term, B), ("constrain", constrain, B),
                           ("g", g, B * 3 * N)):
        if x is not None and x.numel() != numel:
            raise _lib.Geoa3Error("reg_fold_points: %s holds %d elements, expected %d" % (name, x.numel(), numel))
    check(_lib.load().geoa3_reg_fold_points(_p(out, torch.float32), _p(grad, torch.float32), float(w), B, N,
                                            _p(term, torch.float32), _p(constrain, torch.float32), int(constrain_add),
                                            _p(g, torch.float32), int(g_add), _stream() if stream is None else stream),
          "geoa3_reg_fold_points")


# ---------------------------------------------------------------------------------------------
# Operator-level mirror of pytorch3d.ops: [b,n,D] point-major arguments (1 <= D <= 128), int64 idx,
# differentiable through `dists`.
# ---------------------------------------------------------------------------------------------
_KNN = collections.namedtuple("KNN", ["dists", "idx", "knn"])


def _check_lengths(name: str, lengths, b: int, n: int) -> None:
    """Ragged batches are not supported: a `lengths` argument must say that every cloud is full."""
    if lengths is None:
        return
    t = torch.as_tensor(lengths)
    if t.numel() != b or not bool((t.reshape(-1) == n).all()):
        raise _lib.Geoa3Error("knn_points: %s must be None or %d for each of the %d clouds (ragged batches are not "
                              "supported)" % (name, n, b))


def knn_points(p1: Tensor, p2: Tensor, K: int = 1, return_nn: bool = False, lengths1=None, lengths2=None, **_ignored):
    """pytorch3d.ops.knn_points(p1 [b,n1,D], p2 [b,n2,D], K) -> KNN(dists, idx, knn).  D == 3: the pruned searches of the
    attack loop; any other 1 <= D <= 128 (n1, n2 <= 8192, K <= min(n2, 64)): geoa3_knn_nd, whose distance is the sequential
    float32 sum over d and whose ties go to the lower index.  The gradient through `dists` is summed per point in ascending
    (query, neighbour) order (D == 3: geoa3_knn_points_grad; else the ordered knn_gather backward): the same bits on every
    run.  return_nn: knn = knn_gather(p2, idx) [b,n1,K,D], differentiable in p2 (None otherwise).  lengths1 / lengths2
    other than None or all-full raise Geoa3Error."""
    from . import library  # noqa: F401  (registers geoa3::knn_points with its autograd formula)
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[2] != p2.shape[2] or p1.shape[0] != p2.shape[0]:
        raise _lib.Geoa3Error("knn_points: p1 %s and p2 %s must be [b,n1,D] and [b,n2,D]" % (tuple(p1.shape), tuple(p2.shape)))
    _check_lengths("lengths1", lengths1, p1.shape[0], p1.shape[1])
    _check_lengths("lengths2", lengths2, p2.shape[0], p2.shape[1])
    d, idx = torch.ops.geoa3.knn_points(p1, p2, int(K))
    knn = None
    if return_nn:   # (the search has no CPU kernel: whatever got here is a device tensor, or a fake one of any device)
        knn = torch.ops.geoa3.knn_gather(p2, idx) if p2.dtype == torch.float32 else knn_gather(p2, idx)
    return _KNN(d, idx, knn)


def knn_gather(x: Tensor, idx: Tensor) -> Tensor:
    """pytorch3d.ops.knn_gather(x [b,m,u], idx [b,l,k]) -> [b,l,k,u] (pure data movement).  float32 device tensors: the
    library's gather (geoa3::knn_gather), whose gradient sums every row of x in ascending (l, k) order; anything else:
    torch.gather."""
    if x.is_cuda and idx.is_cuda and x.dtype == torch.float32 and idx.dtype == torch.int64 and x.dim() == 3 and idx.dim() == 3:
        from . import library  # noqa: F401
        return torch.ops.geoa3.knn_gather(x, idx)
    b, m, u = x.shape
    _, l, k = idx.shape
    return torch.gather(x, 1, idx.reshape(b, l * k, 1).expand(b, l * k, u)).view(b, l, k, u)


def knn_scatter_scratch(B: int, E: int, M: int, device) -> Tensor:
    """Scratch of knn_gather_grad / knn_points_grad for B instances of E entries that point into M rows."""
    nbytes = int(_lib.load().geoa3_knn_scatter_scratch_bytes(B, E, M))
    if nbytes < 0:
        raise _lib.Geoa3Error("knn scatter: sizes out of range (B=%d, entries=%d, rows=%d)" % (B, E, M))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def knn_gather_fwd(x: Tensor, idx: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """geoa3_knn_gather: x [B,M,U] float32, idx int64 [B,L,K] -> [B,L,K,U]; an index outside [0,M) gives NaN."""
    B, M, U = x.shape
    _, L, K = idx.shape
    if out is None:
        out = torch.empty(B, L, K, U, device=x.device, dtype=torch.float32)
    if out.numel():
        check(_lib.load().geoa3_knn_gather(_p(x, torch.float32), _p(idx, torch.int64), B, M, L, K, U, _p(out, torch.float32),
                                           _stream()), "geoa3_knn_gather")
    return out


def knn_gather_grad(g: Tensor, idx: Tensor, M: int, scratch: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """geoa3_knn_gather_grad: g [B,L,K,U] float32, idx int64 [B,L,K] -> gx [B,M,U], row j the sequential float32 sum of
    the g[b,l,k,:] with idx[b,l,k] == j in ascending l K + k (indices outside [0,M) dropped)."""
    B, L, K, U = g.shape
    if out is None:
        out = torch.empty(B, M, U, device=g.device, dtype=torch.float32)
    if g.numel() == 0:
        return out.zero_()
    if out.numel():
        if scratch is None:
            scratch = knn_scatter_scratch(B, L * K, M, g.device)
        check(_lib.load().geoa3_knn_gather_grad(_p(g, torch.float32), _p(idx, torch.int64), B, M, L, K, U,
                                                _p(out, torch.float32), _p(scratch), _stream()), "geoa3_knn_gather_grad")
    return out


def knn_points_grad(p1: Tensor, p2: Tensor, idx: Tensor, gd: Tensor, want1: bool = True, want2: bool = True,
                    scratch: Optional[Tensor] = None, out=None):
    """geoa3_knn_points_grad: p1 [B,N1,3], p2 [B,N2,3] float32, idx int64 / gd float32 [B,N1,K] -> (g1 [B,N1,3] | None,
    g2 [B,N2,3] | None): pytorch3d's knn backward, every point's terms added in ascending (query, neighbour) order."""
    B, N1, _ = p1.shape
    N2 = p2.shape[1]
    K = idx.shape[2]
    g1, g2 = out if out is not None else (None, None)
    if want1 and g1 is None:
        g1 = torch.empty(B, N1, 3, device=p1.device, dtype=torch.float32)
    if want2 and g2 is None:
        g2 = torch.empty(B, N2, 3, device=p1.device, dtype=torch.float32)
    if want2 and scratch is None:
        scratch = knn_scatter_scratch(B, N1 * K, N2, p1.device)
    check(_lib.load().geoa3_knn_points_grad(_p(p1, torch.float32), _p(p2, torch.float32), _p(idx, torch.int64),
                                            _p(gd, torch.float32), B, N1, N2, K, _p(g1, torch.float32) if want1 else None,
                                            _p(g2, torch.float32) if want2 else None, _p(scratch) if want2 else None,
                                            _stream()), "geoa3_knn_points_grad")
    return (g1 if want1 else None), (g2 if want2 else None)
