"""Driver-level boundary: ``attack(net, input_data, cfg, i, loader_len, saved_dir)`` with the
reference's signature, return tuple and semantics (Attacker/geoA3_attack.py:182-386), as a device-resident
loop: every inner iteration is seven enqueues into the HIP library and ZERO host synchronisations (the
reference does ~15 000 tiny launches and ~760 ``.item()`` syncs per iteration at b=250).

Reference quirks kept on purpose:
  * the success check of step s ranks the CURRENT iterate with the constrain loss of step s-1
    (1e10 at step 0), geoA3_attack.py:301;
  * the binary search compares the label of the LAST instance at the LAST step against every
    instance's target (geoA3_attack.py:298,375);
  * ``loss = loss_n.mean()`` scales every gradient by 1/b (geoA3_attack.py:178) -- the GLOBAL b when the batch
    is sharded over GPUs, so shards reproduce the single-GPU iterates.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from ._lib import AttackState, check
from .pointnet import PointNet

Tensor = torch.Tensor


def _cfg(cfg, name, default):
    return getattr(cfg, name, default)


def knn_table_plan(use_curv, k, w_disp, k_disp, w_rep, k_rep, w_cn, k_cn, w_knn, ks, knn_share_table=True,
                   reg_share_table=True):
    """Which neighbour table each active neighbour term reads and how many columns it has: ({term: (table, columns)},
    geoa3_knn_self launches per iteration).  Terms: "knn" (kNN smoothing), "disp", "rep", "cn".  Tables: "curv" the curvature
    term's (of this iteration's iterate; for "disp" the clean cloud's, built with it once per batch), whose first columns
    hold the nearer neighbours of any narrower term; "own" the smoothing term's own search; "reg" the ONE search the
    repulsion and normal terms share; "clean" the displacement term's own table of the clean cloud, once per batch.
    The *_share_table switches (tests) refuse the curvature term's table."""
    curv, plan = ("curv", k + 1), {}
    if w_knn != 0:
        plan["knn"] = curv if use_curv and ks <= k and knn_share_table else ("own", ks + 1)
    if w_disp != 0:
        plan["disp"] = curv if use_curv and k_disp <= k else ("clean", k_disp + 1)
    if w_rep != 0 or w_cn != 0:
        kmax = max(k_rep if w_rep != 0 else 1, k_cn if w_cn != 0 else 1)
        reg = curv if use_curv and kmax <= k and reg_share_table else ("reg", kmax + 1)
        plan.update({term: reg for term, w in (("rep", w_rep), ("cn", w_cn)) if w != 0})
    return plan, int(use_curv) + len({table for table, _ in plan.values() if table in ("own", "reg")})


class _SelfKnnTable:
    """A self-K-NN table of the iterate, searched once per iteration: double-buffered, last iteration's table being the
    prior of this one's search.  The buffers live in the runner's t under prefix + "knn" / "knn_d" / "scratch"."""

    def __init__(self, t: dict, prefix: str, b: int, ne: int, cols: int, device, method: int = 0):
        self.b, self.ne, self.cols, self.method = b, ne, cols, method   # method: geoa3_knn_self's, 0 = by (K, N)
        self.idx = t[prefix + "knn"] = [torch.zeros(b, ne, cols, device=device, dtype=torch.int32) for _ in range(2)]
        self.d = t[prefix + "knn_d"] = torch.zeros(b, ne, cols, device=device, dtype=torch.float32)
        # the searches of an iteration follow each other on one stream: the curvature term's scratch, when there is one,
        # serves the other tables too
        self.scratch = t[(prefix or "knn_") + "scratch"] = (t["knn_scratch"] if "knn_scratch" in t
                                                            else ops.knn_self_scratch(b, ne, device))
        self.knn_self = _lib.load().geoa3_knn_self      # looked up, like the buffers' addresses, once
        self.ptrs = [x.data_ptr() for x in (*self.idx, self.d, self.scratch)]

    def reset(self, clean_idx: Optional[Tensor]):
        """A new batch: the clean cloud's table [b,ne,cols] is the first prior (None: the first search has none)."""
        self.cur, self.seeded = 0, clean_idx is not None
        if self.seeded:
            self.idx[0].copy_(clean_idx)

    def search(self, xe: Tensor, stream: int):
        """-> (dists [b,ne,cols], idx, cols) of xe, enqueued on stream"""
        prior, out = self.ptrs[self.cur] if self.seeded else None, self.ptrs[1 - self.cur]
        check(self.knn_self(xe.data_ptr(), self.b, self.ne, self.cols, prior, self.ptrs[2], out, self.ptrs[3],
                            self.method, stream), "knn_self")
        self.seeded, self.cur = True, 1 - self.cur
        return self.d, self.idx[self.cur], self.cols


class AttackRunner:
    """Owns the device state of one batch of b attacks in flight and enqueues the loop."""

    def __init__(self, net: PointNet, b: int, n: int, cfg, device, global_batch: Optional[int] = None,
                 ne: Optional[int] = None, geo_n: Optional[int] = None):
        # ne, geo_n (a subclass whose variable is not the cloud itself, geoa3_amd/mesh_attack.py): the points of the cloud
        # the objective is evaluated on, and of the clean cloud the geometry stages compare it with.  Default: derived
        # from n as below, and n.
        # --uniform_loss_weight (geoA3_attack.py:168-174): w * U joins every row's constrain loss; U is ONE scalar for the
        # batch (Lib/loss_utils.py:151-189), so its gradient couples the rows -- a sharded batch would need an all-reduce
        self.w_uni = float(_cfg(cfg, "uniform_loss_weight", 0.0))
        if self.w_uni != 0 and global_batch is not None and global_batch != b:
            raise ValueError("uniform_loss_weight != 0 needs the whole batch on one GPU: U is a mean over all %d "
                             "instances (this shard holds %d)" % (global_batch, b))
        # --is_use_knn_smoothing_loss (an extension: the reference parses --knn_smoothing_loss_weight / --knn_smoothing_k /
        # --knn_threshold_coef, main_attack.py:52-54, and never reads them): w * kNN_smoothing_loss(x, k, coef)
        # (Lib/loss_utils.py:135-149) joins every row's constrain loss.  Per row: a sharded batch needs nothing.
        self.w_knn = (float(_cfg(cfg, "knn_smoothing_loss_weight", 0.0))
                      if bool(_cfg(cfg, "is_use_knn_smoothing_loss", False)) else 0.0)
        if cfg.dis_loss_type == "L2" and cfg.hd_loss_weight != 0:
            raise AssertionError("L2 distance needs hd_loss_weight == 0")  # geoA3_attack.py:140
        if cfg.optim not in ("adam", "sgd"):
            raise AssertionError("Not support such optimizer.")
        self.net, self.cfg, self.b, self.n, self.dev = net, cfg, b, n, device
        self.lib = _lib.load()
        # Native victims, whose forward / input-gradient live in the HIP library: the PointNet, and the PointNet++ SSG
        # classifier of geoa3_amd/pointnet2.py in eval mode on xyz only (geoa3_pn2ssg_forward / _backward,
        # csrc/pointnet2_net.hip).  Any other eval-mode nn.Module is driven through torch autograd:
        # logits = net(x); logits.backward(dlogits) -- still no host synchronisation.
        from .pointnet2 import PointNet2ClassificationSSG
        self.ssg = (isinstance(net, PointNet2ClassificationSSG) and not net.training and not net.use_normal and
                    (min(n, int(_cfg(cfg, "npoint", n))) if ne is None else ne) >= PointNet2ClassificationSSG.MIN_POINTS)
        self.native = isinstance(net, PointNet) or self.ssg
        if self.native:
            self.packed = net.packed(device)
            self.classes = self.packed.classes
        else:
            self.packed = None
            self.classes = int(_cfg(cfg, "classes", 40))
            # only d/d input is needed (the reference also forms the unused weight gradients: its parameters keep
            # requires_grad=True): the flags are cleared for the duration of run() and restored after it
            self._grad_flags = None
        self.global_batch = global_batch or b
        self.targeted = cfg.attack_label != "Untarget"
        self.k = int(cfg.curv_loss_knn)
        self.use_curv = cfg.curv_loss_weight != 0
        self.dis_type = {"CD": 1, "L2": 2, "None": 0}[cfg.dis_loss_type]
        self.need_nn = self.dis_type == 1 or cfg.hd_loss_weight != 0 or self.use_curv
        self.geo_runs = self.need_nn or self.dis_type == 2     # the geometric objective runs at all: L2 needs no 1-NN
        self.both = self.dis_type == 1 and not cfg.is_cd_single_side      # two-sided Chamfer: the clean cloud's 1-NN too
        self.iters = int(cfg.iter_max_steps)
        # the objective's gradient summed in a fixed order (geoa3_geo_args.deterministic): iterates are reproducible bit
        # for bit and shard rows equal the full batch's; cfg.deterministic / GEOA3_DETERMINISTIC=0 select the atomics
        self.deterministic = bool(_cfg(cfg, "deterministic", os.environ.get("GEOA3_DETERMINISTIC", "1") != "0"))
        # Dense-cloud path (geoA3_attack.py:283-296): the offset lives on all n points, the objective sees the
        # farthest-point sample of cfg.npoint of them, success is a vote over eval_num resamplings.
        self.npoint = int(_cfg(cfg, "npoint", n))
        # --is_partial_var (geoA3_attack.py:239-262): a [b,3,knn_range] offset on the neighbours of one random clean
        # point, re-drawn (with a fresh optimiser) every 50 steps on top of the iterate reached so far
        self.partial = bool(_cfg(cfg, "is_partial_var", False))
        self.kr = int(_cfg(cfg, "knn_range", 3))
        self.sub = bool(_cfg(cfg, "is_subsample_opt", False)) and n > self.npoint and not self.partial
        self.ne = (self.npoint if self.sub else n) if ne is None else int(ne)   # points the objective is evaluated on
        self.geo_n = n if geo_n is None else int(geo_n)   # points of the clean cloud of the geometry stages (geo_ori)
        self.eval_num = int(_cfg(cfg, "eval_num", 1))
        if self.sub and not 1 <= self.eval_num <= 64:
            raise ValueError("eval_num must be in 1..64")
        # --is_pre_jitter_input (geoA3_attack.py:312-317): the objective is evaluated at x + tangent-plane noise
        self.jitter = bool(_cfg(cfg, "is_pre_jitter_input", False))
        self.hooks = {}
        # The geometry kernels of an iteration (1-NN, K-NN, losses: VALU / latency bound) do not depend on the victim's
        # forward (MFMA / HBM bound): they are enqueued on a second HIP stream between two events, so the hardware
        # runs them beside it (GEOA3_GEO_STREAM=0: everything on the current stream).  Same kernels, same results.
        # Measured: 2.78 -> 2.72 ms/iteration (N = 4096: 12.7 -> 11.7); joining only after the backward (head without
        # the constrain loss, added afterwards) gained nothing more: the kernels slow each other down.
        self.geo_stream = (torch.cuda.Stream(device=device)
                           if os.environ.get("GEOA3_GEO_STREAM", "1") != "0" and torch.device(device).type == "cuda"
                           else None)
        self.ev_x, self.ev_geo = ((torch.cuda.Event(), torch.cuda.Event()) if self.geo_stream is not None
                                  else (None, None))
        # Small shards (the 32-instance regime of an 8-GPU split) are latency bound: there the geometry chain is as long
        # as the forward, so the head is split (geoa3_attack_head_classify / _finish) and the geometry stream is joined
        # only AFTER the victim's backward.  At 250 instances the kernels are throughput bound and the late join gains
        # nothing (measured), so it is taken for b <= 96 (cfg.late_join overrides).  Same results.
        lj = _cfg(cfg, "late_join", None)           # (tests: cfg.late_join = True / False)
        self.late_join = (b <= 96) if lj is None else bool(lj)
        # the 1-NN tables through the pruned searches (geom_grid.hip / geom_filter.hip; same bits as the all-pairs kernel,
        # which stays the path for clouds of fewer than 32 points or when cfg.brute_force_nn1 is set)
        self.grid_nn1 = min(self.geo_n, self.ne) >= 32 and not _cfg(cfg, "brute_force_nn1", False)
        # (tools: GEOA3_NN1_POLICY="brute_frac,filter" runs the loop's searches through geoa3_debug_grid_nn1_pair -- same
        # bits, another split between grid walk, in-kernel sweep and filter search: include/geoa3_hip_debug.h)
        pol = os.environ.get("GEOA3_NN1_POLICY")
        self.nn1_policy = (float(pol.split(",")[0]), int(pol.split(",")[1])) if pol else None
        ne = self.ne
        f32 = dict(device=device, dtype=torch.float32)
        i32 = dict(device=device, dtype=torch.int32)
        z = lambda *s: torch.zeros(*s, **f32)
        self.t = t = {}
        for name in ("offset", "m", "v", "x"):
            t[name] = z(b, 3, n)
        for name in ("g_cls", "g_geo"):
            t[name] = z(b, 3, ne)
        if self.sub:
            E = self.eval_num
            t["g_cls_full"], t["g_geo_full"], t["x_cur"] = z(b, 3, n), z(b, 3, n), z(b, 3, ne)
            t["sub_idx"] = torch.zeros(b, ne, **i32)
            t["vote_idx"], t["vote_pts"] = torch.zeros(b * E, ne, **i32), z(b * E, 3, ne)
            t["vote_logits"] = z(b * E, self.classes)
        if self.partial:
            t["part"], t["pm"], t["pv"] = z(b, 3, self.kr), z(b, 3, self.kr), z(b, 3, self.kr)
            t["pidx"], t["periodical"] = torch.zeros(b, self.kr, **i32), z(b, 3, n)
        if self.jitter:
            t["noise"], t["x_eval"] = z(b, 3, ne), z(b, 3, ne)
            if not self.sub:
                t["check_logits"] = z(b, self.classes)
        t["best_attack"] = torch.ones(b, 3, n, **f32)
        for name in ("scale_const", "lower", "upper", "best_loss", "iter_best_loss", "prev_constrain", "cls_loss",
                     "loss_n"):
            t[name] = z(b)
        for name in ("best_step", "best_bs", "iter_best_score", "label"):
            t[name] = torch.zeros(b, **i32)
        t["last_label"] = torch.zeros(1, **i32)
        t["ok"] = torch.zeros(b, **i32)
        t["loss_hist"] = z(self.iters, b)
        t["logits"], t["dlogits"] = z(b, self.classes), z(b, self.classes)
        t["d_ao"], t["d_oa"] = z(b, ne), z(b, self.geo_n)
        t["i_ao"], t["i_oa"] = torch.zeros(b, ne, **i32), torch.zeros(b, self.geo_n, **i32)
        if self.sub and _cfg(cfg, "is_pro_grad", False):   # the projections search with all n points
            t["proj_d"], t["proj_i"] = z(b, n), torch.zeros(b, n, **i32)
        else:
            t["proj_d"], t["proj_i"] = t["d_ao"], t["i_ao"]
        self.geo_out = {name: z(b) for name in ("dis_loss", "hd_loss", "curv_loss", "constrain")}
        if self.w_uni != 0:   # U [] and dU/dx of the cloud the objective sees (geoa3_uniform_loss)
            t["uni_loss"], t["uni_grad"] = torch.zeros((), **f32), z(b, 3, ne)
            self.uni_ws = ops.uniform_workspace(b, ne, device)
            self.uni_contract = getattr(net, "ext_contract", None)
        self.geo_out["grad"] = t["g_geo"]
        # clouds of 1025..4096 points (or k > 32): the records of the fixed-point objective kernel (geoa3_geo_args.scratch)
        # 5840..8192 points: the records and partial sums of the two-pass kernels, with or without the curvature term
        self.geo_scratch = (ops.geo_scratch(b, ne, device, self.k)
                            if (((1024 < ne or self.k > 32) and ne <= 4096 and self.use_curv)
                                or ops.GEO_WIDE_MIN_N <= ne <= 8192) else None)
        self.ks = int(_cfg(cfg, "knn_smoothing_k", 5))
        self.knn_coef = float(_cfg(cfg, "knn_threshold_coef", 1.10))
        if self.w_knn != 0 and not 1 <= self.ks < min(ne, 64):
            raise ValueError("knn_smoothing_k must be in 1..%d" % (min(ne, 64) - 1))
        # --displacement_loss_weight / --repulsion_loss_weight / --corr_normal_loss_weight (extensions): the per-point
        # regularisers of Lib/loss_utils.py:99-123 on the cloud the objective sees, each through its mean over the points
        # (as curvature_loss reduces its own, :95).  Per row: a sharded batch needs nothing.
        self.w_disp = float(_cfg(cfg, "displacement_loss_weight", 0.0))
        self.w_rep = float(_cfg(cfg, "repulsion_loss_weight", 0.0))
        self.w_cn = float(_cfg(cfg, "corr_normal_loss_weight", 0.0))
        self.k_disp = int(_cfg(cfg, "displacement_loss_knn", 16))
        self.k_rep = int(_cfg(cfg, "repulsion_loss_knn", 4))
        self.k_cn = int(_cfg(cfg, "corr_normal_loss_knn", 2))
        self.h_rep = float(_cfg(cfg, "repulsion_loss_h", 0.03))
        for w, k, name in ((self.w_disp, self.k_disp, "displacement_loss_knn"), (self.w_rep, self.k_rep, "repulsion_loss_knn"),
                           (self.w_cn, self.k_cn, "corr_normal_loss_knn")):
            if w != 0 and not 1 <= k < min(ne, 64):
                raise ValueError("%s must be in 1..%d" % (name, min(ne, 64) - 1))
        if self.w_rep != 0 and not self.h_rep > 0:
            raise ValueError("repulsion_loss_h must be positive")
        if self.sub and (self.w_disp != 0 or self.w_cn != 0):
            raise ValueError("displacement_loss_weight / corr_normal_loss_weight != 0 cannot be combined with the dense "
                             "sub-sample path (is_subsample_opt with n > npoint): point i of the sample is not point i of "
                             "the clean cloud")
        # The neighbour tables (knn_table_plan): the curvature term's table of this iteration holds the nearest of any
        # narrower term in its first columns; a term it does not serve searches for itself, repulsion and normal with ONE
        # search for both.  The displacement term reads the clean cloud's table, built once per batch (setup()).
        plan, self.knn_searches_per_iteration = knn_table_plan(
            self.use_curv, self.k, self.w_disp, self.k_disp, self.w_rep, self.k_rep, self.w_cn, self.k_cn, self.w_knn,
            self.ks, bool(_cfg(cfg, "knn_smoothing_share_table", True)), bool(_cfg(cfg, "reg_share_table", True)))
        self.ks_table = self.reg_table = None
        self.curv_table = (_SelfKnnTable(t, "", b, ne, self.k + 1, device, int(_cfg(cfg, "knn_method", 0)))
                           if self.use_curv else None)
        if self.w_knn != 0:
            self.knn_share = plan["knn"][0] == "curv"
            t["ks_loss"], t["ks_grad"] = z(b), z(b, 3, ne)
            self.ks_ws = ops.reg_workspace(b, ne, self.ks, device)
            if not self.knn_share:
                self.ks_table = _SelfKnnTable(t, "ks_", b, ne, plan["knn"][1], device)
        # the per-point terms that are on, in their fold order
        self.point_terms = [(name, w, k) for name, w, k in (("disp", self.w_disp, self.k_disp), ("rep", self.w_rep, self.k_rep),
                                                            ("cn", self.w_cn, self.k_cn)) if w != 0]
        for name, _, _ in self.point_terms:
            t[name + "_out"], t[name + "_grad"], t[name + "_loss"] = z(b, ne), z(b, 3, ne), z(b)
        if self.point_terms:
            self.reg_ws = ops.reg_workspace(b, ne, max(k for _, _, k in self.point_terms), device)
        if self.w_disp != 0:
            self.disp_share = plan["disp"][0] == "curv"
            if not self.disp_share:
                t["disp_knn_d"], t["disp_knn"] = z(b, n, self.k_disp + 1), torch.zeros(b, n, self.k_disp + 1, **i32)
        if self.w_rep != 0 or self.w_cn != 0:
            table, self.reg_K = plan.get("rep") or plan["cn"]
            self.reg_share = table == "curv"
            if not self.reg_share:
                self.reg_table = _SelfKnnTable(t, "reg_", b, ne, self.reg_K, device)
        if self.w_cn != 0:
            # corresponding_normal_loss = geoa3_kappa with the point's own normal (a table of exactly k + 1 columns); its
            # gradient = geoa3_corr_normal_loss_grad, pair terms in double
            t["cn_knn"] = torch.zeros(b, ne, self.k_cn + 1, **i32)   # the table's first k + 1 columns, inside the cloud
        if self.native:
            bw = b * self.eval_num if self.sub else b
            nbytes = (self.lib.geoa3_pn2ssg_workspace_bytes(bw, ne) if self.ssg
                      else self.lib.geoa3_pointnet_workspace_bytes(bw, ne, self.classes))
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.state: Optional[AttackState] = None
        self._ws_fwd_shape = None       # (B, N) of the last victim forward that used self.ws

    # ------------------------------------------------------------------------------------
    def _p(self, x: Optional[Tensor]):
        return None if x is None else x.data_ptr()

    def _freeze(self):
        if not self.native and self._grad_flags is None:
            self._grad_flags = [(prm, prm.requires_grad) for prm in self.net.parameters()]
            for prm, _ in self._grad_flags:
                prm.requires_grad_(False)

    def _unfreeze(self):
        if not self.native and self._grad_flags is not None:
            for prm, flag in self._grad_flags:
                prm.requires_grad_(flag)
            self._grad_flags = None

    def setup(self, pc_ori: Tensor, normal_ori: Tensor, gt: Tensor, target: Tensor):
        cfg, t = self.cfg, self.t
        if self.native:   # re-read the folded weights: a cached runner must see a victim whose weights were reloaded
            self.packed = self.net.packed(self.dev)
            if isinstance(self.net, PointNet):
                from .pointnet import ab_flags
                self.packed.struct.flags = ab_flags()
        self.ori = pc_ori.to(self.dev, torch.float32).contiguous()
        self.nrm = normal_ori.to(self.dev, torch.float32).contiguous()
        # the clean cloud of the geometry stages and its normals: the clean variable itself, unless a subclass says otherwise
        self.geo_ori, self.geo_nrm = self._clean_geometry()
        self.gt = gt.to(self.dev, torch.int32).contiguous()
        self.target = target.to(self.dev, torch.int32).contiguous()
        t["scale_const"].fill_(float(cfg.initial_const))
        t["lower"].zero_()
        t["upper"].fill_(1e10)
        t["best_loss"].fill_(1e10)
        t["best_attack"].fill_(1.0)
        t["best_step"].fill_(-1)
        t["best_bs"].fill_(-1)
        self.kappa_ori = None
        self.nn1_seeded = False
        knn_ori_d = knn_ori = None
        if self.use_curv:  # _get_kappa_ori once per batch (geoA3_attack.py:216-217)
            knn_ori_d, knn_ori = ops.knn_planar(self.geo_ori, self.geo_ori, self.k + 1)
            self.kappa_ori = ops.kappa(self.geo_ori, self.geo_nrm, knn_ori)
            self.curv_table.reset(None if self.sub else knn_ori)
        # the first prior of a term's own search: the clean cloud's neighbours (none for a sample: other points)
        own_prior = lambda tb: None if self.sub else ops.knn_planar(self.geo_ori, self.geo_ori, tb.cols)[1]
        if self.ks_table is not None:
            self.ks_table.reset(own_prior(self.ks_table))
        if self.w_disp != 0:   # displacement_loss reads the CLEAN cloud's neighbours (Lib/loss_utils.py:101): once per batch
            if self.disp_share:
                self.disp_table = (knn_ori_d, knn_ori, self.k + 1)
            else:
                ops.knn_planar(self.geo_ori, self.geo_ori, self.k_disp + 1, out=(t["disp_knn_d"], t["disp_knn"]))
                self.disp_table = (t["disp_knn_d"], t["disp_knn"], self.k_disp + 1)
        if self.reg_table is not None:
            self.reg_table.reset(own_prior(self.reg_table))
        cls_type = {"None": 0, "CE": 1, "Margin": 2}[cfg.cls_loss_type]
        self.state = AttackState(
            B=self.b, N=self.n, classes=self.classes, targeted=int(self.targeted), cls_loss_type=cls_type,
            confidence=float(_cfg(cfg, "confidence", 0.0)), inv_global_batch=1.0 / float(self.global_batch),
            gt=self._p(self.gt), target=self._p(self.target), scale_const=self._p(t["scale_const"]),
            lower_bound=self._p(t["lower"]), upper_bound=self._p(t["upper"]), best_loss=self._p(t["best_loss"]),
            best_attack=self._p(t["best_attack"]), best_step=self._p(t["best_step"]), best_bs=self._p(t["best_bs"]),
            iter_best_loss=self._p(t["iter_best_loss"]), iter_best_score=self._p(t["iter_best_score"]),
            prev_constrain=self._p(t["prev_constrain"]), label=self._p(t["label"]), cls_loss=self._p(t["cls_loss"]),
            loss_n=self._p(t["loss_n"]), loss_hist=self._p(t["loss_hist"]), last_label=self._p(t["last_label"]))

    def _clean_geometry(self):
        """-> (clean cloud [b,3,geo_n], its normals) of the geometry stages, called by setup() once self.ori / self.nrm stand"""
        return self.ori, self.nrm

    def _variable_terms(self, sg: int):
        """Constraint terms on the optimised variable itself rather than on xe, folded last (a subclass; none here)"""

    # ------------------------------------------------------------------------------------
    def begin_search_step(self, init_offset: Optional[Tensor]):
        t = self.t
        if self.partial:   # the offset is drawn inside the loop (every 50 steps): start from the clean cloud
            init_offset = torch.zeros(self.b, 3, self.n, device=self.dev)
        init = init_offset.to(self.dev, torch.float32).contiguous()
        self._freeze()   # callers that drive step() themselves (bench.py, tests): undone by end_search_step()
        s = torch.cuda.current_stream().cuda_stream
        check(self.lib.geoa3_attack_begin_search_step(C.byref(self.state), self._p(self.ori), self._p(init),
                                                      self._p(t["offset"]), self._p(t["m"]), self._p(t["v"]),
                                                      self._p(t["x"]), s), "begin_search_step")

    def _native_forward(self, pts: Tensor, out: Tensor, s: int):
        fn = self.lib.geoa3_pn2ssg_forward if self.ssg else self.lib.geoa3_pointnet_forward
        st = self.packed.struct
        shape = (int(pts.shape[0]), int(pts.shape[2]))
        # PointNet: a forward of the same shape as the last one on this workspace finds its arg-max keys zero already
        # (GEOA3_PN_KEYS_CLEAN: no clearing launch); the weight table is shared with the module, so the bit is set for
        # this call only
        clean = not self.ssg and self._ws_fwd_shape == shape
        self._ws_fwd_shape = None
        if clean:
            st.flags |= 4
        try:
            check(fn(C.byref(st), pts.data_ptr(), pts.shape[0], pts.shape[2], out.data_ptr(), self.ws.data_ptr(), s),
                  "victim forward")
        finally:
            if clean:
                st.flags &= ~4
        self._ws_fwd_shape = shape

    def _victim_labels_logits(self, pts: Tensor, out: Tensor):
        """logits of the victim on pts [B',3,m] (no gradient kept) -> out [B',classes]."""
        if self.native:
            self._native_forward(pts, out, torch.cuda.current_stream().cuda_stream)
        else:
            with torch.no_grad():
                out.copy_(self.net(pts))

    def step(self, step: int, search_step: int):
        """One inner iteration (geoA3_attack.py:238-352) for all b instances; only enqueues."""
        g = self.objective(step, search_step)
        if g is not None:
            self.optimiser_step(step, g[0], g[1])

    def objective(self, step: int, search_step: int):
        """Success check + `_forward_step` + backward of one iteration (geoA3_attack.py:238-326) on the current
        iterate t["x"]: fills logits / cls_loss / loss_n / the distance losses and returns the two gradient parts
        (g_cls [b,3,n] already scaled by 1/b, g_geo [b,3,n] = d constrain / dx un-scaled; either may be None), or None
        when the step is complete (--is_partial_var keeps its own optimiser)."""
        main = torch.cuda.current_stream()
        s = main.cuda_stream
        if self.partial and step % 50 == 0:
            self._partial_redraw(step, search_step, s)
        xe, vote_logits = self.t["x"], None     # what the objective is evaluated on [b,3,ne]; what the success check sees
        if self.sub:
            xe, vote_logits = self._sample_and_votes(step, search_step, s)
        if self.jitter:
            xe, vote_logits = self._jitter(step, search_step, xe, vote_logits)
        late = self.late_join and self.geo_stream is not None
        sg = self._fork_geometry(main, s)
        autograd = self._victim_forward(xe, s)
        constrain, geo_on = self._geometry(xe, sg, main, late)
        self._head(late, vote_logits, constrain, step, search_step, s)
        g_cls = self._victim_backward(xe, autograd, s) if self.cfg.cls_loss_type != "None" else None
        if late:
            self._head_finish(main, constrain, step, search_step, s)
        if self.w_uni != 0:
            g_cls = self._uniform_grad(g_cls, s)
        g_geo = self.t["g_geo"] if geo_on else None
        if self.sub:
            g_cls, g_geo = self._scatter_to_full_cloud(g_cls, g_geo, s)
        if self.partial:
            return self._partial_update(step, g_cls, g_geo, s)
        return g_cls, g_geo

    # ---- the stages of objective(), in its order
    def _partial_redraw(self, step: int, search_step: int, s: int):
        """--is_partial_var, every 50 steps (geoA3_attack.py:240-262): new neighbourhood, new offset, fresh optimiser."""
        t, x = self.t, self.t["x"]
        hook = self.hooks.get("partial_points")
        p0 = int(hook(search_step, step)) if hook else int(np.random.randint(self.n))
        _, nbr = ops.knn_planar(self.ori[:, :, p0:p0 + 1].contiguous(), self.ori, self.kr + 1)
        t["pidx"].copy_(nbr[:, 0, 1:])
        hook = self.hooks.get("partial_inits")
        t["part"].copy_(hook(search_step, step) if hook else torch.randn(self.b, 3, self.kr, device=self.dev) * 1e-3)
        t["pm"].zero_()
        t["pv"].zero_()
        t["periodical"].copy_(x)    # the iterate of the last forward (its optimiser step is dropped, as :259-262)
        check(self.lib.geoa3_attack_partial_step(C.byref(self.state), None, None, t["pidx"].data_ptr(), self.kr,
                                                 t["periodical"].data_ptr(), t["part"].data_ptr(), None, None,
                                                 x.data_ptr(), -1, 0.0, 1.0, 0.0, 0, s), "attack_partial_step")
        self.part_t = 0

    def _sample_and_votes(self, step: int, search_step: int, s: int):
        """geoA3_attack.py:283-284: the objective's sample; :289-295: eval_num resamplings per instance for the
        success vote.  The reference draws the start indices with torch.randint on its device.  -> (xe, vote logits)"""
        t, lib, x, ne, E = self.t, self.lib, self.t["x"], self.ne, self.eval_num
        hook = self.hooks.get("sub_starts")
        start = hook(search_step, step) if hook else torch.randint(self.n, (self.b,), device=self.dev)
        start = start.to(self.dev, torch.int32).contiguous()
        check(lib.geoa3_fps_sample(x.data_ptr(), self.b, self.n, ne, start.data_ptr(), t["sub_idx"].data_ptr(),
                                   t["x_cur"].data_ptr(), s), "fps_sample")
        hook = self.hooks.get("vote_starts")
        vstart = hook(search_step, step) if hook else torch.randint(self.n, (self.b, E), device=self.dev)
        vstart = vstart.to(self.dev, torch.int32).reshape(-1).contiguous()
        xrep = x if E == 1 else x.unsqueeze(1).expand(self.b, E, 3, self.n).reshape(self.b * E, 3, self.n)
        check(lib.geoa3_fps_sample(xrep.data_ptr(), self.b * E, self.n, ne, vstart.data_ptr(),
                                   t["vote_idx"].data_ptr(), t["vote_pts"].data_ptr(), s), "fps_sample")
        self._victim_labels_logits(t["vote_pts"], t["vote_logits"])
        return t["x_cur"], t["vote_logits"]

    def _jitter(self, step: int, search_step: int, xe: Tensor, vote_logits: Optional[Tensor]):
        """--is_pre_jitter_input (geoA3_attack.py:312-317) -> (xe + tangent-plane noise, vote logits)"""
        from . import utility as U
        cfg, t = self.cfg, self.t
        if not self.sub:   # the success check sees the iterate WITHOUT the jitter (geoA3_attack.py:297 vs :317)
            self._victim_labels_logits(xe, t["check_logits"])
            vote_logits = t["check_logits"]
        if step % int(cfg.calculate_project_jitter_noise_iter) == 0:
            hook = self.hooks.get("jitter_noise")
            if hook:
                t["noise"].copy_(hook(search_step, step, xe))
            else:
                aux = self.hooks["jitter_aux"](search_step, step) if "jitter_aux" in self.hooks else None
                t["noise"].copy_(U.estimate_perpendicular(xe, int(cfg.jitter_k), float(cfg.jitter_sigma),
                                                          float(cfg.jitter_clip), aux=aux))
        torch.add(xe, t["noise"], out=t["x_eval"])
        return t["x_eval"], vote_logits

    def _fork_geometry(self, main, s: int) -> int:
        """xe is final on the main stream: the geometry may start beside the victim's forward.  -> its stream"""
        if self.geo_stream is None:
            return s
        self.ev_x.record(main)
        self.geo_stream.wait_event(self.ev_x)
        return self.geo_stream.cuda_stream

    def _victim_forward(self, xe: Tensor, s: int):
        """logits of xe -> t["logits"]; -> (logits, leaf) of the autograd graph of a victim that is not native"""
        t = self.t
        if self.native:
            self._native_forward(xe, t["logits"], s)
            return None
        x_leaf = xe.detach().clone().requires_grad_()
        with torch.enable_grad():
            logits_ag = self.net(x_leaf)
        if logits_ag.shape != t["logits"].shape:
            raise _lib.Geoa3Error("the victim returned logits of shape %s, expected %s (set cfg.classes)"
                                  % (tuple(logits_ag.shape), tuple(t["logits"].shape)))
        t["logits"].copy_(logits_ag.detach())
        return logits_ag, x_leaf

    def _geometry(self, xe: Tensor, sg: int, main, late: bool):
        """The constraint terms on the geometry stream, each folded into constrain / g_geo (_fold), in a FIXED order:
        objective, kNN smoothing, displacement, repulsion, normal, uniform.  -> (constrain or None, g_geo was written)"""
        with (torch.cuda.stream(self.geo_stream) if self.geo_stream is not None else contextlib.nullcontext()):
            self._constrain, self._geo_on = None, False
            curv = self._distance_curvature(xe, sg) if self.geo_runs else None    # the curvature term's table, if any
            if self.w_knn != 0:
                self._knn_smoothing(xe, sg, curv if self.knn_share else self.ks_table.search(xe, sg))
            if self.point_terms:
                self._point_regularisers(xe, sg, curv)
            if self.w_uni != 0:
                self._uniform(xe, sg)
            self._variable_terms(sg)
        if self.geo_stream is not None:     # join: the bookkeeping needs the constrain loss, the update the gradient
            self.ev_geo.record(self.geo_stream)
            if not late:
                main.wait_event(self.ev_geo)
        return self._constrain, self._geo_on

    def _fold(self, sg: int, fold, *args, g: bool = True, **kw):
        """The one fold step: constrain_b (+)= w term_b (before the head reads it) and, with g, g_geo (+)= w d term_b / dx,
        through fold(*args, b, ne, ...) on the geometry stream; fold None: the objective, first in the order, has written
        both itself.  The only place that knows whether either has been written yet.  g_geo stays UN-scaled:
        attack_update_kernel multiplies all of it by scale_const[b] * inv_global_batch (= c_b / b, the gradient of
        mean_b(c_b constrain_b)) when it forms g = g_cls + (c_b / b) g_geo, so every term gets that factor there, once."""
        on = self._geo_on
        if fold is not None:
            if g:
                kw.update(g=self.t["g_geo"], g_add=on)
            fold(*args, self.b, self.ne, constrain=self.geo_out["constrain"], constrain_add=on, stream=sg, **kw)
        self._constrain, self._geo_on = self.geo_out["constrain"], on or g

    def _distance_curvature(self, xe: Tensor, sg: int):
        """The 1-NN tables, the curvature term's K-NN table and the fused distance / Hausdorff / curvature objective
        (geoA3_attack.py:131-166), which writes constrain and g_geo.  -> the curvature term's table or None"""
        cfg, t, lib = self.cfg, self.t, self.lib
        ao = (t["d_ao"], t["i_ao"]) if self.need_nn else (None, None)
        oa = (t["d_oa"], t["i_oa"]) if self.both else (None, None)
        if self.need_nn:
            head = (xe.data_ptr(), self.geo_ori.data_ptr(), self.b, self.ne, self.geo_n)
            out = [self._p(x) for x in ao + oa]
            if self.grid_nn1:   # seeded with the tables of the previous iteration (in place)
                pa, pr = (out[1], out[3]) if self.nn1_seeded else (None, None)
                fn, policy = ((lib.geoa3_grid_nn1_pair, ()) if self.nn1_policy is None
                              else (lib.geoa3_debug_grid_nn1_pair, self.nn1_policy))
                check(fn(*head, pa, pr, *out, *policy, sg), "grid_nn1_pair")
                self.nn1_seeded = not self.sub
            else:
                check(lib.geoa3_nn1_pair(*head, *out, sg), "nn1_pair")
        curv = self.curv_table.search(xe, sg) if self.use_curv else None
        ops.geo_loss_grad(xe, self.geo_ori, normal_ori=self.geo_nrm if self.use_curv else None, kappa_ori=self.kappa_ori,
                          d_ao=ao[0], i_ao=ao[1], d_oa=oa[0], i_oa=oa[1], knn_adv=curv[1] if curv else None,
                          k=self.k if self.use_curv else 0, dis_type=self.dis_type,
                          single_side=bool(cfg.is_cd_single_side), w_dis=float(cfg.dis_loss_weight),
                          w_hd=float(cfg.hd_loss_weight), w_curv=float(cfg.curv_loss_weight), out=self.geo_out,
                          deterministic=self.deterministic, scratch=self.geo_scratch)
        self._fold(sg, None)
        return curv

    def _knn_smoothing(self, xe: Tensor, sg: int, table):
        """S_b = kNN_smoothing_loss(xe)[b] and dS_b/dx (Lib/loss_utils.py:135-149), folded as they are"""
        t, lib, ws = self.t, self.lib, self.ks_ws.data_ptr()
        head = (xe.data_ptr(), self.b, self.ne, self.ks, self.knn_coef, table[0].data_ptr(), table[1].data_ptr(), table[2])
        check(lib.geoa3_knn_smoothing_loss(*head, t["ks_loss"].data_ptr(), None, ws, sg), "knn_smoothing_loss")
        check(lib.geoa3_knn_smoothing_loss_grad(*head, None, t["ks_grad"].data_ptr(), ws, sg), "knn_smoothing_loss_grad")
        self._fold(sg, ops.reg_fold, t["ks_loss"], t["ks_grad"], self.w_knn)

    def _point_regularisers(self, xe: Tensor, sg: int, curv):
        """displacement, repulsion and normal, those that are on: out[b,i] and d(sum_i out[b,i])/dx of each, then folded
        through their row means: constrain_b (+)= w mean_i out[b,i], g_geo (+)= (w / ne) d(sum_i out[b,i])/dx"""
        t, lib, b, ne, ws = self.t, self.lib, self.b, self.ne, self.reg_ws.data_ptr()
        if self.w_disp != 0:   # on the CLEAN cloud's table (setup())
            clean = self.disp_table
            head = (xe.data_ptr(), self.geo_ori.data_ptr(), b, ne, self.k_disp, clean[0].data_ptr(), clean[1].data_ptr(), clean[2])
            check(lib.geoa3_displacement_loss(*head, t["disp_out"].data_ptr(), ws, sg), "displacement_loss")
            check(lib.geoa3_displacement_loss_grad(*head, None, t["disp_grad"].data_ptr(), ws, sg), "displacement_loss_grad")
        if self.w_rep != 0 or self.w_cn != 0:
            reg = curv if self.reg_share else self.reg_table.search(xe, sg)
            reg_ptrs = (reg[0].data_ptr(), reg[1].data_ptr(), reg[2])
        if self.w_rep != 0:
            head = (xe.data_ptr(), b, ne, self.k_rep, self.h_rep, *reg_ptrs)
            check(lib.geoa3_repulsion_loss(*head, t["rep_out"].data_ptr(), ws, sg), "repulsion_loss")
            check(lib.geoa3_repulsion_loss_grad(*head, None, t["rep_grad"].data_ptr(), ws, sg), "repulsion_loss_grad")
        if self.w_cn != 0:
            # geoa3_kappa takes a table of exactly k + 1 columns: the columns are copied as they are.  A point with a
            # non-finite coordinate has no neighbours (index -1, which geoa3_kappa does not follow: its term is NaN, and
            # so is the row's mean).  The gradient kernel reads the table itself and refuses such a row whole.
            t["cn_knn"].copy_(reg[1][:, :, :self.k_cn + 1])
            check(lib.geoa3_kappa(xe.data_ptr(), self.geo_nrm.data_ptr(), t["cn_knn"].data_ptr(), None, b, ne, ne, self.k_cn,
                                  t["cn_out"].data_ptr(), sg), "kappa")
            check(lib.geoa3_corr_normal_loss_grad(xe.data_ptr(), self.geo_nrm.data_ptr(), b, ne, self.k_cn, *reg_ptrs, None,
                                                  t["cn_grad"].data_ptr(), ws, sg), "corr_normal_loss_grad")
        for name, w, _ in self.point_terms:
            self._fold(sg, ops.reg_fold_points, t[name + "_out"], t[name + "_grad"], w, term=t[name + "_loss"])

    def _uniform(self, xe: Tensor, sg: int):
        """constrain (+)= w U before the head reads it (no other term on: constrain = w U); dU/dx joins g_cls after the
        join (_uniform_grad), g_geo is not written"""
        t = self.t
        ops.uniform_loss(xe, contract=self.uni_contract, workspace=self.uni_ws, out=(t["uni_loss"], t["uni_grad"]))
        self._fold(sg, ops.uniform_fold, t["uni_loss"], None, None, self.w_uni, g=False)

    def _head(self, late: bool, vote_logits, constrain, step: int, search_step: int, s: int):
        t, lib, st, votes = self.t, self.lib, C.byref(self.state), self.eval_num if self.sub else 1
        if late:   # the classification half of the head now, the victim's backward beside the geometry kernels
            check(lib.geoa3_attack_head_classify(st, t["logits"].data_ptr(), self._p(vote_logits), votes,
                                                 t["dlogits"].data_ptr(), t["ok"].data_ptr(), s), "attack_head_classify")
        else:
            check(lib.geoa3_attack_head_vote(st, t["logits"].data_ptr(), self._p(vote_logits), votes, self._p(constrain),
                                             t["x"].data_ptr(), step, search_step, t["dlogits"].data_ptr(), s),
                  "attack_head_vote")

    def _victim_backward(self, xe: Tensor, autograd, s: int) -> Tensor:
        t = self.t
        if self.native:
            fn = self.lib.geoa3_pn2ssg_backward if self.ssg else self.lib.geoa3_pointnet_backward
            check(fn(C.byref(self.packed.struct), xe.data_ptr(), t["dlogits"].data_ptr(), xe.shape[0], xe.shape[2],
                     t["g_cls"].data_ptr(), self.ws.data_ptr(), s), "victim backward")
        else:
            logits_ag, x_leaf = autograd
            logits_ag.backward(t["dlogits"])
            t["g_cls"].copy_(x_leaf.grad)
        return t["g_cls"]

    def _head_finish(self, main, constrain, step: int, search_step: int, s: int):
        """The late join: the rest of the head, once the geometry stream has delivered the constrain loss"""
        main.wait_event(self.ev_geo)
        check(self.lib.geoa3_attack_head_finish(C.byref(self.state), self.t["ok"].data_ptr(), self._p(constrain),
                                                self.t["x"].data_ptr(), step, search_step, s), "attack_head_finish")

    def _uniform_grad(self, g_cls: Optional[Tensor], s: int) -> Tensor:
        """d mean_b(c_b w U) / dx = w (sum_b c_b) / b dU/dx, unscaled like g_cls (geo stream joined)"""
        t = self.t
        ops.uniform_fold(t["uni_loss"], t["uni_grad"], t["scale_const"], self.w_uni, self.b, self.ne, g=t["g_cls"],
                         g_add=g_cls is not None, stream=s)
        return t["g_cls"]

    def _scatter_to_full_cloud(self, g_cls: Optional[Tensor], g_geo: Optional[Tensor], s: int):
        """torch.gather's backward (Lib/utility.py:185): scatter the sample's gradient to the full cloud"""
        t = self.t
        for src, dst in ((g_cls, "g_cls_full"), (g_geo, "g_geo_full")):
            if src is not None:
                check(self.lib.geoa3_pn2_gather_points_grad(src.data_ptr(), t["sub_idx"].data_ptr(), self.b, 3, self.n,
                                                            self.ne, t[dst].data_ptr(), s), "gather_points_grad")
        return (t["g_cls_full"] if g_cls is not None else None), (t["g_geo_full"] if g_geo is not None else None)

    def _partial_update(self, step: int, g_cls: Optional[Tensor], g_geo: Optional[Tensor], s: int) -> None:
        """--is_partial_var: its own optimiser on the [b,3,knn_range] offset; the step is complete"""
        t = self.t
        self.part_t += 1
        if (step + 1) % 50 != 0:    # the step before a re-draw is never used (periodical_pc = input_all, :260)
            check(self.lib.geoa3_attack_partial_step(C.byref(self.state), self._p(g_cls), self._p(g_geo),
                                                     t["pidx"].data_ptr(), self.kr, t["periodical"].data_ptr(),
                                                     t["part"].data_ptr(), t["pm"].data_ptr(), t["pv"].data_ptr(),
                                                     t["x"].data_ptr(), *self._optim_scalars(self.part_t - 1), s),
                  "attack_partial_step")
        return None  # the projections / lp_clip act on a padded copy in the reference: no effect (:341-352)

    def _optim_scalars(self, done: int):
        """(optim, step_size, sqrt_bc2, momentum, first) of the step after `done` steps of this optimiser, in double as
        torch.optim forms them"""
        cfg = self.cfg
        lr = cfg.lr * (0.9990 ** done if _cfg(cfg, "is_use_lr_scheduler", False) else 1.0)
        if cfg.optim == "adam":
            return 0, lr / (1.0 - 0.9 ** (done + 1)), math.sqrt(1.0 - 0.999 ** (done + 1)), 0.0, 0
        return 1, lr, 1.0, 0.9, int(done == 0)

    def optimiser_step(self, step: int, g_cls: Optional[Tensor], g_geo: Optional[Tensor]):
        """Adam / SGD on the offset with g = g_cls + (scale_const / b) g_geo, then the flag-gated projections
        (geoA3_attack.py:326-352)."""
        cfg, t, lib = self.cfg, self.t, self.lib
        s = torch.cuda.current_stream().cuda_stream
        st = C.byref(self.state)
        x = t["x"]
        pro_grad = bool(_cfg(cfg, "is_pro_grad", False))
        optim, step_size, sqrt_bc2, _, _ = self._optim_scalars(step)
        check(lib.geoa3_attack_update(st, self._p(g_cls), self._p(g_geo),
                                      self.ori.data_ptr(), t["offset"].data_ptr(), t["m"].data_ptr(),
                                      t["v"].data_ptr(), x.data_ptr(), optim, step_size, sqrt_bc2,
                                      0.0 if pro_grad else float(_cfg(cfg, "cc_linf", 0.0)), s), "attack_update")
        if pro_grad:   # geoA3_attack.py:341-352: (real offset,) projection onto the normal, then lp_clip
            pd, pi = t["proj_d"], t["proj_i"]
            if _cfg(cfg, "is_real_offset", False):
                check(lib.geoa3_nn1_pair(x.data_ptr(), self.ori.data_ptr(), self.b, self.n, self.n,
                                         pd.data_ptr(), pi.data_ptr(), None, None, s), "nn1_pair")
                check(lib.geoa3_attack_project(0, self.ori.data_ptr(), None, pi.data_ptr(),
                                               t["offset"].data_ptr(), x.data_ptr(), self.b, self.n, 0.0, s),
                      "attack_project")
            check(lib.geoa3_nn1_pair(t["offset"].data_ptr(), self.ori.data_ptr(), self.b, self.n, self.n,
                                     pd.data_ptr(), pi.data_ptr(), None, None, s), "nn1_pair")
            check(lib.geoa3_attack_project(1, self.ori.data_ptr(), self.nrm.data_ptr(), pi.data_ptr(),
                                           t["offset"].data_ptr(), x.data_ptr(), self.b, self.n,
                                           float(_cfg(cfg, "cc_linf", 0.0)), s), "attack_project")

    def end_search_step(self, sync_last_label: Optional[Callable[[Tensor], None]] = None):
        if sync_last_label is not None:
            sync_last_label(self.t["last_label"])
        s = torch.cuda.current_stream().cuda_stream
        check(self.lib.geoa3_attack_binary_update(C.byref(self.state), s), "binary_update")
        self._unfreeze()

    def info_line(self, search_step, step, i, loader_len) -> str:
        """The reference's progress line (geoA3_attack.py:129,138,154,163,365); the ONLY host sync in the loop."""
        cfg, t, go = self.cfg, self.t, self.geo_out
        tight, spaced = "{0}: {1:6.4f}\t", "{0} : {1:6.4f}\t"
        # (active, label, format, per-instance values or a scalar), in the order of the line
        rows = ((True, "loss", tight, t["loss_n"].mean() * (self.b / float(self.global_batch))),
                (True, "cls_loss", tight, t["cls_loss"]),
                (cfg.dis_loss_type in ("CD", "L2"), cfg.dis_loss_type.lower() + "_loss", tight, go["dis_loss"]),
                (cfg.hd_loss_weight != 0, "hd_loss", spaced, go["hd_loss"]),
                (cfg.curv_loss_weight != 0, "curv_loss", spaced, go["curv_loss"]),
                (self.w_uni != 0, "uniform", spaced, t.get("uni_loss")),
                (self.w_knn != 0, "knn_smooth", spaced, t.get("ks_loss")),
                (self.w_disp != 0, "disp_loss", spaced, t.get("disp_loss")),
                (self.w_rep != 0, "rep_loss", spaced, t.get("rep_loss")),
                (self.w_cn != 0, "cnor_loss", spaced, t.get("cn_loss")))
        rows = [row for row in rows if row[0]]
        vals = torch.stack([value.mean() for _, _, _, value in rows]).tolist()
        return "[{4}/{5}][{0}/{1}][{2}/{3}] \t ".format(search_step + 1, cfg.binary_max_steps, step + 1,
                                                         cfg.iter_max_steps, i, loader_len) + "".join(
            fmt.format(label, v) for (_, label, fmt, _), v in zip(rows, vals))

    def run(self, init_offsets: Optional[Sequence[Tensor]] = None, i: int = 0, loader_len: int = 1,
            verbose: bool = False, sync_last_label: Optional[Callable[[Tensor], None]] = None,
            on_step: Optional[Callable[[int, int], None]] = None, hooks: Optional[dict] = None):
        """hooks (parity runs): the reference's random draws as inputs -- sub_starts(search_step, step) -> [b],
        vote_starts(search_step, step) -> [b, eval_num] (torch.randint of farthest_points_sample),
        jitter_aux(search_step, step) -> (aux1, aux2) [b,ne] or jitter_noise(search_step, step, x) -> [b,3,ne];
        partial_points(search_step, step) -> int (np.random.randint) and partial_inits(search_step, step) ->
        [b,3,knn_range] (nn.init.normal_) for --is_partial_var."""
        self.hooks = dict(hooks or {})
        self._freeze()
        try:
            self._run(init_offsets, i, loader_len, verbose, sync_last_label, on_step)
        finally:
            self._unfreeze()

    def _run(self, init_offsets, i, loader_len, verbose, sync_last_label, on_step):
        cfg = self.cfg
        for search_step in range(int(cfg.binary_max_steps)):
            if self.partial:
                init = None
            elif init_offsets is not None:
                init = init_offsets[search_step]
            else:  # nn.init.normal_(offset, mean=0, std=1e-3), geoA3_attack.py:264-266
                init = torch.randn(self.b, 3, self.n, device=self.dev) * 1e-3
            self.begin_search_step(init)
            for step in range(self.iters):
                self.step(step, search_step)
                if on_step is not None:
                    on_step(search_step, step)
                if verbose and (step % 50 == 0 or step == self.iters - 1):
                    print(self.info_line(search_step, step, i, loader_len))
            self.end_search_step(sync_last_label)

    def results(self):
        """-> the reference 5-tuple (geoA3_attack.py:386)."""
        t = self.t
        success = (t["best_loss"].cpu().numpy() < 1e10)
        best_step = t["best_step"].cpu().tolist()
        all_loss = t["loss_hist"].cpu().tolist()
        # a fresh tensor per call, as the reference allocates one (geoA3_attack.py:226): a cached runner refills its
        # own buffer at the next setup()
        return t["best_attack"].clone(), self.target.long(), success, best_step, all_loss


# cfg fields that shape an AttackRunner's buffers / kernel choices at construction
RUNNER_CFG_FIELDS = ("attack_label", "iter_max_steps", "curv_loss_knn", "curv_loss_weight", "dis_loss_type",
                     "hd_loss_weight", "cls_loss_type", "optim", "uniform_loss_weight", "npoint", "is_partial_var",
                     "knn_range", "is_subsample_opt", "eval_num", "is_pre_jitter_input", "is_pro_grad",
                     "brute_force_nn1", "classes", "deterministic", "late_join", "knn_method",
                     "is_use_knn_smoothing_loss", "knn_smoothing_loss_weight", "knn_smoothing_k", "knn_threshold_coef",
                     "knn_smoothing_share_table", "displacement_loss_weight", "displacement_loss_knn",
                     "repulsion_loss_weight", "repulsion_loss_knn", "repulsion_loss_h", "corr_normal_loss_weight",
                     "corr_normal_loss_knn", "reg_share_table", "is_cd_single_side")


def unpack_input(input_data, targeted: bool):
    """The DataLoader batch of main_attack.py -> ([b,3,n] pc, [b,3,n] normal, gt [b], target [b])
    (geoA3_attack.py:196-214)."""
    pc, normal, gt_labels = input_data[0], input_data[1], input_data[2]
    if pc.size(3) == 3:
        pc = pc.permute(0, 1, 3, 2)
    if normal.size(3) == 3:
        normal = normal.permute(0, 1, 3, 2)
    bs, l, _, n = pc.size()
    b = bs * l
    pc_ori = pc.reshape(b, 3, n)
    normal_ori = normal.reshape(b, 3, n)
    gt = gt_labels.reshape(-1)
    target = input_data[3].reshape(-1) if targeted else gt
    return pc_ori, normal_ori, gt, target


def attack(net, input_data, cfg, i, loader_len, saved_dir=None, *, init_offsets=None, verbose=True,
           global_batch=None, sync_last_label=None, runner_cache: Optional[dict] = None,
           hooks: Optional[dict] = None):
    """Drop-in for geoA3_attack.attack (same positional arguments, same 5-tuple).  Keyword-only extras:
    init_offsets (list of [b,3,n] step-0 offsets, one per binary step, for reproducible parity runs),
    global_batch / sync_last_label (set by geoa3_amd.distributed when the batch is sharded)."""
    targeted = cfg.attack_label != "Untarget"
    pc_ori, normal_ori, gt, target = unpack_input(input_data, targeted)
    b, _, n = pc_ori.shape
    device = next(net.parameters()).device
    if device.type != "cuda":
        raise _lib.Geoa3Error("attack() needs the victim network on the GPU")
    # everything AttackRunner.__init__ derives from cfg is part of the key: a changed flag builds a new runner
    key = (b, n, id(net), global_batch) + tuple(
        (name, repr(getattr(cfg, name, None))) for name in RUNNER_CFG_FIELDS)
    runner = runner_cache.get(key) if runner_cache is not None else None
    if runner is None:
        runner = AttackRunner(net, b, n, cfg, device, global_batch)
        if runner_cache is not None:
            runner_cache[key] = runner
    runner.cfg = cfg
    runner.setup(pc_ori, normal_ori, gt, target)
    runner.run(init_offsets, i, loader_len, verbose, sync_last_label, hooks=hooks)
    return runner.results()


def attack_sharded(net, input_data, cfg, i, loader_len, saved_dir=None, *, init_offsets=None, verbose=False,
                   group=None):
    """attack() with the batch sharded by instance over the ranks of an initialised process group (one process
    per GPU, RCCL).  Every rank passes the SAME full batch and receives the full 5-tuple; a rank computes only
    its own block of instances (geoa3_amd.distributed)."""
    import torch.distributed as dist
    from .distributed import sharded_attack
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return attack(net, input_data, cfg, i, loader_len, saved_dir, init_offsets=init_offsets, verbose=verbose)
    targeted = cfg.attack_label != "Untarget"
    pc_ori, normal_ori, gt, target = unpack_input(input_data, targeted)
    b, _, n = pc_ori.shape
    device = next(net.parameters()).device
    if init_offsets is None:   # one shared draw so every rank sees the same global initial offsets
        g = torch.Generator(device="cpu").manual_seed(int(getattr(cfg, "id", 0)) * 1000003 + int(i))
        init_offsets = [torch.randn(b, 3, n, generator=g) * 1e-3 for _ in range(int(cfg.binary_max_steps))]

    def run_shard(pc, normal, g_, t_, inits, global_batch, sync):
        bl = pc.shape[0]
        if bl == 0:   # more ranks than instances: still take part in the per-binary-step broadcasts
            dummy = torch.zeros(1, dtype=torch.int32, device=device)
            for _ in range(int(cfg.binary_max_steps)):
                sync(dummy)
            return (torch.zeros(0, 3, n, device=device), t_.to(device).long(), np.zeros(0, bool), [],
                    [[] for _ in range(int(cfg.iter_max_steps))])
        runner = AttackRunner(net, bl, n, cfg, device, global_batch)
        runner.setup(pc, normal, g_, t_)
        runner.run([o.to(device) for o in inits], i, loader_len, verbose and dist.get_rank(group) == 0, sync)
        return runner.results()

    return sharded_attack(run_shard, pc_ori, normal_ori, gt, target, init_offsets, group)
