"""The mesh attack (--attack GeoA3_mesh; the reference parses the flag and raises "Not uploaded yet.", main_attack.py:27-28,
and shows only what it would write: Mesh/<name>.obj and Mat/<name>.mat with `vert` / `faces`, main_attack.py:283-293).

The optimised variable is the VERTEX array of a batch of triangle meshes, planar and padded like every cloud of the loop
([b,3,Vp], nv [b]); the state kernels of attack_state.hip run on it as they are (x = ori + offset, Adam / SGD, cc_linf,
binary search, best_attack).  The objective is evaluated on xe = surface_points(x): S = cfg.npoint points of a draw
(face_idx, u) made ONCE per batch with sample_surface on the clean mesh and kept (hooks["mesh_u"]() -> u [b,S,3] supplies
it for parity runs).  The geometric objective's clean cloud is the clean mesh's sample with its face normals.  g_cls and
g_geo of the points are pulled back to the vertices separately (geoa3_mesh_points_grad, ordered: same bits every run); the
two mesh terms -- pytorch3d's mesh_laplacian_smoothing(method="uniform") and mesh_edge_loss with the clean mesh's own edge
lengths as target, so that both the term and its gradient are 0 at offset 0 -- are folded like every other constraint
term: constrain_b += w_lap Lap_b + w_edge Edge_b before the head reads it, their gradient into the vertex-level g_geo.
No host synchronisation in the loop; setup reads the batch on the host (the topology is built there, and a mesh without
area, or with bad faces, is refused by name).

    adv_verts, target, success, best_step, loss = attack_mesh(net, packed, labels, targets, cfg)

Not defined here, refused by name: --is_subsample_opt, --is_partial_var, --is_pre_jitter_input, --is_pro_grad,
--uniform_loss_weight, the kNN-smoothing / displacement / repulsion / normal extension weights, sharded runs.
Out of scope: re-drawing the samples during a run, non-triangle faces, multi-GPU, a CPU path."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib, mesh as M
from ._lib import check
from .attack import AttackRunner, _cfg

Tensor = torch.Tensor

# what this mode does not define: (cfg field, flag) refused when set / non-zero
REFUSED_FLAGS = (("is_subsample_opt", "--is_subsample_opt"), ("is_partial_var", "--is_partial_var"),
                 ("is_pre_jitter_input", "--is_pre_jitter_input"), ("is_pro_grad", "--is_pro_grad"),
                 ("is_use_knn_smoothing_loss", "--is_use_knn_smoothing_loss"))
REFUSED_WEIGHTS = (("uniform_loss_weight", "--uniform_loss_weight"), ("displacement_loss_weight", "--displacement_loss_weight"),
                   ("repulsion_loss_weight", "--repulsion_loss_weight"), ("corr_normal_loss_weight", "--corr_normal_loss_weight"))


def refuse_unsupported(cfg, world_size: int = 1) -> None:
    """Raise ValueError naming the first flag the mesh attack does not define."""
    for field, flag in REFUSED_FLAGS:
        if bool(_cfg(cfg, field, False)):
            raise ValueError("%s is not defined for --attack GeoA3_mesh (the variable is the vertex array, evaluated on a "
                             "fixed surface draw)" % flag)
    for field, flag in REFUSED_WEIGHTS:
        if float(_cfg(cfg, field, 0.0)) != 0:
            raise ValueError("%s != 0 is not defined for --attack GeoA3_mesh" % flag)
    if world_size > 1:
        raise ValueError("a sharded run (WORLD_SIZE > 1) is not defined for --attack GeoA3_mesh")


class MeshAttackRunner(AttackRunner):
    """AttackRunner whose variable is the vertex array [b,3,vp] and whose objective sees surface_points(x) [b,3,S]."""

    def __init__(self, net, b: int, vp: int, cfg, device, global_batch: Optional[int] = None):
        refuse_unsupported(cfg, 1 if global_batch in (None, b) else 2)
        s = int(cfg.npoint)
        super().__init__(net, b, vp, cfg, device, global_batch, ne=s, geo_n=s)
        self.w_lap = float(_cfg(cfg, "laplacian_loss_weight", 0.0))
        self.w_edge = float(_cfg(cfg, "edge_loss_weight", 0.0))
        z = lambda *shape: torch.zeros(*shape, device=device, dtype=torch.float32)
        t = self.t
        t["xe"] = z(b, 3, s)
        t["g_cls_full"], t["g_geo_full"] = z(b, 3, vp), z(b, 3, vp)
        t["mesh_unit"], t["lap_loss"], t["edge_loss"] = z(b, 4, vp), z(b), z(b)

    # ------------------------------------------------------------------------------------
    def setup_mesh(self, packed, gt: Tensor, target: Tensor, u: Optional[Tensor] = None):
        """A new batch: the draw, the clean cloud of the geometry stages, the topology and the pullback's lists (once)."""
        packed, b, _, tf, _ = M._unpack(packed)
        if b != self.b:
            raise ValueError("the runner was built for %d meshes, the batch holds %d" % (self.b, b))
        s = self.ne
        if u is None:
            u = torch.rand(b, s, 3, device=self.dev, dtype=torch.float32)
        u = u.to(self.dev, torch.float32).contiguous()
        verts, nv = M.to_planar(packed, self.n)
        pts, nrm, fidx, bad = M.sample_surface(packed, s, u=u)
        state = torch.stack([bad, (fidx < 0).sum(1).to(torch.int32)]).cpu().numpy()     # the one synchronisation
        for i in range(b):
            if state[0, i] != 0:
                raise ValueError("mesh %d of the batch has %d bad faces (an index outside its vertices, or a non-finite "
                                 "area): it cannot be attacked" % (i, state[0, i]))
            if state[1, i] != 0:
                raise ValueError("mesh %d of the batch has no surface area (or its draw holds a NaN): it cannot be attacked" % i)
        self.mesh, self.nv, self.total_faces = packed, nv, tf
        self.face_idx, self.u = fidx, u
        self.topo = M.MeshTopology.from_packed(packed, self.n)
        self.lists = M.mesh_point_lists(nv, packed.faces, packed.face_off, fidx, self.n)
        self.edge_target = self.topo.edge_lengths(verts)
        self._sample = (pts, nrm)
        super().setup(verts, torch.zeros_like(verts), gt, target)

    def _clean_geometry(self):
        return self._sample

    # ------------------------------------------------------------------------------------
    def _surface_points(self, x: Tensor, out: Tensor, s: int) -> Tensor:
        m = self.mesh
        check(self.lib.geoa3_mesh_points(x.data_ptr(), self.nv.data_ptr(), m.faces.data_ptr(), m.face_off.data_ptr(),
                                         self.face_idx.data_ptr(), self.u.data_ptr(), self.b, self.n, self.ne,
                                         self.total_faces, out.data_ptr(), s), "mesh_points")
        return out

    def objective(self, step: int, search_step: int):
        """AttackRunner.objective on xe = surface_points(x); the two gradient parts come back on the vertices."""
        main = torch.cuda.current_stream()
        s = main.cuda_stream
        xe = self._surface_points(self.t["x"], self.t["xe"], s)
        late = self.late_join and self.geo_stream is not None
        sg = self._fork_geometry(main, s)
        autograd = self._victim_forward(xe, s)
        constrain, geo_on = self._geometry(xe, sg, main, late)
        self._head(late, None, constrain, step, search_step, s)
        g_cls = self._victim_backward(xe, autograd, s) if self.cfg.cls_loss_type != "None" else None
        if late:
            self._head_finish(main, constrain, step, search_step, s)
        return self._pull_back(g_cls, self.t["g_geo"] if geo_on else None, s)

    def _mesh_fold(self, b: int, ne: int, constrain: Tensor, constrain_add: bool, stream: int):
        """constrain_b (+)= w_lap Lap_b + w_edge Edge_b of the current vertices; u_i stays in t["mesh_unit"] for the gradient"""
        t, tp = self.t, self.topo
        check(self.lib.geoa3_mesh_reg(t["x"].data_ptr(), self.nv.data_ptr(), tp.row_off.data_ptr(), M._ptr(tp.col),
                                      tp.ne.data_ptr(), M._ptr(self.edge_target), 0.0, b, self.n, tp.nnz, self.w_lap,
                                      self.w_edge, t["mesh_unit"].data_ptr(), t["lap_loss"].data_ptr(),
                                      t["edge_loss"].data_ptr(), constrain.data_ptr(), int(constrain_add), stream), "mesh_reg")

    def _variable_terms(self, sg: int):
        if self.w_lap != 0 or self.w_edge != 0:
            self._fold(sg, self._mesh_fold, g=False)    # (their gradient lives on the vertices: _pull_back)

    def _pull_back(self, g_cls: Optional[Tensor], g_geo: Optional[Tensor], s: int):
        """The points' two gradients to the vertices, each on its own; then the mesh terms' gradient onto g_geo"""
        t, tp, lib = self.t, self.topo, self.lib
        out = [None, None]
        for k, (src, dst) in enumerate(((g_cls, "g_cls_full"), (g_geo, "g_geo_full"))):
            if src is not None:
                check(lib.geoa3_mesh_points_grad(src.data_ptr(), self.u.data_ptr(), self.lists.data_ptr(), self.b, self.n,
                                                 self.ne, t[dst].data_ptr(), s), "mesh_points_grad")
                out[k] = t[dst]
        if self.w_lap != 0 or self.w_edge != 0:
            check(lib.geoa3_mesh_reg_grad(t["x"].data_ptr(), self.nv.data_ptr(), tp.row_off.data_ptr(), M._ptr(tp.col),
                                          tp.ne.data_ptr(), M._ptr(self.edge_target), 0.0, t["mesh_unit"].data_ptr(), None,
                                          None, self.w_lap, self.w_edge, self.b, self.n, tp.nnz, t["g_geo_full"].data_ptr(),
                                          int(out[1] is not None), s), "mesh_reg_grad")
            out[1] = t["g_geo_full"]
        return out[0], out[1]

    def info_line(self, search_step, step, i, loader_len) -> str:
        line, t = super().info_line(search_step, step, i, loader_len), self.t
        for on, label, value in ((self.w_lap != 0, "lap_loss", t["lap_loss"]), (self.w_edge != 0, "edge_loss", t["edge_loss"])):
            if on:
                line += "{0} : {1:6.4f}\t".format(label, value.mean().item())
        return line

    def results(self):
        """-> the reference 5-tuple (geoA3_attack.py:386) with the adversarial VERTICES: a list of [3,V_b] tensors."""
        best, target, success, best_step, all_loss = super().results()
        return [best[i, :, :n] for i, n in enumerate(self.nv.cpu().tolist())], target, success, best_step, all_loss


def attack_mesh(net, packed, labels, targets, cfg, i: int = 0, loader_len: int = 1, *,
                init_offsets: Optional[Sequence[Tensor]] = None, verbose: bool = False, hooks: Optional[dict] = None,
                runner: Optional[MeshAttackRunner] = None):
    """The mesh attack on one batch: packed (PackedMeshes on the GPU), labels / targets [b] (targets is read when
    cfg.attack_label != "Untarget", else the labels).  -> (list of adversarial vertices [3,V_b], target [b], success [b],
    best_step, loss history).  init_offsets: one [b,3,Vp] offset per binary step (Vp = the largest vertex count);
    hooks["mesh_u"]() -> the draw u [b,S,3]."""
    packed, b, _, _, _ = M._unpack(packed)
    device = packed.verts.device
    vp = max(1, int((packed.vert_off[1:] - packed.vert_off[:-1]).max().item()))
    if runner is None:
        runner = MeshAttackRunner(net, b, vp, cfg, device)
    runner.cfg = cfg
    hooks = dict(hooks or {})
    u = hooks["mesh_u"]() if "mesh_u" in hooks else None
    gt = torch.as_tensor(labels).reshape(-1)
    target = torch.as_tensor(targets).reshape(-1) if cfg.attack_label != "Untarget" else gt
    runner.setup_mesh(packed, gt, target, u=u)
    runner.run(init_offsets, i, loader_len, verbose, hooks=hooks)
    return runner.results()


# ------------------------------------------------------------------ inputs of the command line
def normalize_mesh(verts: np.ndarray) -> np.ndarray:
    """centred on the mean of the vertices and scaled to unit radius, float32"""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    v = v - v.mean(0)
    r = np.sqrt((v * v).sum(1).max())
    return (v / (r if r > 0 else 1.0)).astype(np.float32)


def icosphere(level: int = 2):
    """an icosahedron subdivided `level` times on the unit sphere: 10 4^level + 2 vertices, 20 4^level faces (level 2: 162, 320)"""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
         (-p, 0, -1), (-p, 0, 1)]
    v = [tuple(np.array(x) / np.linalg.norm(x)) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(level)):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                q = (np.array(v[a]) + np.array(v[b])) / 2
                mid[key] = len(v)
                v.append(tuple(q / np.linalg.norm(q)))
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = out
    return np.array(v, np.float32), np.array(f, np.int32)


def synthetic_meshes(count: int, seed: int = 0, level: int = 2):
    """count seeded meshes: the icosphere stretched along its axes by factors in [0.4, 1] drawn per instance, normalised"""
    rng = np.random.default_rng(seed)
    v, f = icosphere(level)
    return [(normalize_mesh(v.astype(np.float64) * rng.uniform(0.4, 1.0, 3)), f.copy()) for _ in range(int(count))]
