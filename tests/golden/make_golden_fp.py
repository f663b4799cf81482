#!/usr/bin/env python3
"""Generate tests/golden/geoa3_golden_fp.npz from the REFERENCE's own ThreeNN / ThreeInterpolate / PointnetFPModule
(build container only).

Run:  python tests/golden/make_golden_fp.py            (needs /root/reference; CPU only)

The reference's Python (pointnet2_utils.py:104-191, pointnet2_modules.py:149-209) runs unchanged on CPU; the three native
functions it calls are CUDA-only, so the registered `pointnet2_ops._ext` stand-in (make_golden.install_shims) gets its three
missing attributes at run time from the numpy restatement tests/_three_ref.py.  Stored: inputs, the seeded module weights
(arrays) and their state_dict key names, dist / idx / weight / interpolated features, the module's eval and train outputs
and its feature gradients.  Arrays and names only.
"""
from __future__ import annotations

import copy
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REPO, install_shims, t2n  # noqa: E402

# tag -> (B, n, m, C1 (unknown points' own channels, 0 = none), C2 (known channels), seed, mode)
FP_CASES = {
    "gauss": (2, 70, 20, 5, 6, 71, "gauss"),
    "nofeat": (1, 33, 9, 0, 4, 72, "gauss"),
    "lattice": (2, 40, 27, 3, 3, 73, "lattice"),     # known on a 3x3x3 lattice, some unknown points ON it: ties, distance 0
}
MLP_TAIL = [64, 32]


def clouds(B, n, m, seed, mode):
    g = torch.Generator().manual_seed(seed)
    if mode == "lattice":
        ax = torch.tensor([-0.5, 0.0, 0.5])
        known = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(1, 27, 3).repeat(B, 1, 1)[:, :m]
        unknown = torch.round(torch.randn(B, n, 3, generator=g) * 2) * 0.25
        unknown[:, :5] = known[:, :5]
    else:
        known = torch.randn(B, m, 3, generator=g)
        unknown = torch.randn(B, n, 3, generator=g)
    return unknown.contiguous(), known.contiguous()


def seed_module(mod, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in mod.state_dict().items():
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith("running_var"):
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            elif name.endswith("weight") and t.dim() == 1:
                t.copy_(torch.rand(t.shape, generator=g) + 0.5)
            elif t.dim() == 1:
                t.copy_(torch.randn(t.shape, generator=g) * 0.1)
            else:
                t.copy_(torch.randn(t.shape, generator=g) / float(t.shape[1]) ** 0.5)


def main():
    if not os.path.isdir(REF):
        sys.exit("needs /root/reference (build container only)")
    install_shims()
    sys.path.insert(0, REPO)
    from tests import _three_ref as R
    ext = sys.modules["pointnet2_ops._ext"]
    ext.three_nn, ext.three_interpolate, ext.three_interpolate_grad = R.three_nn_t, R.three_interpolate_t, R.three_interpolate_grad_t
    from pointnet2_ops import pointnet2_utils as PU      # the reference's own
    from pointnet2_ops.pointnet2_modules import PointnetFPModule

    out = {}
    for tag, (B, n, m, C1, C2, seed, mode) in FP_CASES.items():
        pre = "fp/%s/" % tag
        unknown, known = clouds(B, n, m, seed, mode)
        g = torch.Generator().manual_seed(seed + 100)
        known_feats = torch.randn(B, C2, m, generator=g)
        unknow_feats = torch.randn(B, C1, n, generator=g) if C1 else None
        cot_interp = torch.randn(B, C2, n, generator=g)
        cot_out = torch.randn(B, MLP_TAIL[-1], n, generator=g)

        # the operators on their own, composed as pointnet2_modules.py:186-193
        dist, idx = PU.three_nn(unknown, known)
        dist_recip = 1.0 / (dist + 1e-8)
        weight = (dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)).requires_grad_()
        kf = known_feats.clone().requires_grad_()
        interp = PU.three_interpolate(kf, idx, weight)
        g_kf, g_w = torch.autograd.grad(interp, (kf, weight), cot_interp)
        out[pre + "unknown"], out[pre + "known"], out[pre + "known_feats"] = t2n(unknown), t2n(known), t2n(known_feats)
        if C1:
            out[pre + "unknow_feats"] = t2n(unknow_feats)
        out[pre + "cot_interp"], out[pre + "cot_out"] = t2n(cot_interp), t2n(cot_out)
        out[pre + "dist"], out[pre + "idx"], out[pre + "weight"] = t2n(dist), t2n(idx).astype(np.int32), t2n(weight)
        out[pre + "interp"], out[pre + "interp_grad_feats"], out[pre + "interp_grad_weight"] = t2n(interp), t2n(g_kf), t2n(g_w)

        # the module
        mod = PointnetFPModule([C1 + C2] + MLP_TAIL)
        seed_module(mod, seed + 200)
        names = list(mod.state_dict().keys())
        out[pre + "sd_names"] = np.array(names)
        for k, v in mod.state_dict().items():
            out[pre + "sd/" + k] = t2n(v)
        mod.eval()
        kf = known_feats.clone().requires_grad_()
        uf = unknow_feats.clone().requires_grad_() if C1 else None
        y = mod(unknown, known, uf, kf)
        grads = torch.autograd.grad(y, (kf, uf) if C1 else (kf,), cot_out)
        out[pre + "out_eval"], out[pre + "grad_known_feats"] = t2n(y), t2n(grads[0])
        if C1:
            out[pre + "grad_unknow_feats"] = t2n(grads[1])
        tr = copy.deepcopy(mod).train()
        with torch.no_grad():
            out[pre + "out_train"] = t2n(tr(unknown, known, unknow_feats, known_feats))
    out["fp/cases"] = np.array(list(FP_CASES))

    path = os.path.join(HERE, "geoa3_golden_fp.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d KB)" % (path, os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()
