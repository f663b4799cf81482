#!/usr/bin/env python3
"""Generate tests/golden/geoa3_golden_uniform.npz from the REFERENCE's own uniform_loss (build container only).

Run:  python tests/golden/make_golden_uniform.py            (needs /root/reference; CPU only)

Lib/loss_utils.py:151-189 calls `pointnet2_utils` without importing it (--uniform_loss_weight != 0 dies with a NameError,
geoA3_attack.py:170).  Here the module attribute is set at run time to the reference's own
pointnet2_ops.pointnet2_utils, whose `_ext` is the CPU oracle (make_golden.install_shims): the one missing import, added
from outside, nothing copied.  Stored: inputs, the loss, its adv_pc gradient, the sampler's and the ball queries'
indices, and short attack trajectories with uniform_loss_weight != 0 in the ATK_CASES shape.
"""
from __future__ import annotations

import io
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, O, install_shims, ref_cfg, t2n  # noqa: E402

# tag -> (B, N, seed, mode, kwargs of uniform_loss); mode: "normal", "dupzero" (duplicates + points near the origin that
# the sampler skips), "bn3" (a [B,N,3] argument)
UNI_CASES = {
    "n188": (2, 188, 51, "normal", {}),
    "n256": (3, 256, 52, "normal", {}),
    "n1024": (2, 1024, 53, "normal", {}),
    "n2048": (1, 2048, 54, "normal", {}),
    "dupzero": (2, 256, 55, "dupzero", {}),
    "custom": (2, 512, 56, "normal", dict(percentages=[0.01, 0.02, 0.005], radius=0.5, k=4)),
    "bn3": (2, 256, 57, "bn3", {}),
}
DEFAULT_PCTS = [0.004, 0.006, 0.008, 0.010, 0.012]

# tag -> (cfg overrides, targeted, batch, seed, N)
UNI_ATK_CASES = {
    "untarget_ce": (dict(uniform_loss_weight=1.0, curv_loss_knn=4, binary_max_steps=2, iter_max_steps=5, lr=0.002),
                    False, 3, 61, 256),
    "target_margin": (dict(uniform_loss_weight=0.5, attack_label="All", cls_loss_type="Margin", curv_loss_knn=4,
                           binary_max_steps=2, iter_max_steps=5, lr=0.003, initial_const=0.5), True, 3, 62, 256),
}


def uni_cloud(B, N, seed, mode):
    ori, _ = O.make_synthetic_clouds(B, N, seed)
    g = torch.Generator().manual_seed(seed + 500)
    x = ori + torch.randn(B, 3, N, generator=g) * 0.01
    if mode == "dupzero":
        x[:, :, 1] = x[:, :, 0]
        x[:, :, 7] = x[:, :, 3]
        x[:, :, 8] = x[:, :, 3]
        x[:, :, 11] = 0.01        # |p|^2 <= 1e-3: never sampled
        x[:, :, 20] = 0.0
    return x.contiguous()


def main():
    if not os.path.isdir(REF):
        sys.exit("needs /root/reference (build container only)")
    install_shims()
    import loss_utils as RL                       # reference Lib/loss_utils.py
    from pointnet2_ops import pointnet2_utils as PU   # reference Model/pointnet2_ops_lib/pointnet2_ops/pointnet2_utils.py
    RL.pointnet2_utils = PU                       # the import Lib/loss_utils.py lacks
    from PointNet import PointNet as RefPointNet
    from Attacker import geoA3_attack as RA

    out = {}
    for tag, (B, N, seed, mode, kw) in UNI_CASES.items():
        x = uni_cloud(B, N, seed, mode)
        arg = x.permute(0, 2, 1).contiguous() if mode == "bn3" else x
        arg = arg.clone().requires_grad_()
        loss = RL.uniform_loss(arg, **kw)
        (g,) = torch.autograd.grad(loss, arg)
        pre = "uni/%s/" % tag
        out[pre + "x"] = t2n(arg)
        out[pre + "loss"] = t2n(loss).astype(np.float32)
        out[pre + "grad"] = t2n(g)
        pcts = kw.get("percentages", DEFAULT_PCTS)
        radius = kw.get("radius", 1.0)
        out[pre + "percentages"] = np.asarray(pcts, dtype=np.float64)
        out[pre + "radius"] = np.float64(radius)
        out[pre + "k"] = np.int64(kw.get("k", 2))
        # the indices the reference's loss saw (the same calls, Lib/loss_utils.py:156-169)
        pm = x.permute(0, 2, 1).contiguous()
        npoint = int(N * 0.05)
        fps = PU.furthest_point_sample(pm, npoint)
        out[pre + "fps"] = t2n(fps).astype(np.int16)
        centres = PU.gather_operation(x.contiguous(), fps).transpose(1, 2).contiguous()
        for i, p in enumerate(pcts):
            p = p * 4
            nsample = int(N * p)
            r = float(np.sqrt(p * radius))
            out[pre + "bq%d" % i] = t2n(PU.ball_query(r, nsample, pm, centres)).astype(np.int16)
    out["uni/cases"] = np.array(list(UNI_CASES))

    sd = O.make_pointnet_state_dict(40, seed=0)
    net = RefPointNet(40)
    net.load_state_dict(sd)
    net.eval()

    for tag, (kw, targeted, b, seed, N) in UNI_ATK_CASES.items():
        cfg = ref_cfg(**kw)
        ori, nrm = O.make_synthetic_clouds(b, N, seed)
        with torch.no_grad():
            gt = net(ori).argmax(1)
        tgt = (gt + 5) % 40
        g = torch.Generator().manual_seed(seed + 1000)
        inits = [torch.randn(b, 3, N, generator=g) * 1e-3 for _ in range(cfg.binary_max_steps)]
        it = iter(inits)

        def fake_normal_(t, mean=0.0, std=1.0):
            with torch.no_grad():
                t.copy_(next(it))
            return t

        real_normal_ = nn.init.normal_
        nn.init.normal_ = fake_normal_
        tr = dict(x=[], loss_n=[], constrain=[], logits=[])
        real_fs = RA._forward_step

        def fs_spy(net_, pc_ori, x, *a, **k):
            r = real_fs(net_, pc_ori, x, *a, **k)
            tr["x"].append(x.detach().clone())
            tr["loss_n"].append(r[3].detach().clone())
            c = r[8].detach().clone() if torch.is_tensor(r[8]) else torch.zeros(b)
            tr["constrain"].append(c.expand(b).clone() if c.dim() == 0 else c)
            tr["logits"].append(r[0].detach().clone())
            return r

        RA._forward_step = fs_spy
        data = [ori.permute(0, 2, 1).unsqueeze(1).contiguous(), nrm.permute(0, 2, 1).unsqueeze(1).contiguous(),
                gt.view(b, 1)]
        if targeted:
            data.append(tgt.view(b, 1))
        so = sys.stdout
        sys.stdout = io.StringIO()
        try:
            best, target, succ, best_step, all_loss = RA.attack(net, data, cfg, 0, 1, None)
        finally:
            sys.stdout = so
            nn.init.normal_ = real_normal_
            RA._forward_step = real_fs
        pre = "atk/%s/" % tag
        out[pre + "ori"], out[pre + "nrm"], out[pre + "gt"], out[pre + "tgt"] = map(t2n, (ori, nrm, gt, tgt))
        out[pre + "inits"] = np.stack([t2n(t) for t in inits])
        out[pre + "best_attack"], out[pre + "target"] = t2n(best), t2n(target)
        out[pre + "success"] = np.asarray(succ)
        out[pre + "best_step"] = np.asarray(best_step, dtype=np.int64)
        out[pre + "all_loss"] = np.asarray(all_loss, dtype=np.float32)
        out[pre + "tr_x"] = np.stack([t2n(t) for t in tr["x"]])
        out[pre + "tr_loss_n"] = np.stack([t2n(t) for t in tr["loss_n"]])
        out[pre + "tr_constrain"] = np.stack([t2n(t) for t in tr["constrain"]])
        out[pre + "tr_logits"] = np.stack([t2n(t) for t in tr["logits"]])
    out["atk/cases"] = np.array(list(UNI_ATK_CASES))

    path = os.path.join(HERE, "geoa3_golden_uniform.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d KB)" % (path, os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()
