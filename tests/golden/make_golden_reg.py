#!/usr/bin/env python3
"""Generate tests/golden/geoa3_golden_reg.npz from the REFERENCE's own displacement_loss / corresponding_normal_loss /
repulsion_loss / kNN_smoothing_loss (Lib/loss_utils.py:99-149; build container only).

Run:  python tests/golden/make_golden_reg.py            (needs /root/reference; CPU only)

Per case: the inputs, the reference's float32 value, its autograd gradient w.r.t. adv_pc under a random upstream gradient
(stored), the same two from a float64 evaluation of the same function, and e_ref = max |float32 - float64| per output --
the reference's own rounding error, which the GPU tests take their bound from.  Also the K-NN indices the reference's
selection amounts to, the mask of kNN_smoothing_loss, and the four signatures (names, parameter names, defaults) as data.

A case is refused (the script stops) when the reference alone is not a well-posed yardstick for it:
  (a) the functions whose result depends on WHICH neighbours are selected (displacement_loss, corresponding_normal_loss;
      and the duplicate-point cases of the other two, whose gradient is scattered to the selected indices) need a gap
      between the k-th and the (k+1)-th neighbour distance above 1e-6 relative at every point;
  (b) kNN_smoothing_loss needs every s_i farther than 1e-5 thr from the threshold (float32 and float64).
"""
from __future__ import annotations

import inspect
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, REPO, O, install_shims, t2n  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))
import _reg_ref as R  # noqa: E402

# cloud tag -> (B, N, seed, duplicates)   (dup256: the first seed from 75 on whose duplicates pass condition (a) at k = 4)
CLOUDS = {"n64": (2, 64, 71, False), "n200": (2, 200, 72, False), "n256": (2, 256, 73, False),
          "n1024": (1, 1024, 74, False), "dup256": (2, 256, 80, True)}
# function -> [(cloud tag, kwargs)]
CASES = {
    "kNN_smoothing_loss": [("n64", dict(k=5)), ("n200", dict(k=8, threshold_coef=1.10)),
                           ("n256", dict(k=5, threshold_coef=1.10)), ("n1024", dict(k=5, threshold_coef=1.10)),
                           ("dup256", dict(k=4, threshold_coef=1.10))],
    "repulsion_loss": [("n64", dict()), ("n200", dict(k=7, h=0.05)), ("n256", dict()), ("n1024", dict()),
                       ("dup256", dict(k=4))],
    "displacement_loss": [("n64", dict()), ("n200", dict(k=5)), ("n256", dict()), ("n1024", dict())],
    "corresponding_normal_loss": [("n64", dict()), ("n200", dict(k=6)), ("n256", dict()), ("n1024", dict())],
}
NAMES = list(CASES)


def make_cloud(B, N, seed, dup):
    ori, nrm = O.make_synthetic_clouds(B, N, seed)
    g = torch.Generator().manual_seed(seed + 500)
    x = ori + torch.randn(B, 3, N, generator=g) * 0.01
    if dup:   # exact duplicates: pairs and one triple
        for a, c in ((1, 0), (7, 3), (8, 3), (100, 40), (255, 254)):
            x[:, :, a] = x[:, :, c]
    return x.contiguous(), ori.contiguous(), nrm.contiguous()


def check_gap(cloud, k, what):
    d = R.knn_self(cloud, k + 2)[0]
    gap = d[:, :, k + 1] - d[:, :, k]
    if not bool((gap > 1e-6 * d[:, :, k + 1]).all()):
        sys.exit("refused (a): %s has a point whose k-th and (k+1)-th neighbours are closer than 1e-6 relative" % what)


def main():
    if not os.path.isdir(REF):
        sys.exit("needs /root/reference (build container only)")
    install_shims()
    import loss_utils as RL                       # reference Lib/loss_utils.py

    out = {}
    clouds = {}
    for tag, (B, N, seed, dup) in CLOUDS.items():
        clouds[tag] = make_cloud(B, N, seed, dup)
        for name, v in zip(("x", "ori", "nrm"), clouds[tag]):
            out["cloud/%s/%s" % (tag, name)] = t2n(v)
    for fi, fname in enumerate(NAMES):
        fn = getattr(RL, fname)
        sig = inspect.signature(fn)
        out["api/%s/params" % fname] = np.array(list(sig.parameters))
        out["api/%s/defaults" % fname] = np.array([("" if p.default is inspect.Parameter.empty else repr(p.default))
                                                   for p in sig.parameters.values()])
        tags = []
        for tag, kw in CASES[fname]:
            x, ori, nrm = clouds[tag]
            B, _, N = x.shape
            k = kw.get("k", sig.parameters["k"].default)
            what = "%s/%s" % (fname, tag)
            if fname == "displacement_loss":
                rest, table_cloud = (ori,), ori
                check_gap(ori, k, what)
                check_gap(ori.double(), k, what)
            elif fname == "corresponding_normal_loss":
                rest, table_cloud = (nrm,), x
                check_gap(x, k, what)
                check_gap(x.double(), k, what)
            else:
                rest, table_cloud = (), x
                if CLOUDS[tag][3]:
                    check_gap(x, k, what)
                    check_gap(x.double(), k, what)
            if fname == "kNN_smoothing_loss":
                coef = kw.get("threshold_coef", sig.parameters["threshold_coef"].default)
                for xx in (x, x.double()):
                    s, thr, c = R.smoothing_parts(xx, k, coef)
                    if bool(((s - thr.unsqueeze(1)).abs() <= 1e-5 * thr.unsqueeze(1)).any()):
                        sys.exit("refused (b): %s has a point within 1e-5 thr of the threshold" % what)
                    if not bool(c.any()):
                        sys.exit("refused: %s keeps no point" % what)
                out["%s/%s/cond" % (fname, tag)] = t2n(R.smoothing_parts(x, k, coef)[2]).astype(np.uint8)
            gen = torch.Generator().manual_seed(9000 + 10 * fi + len(tags))
            xa = x.clone().requires_grad_()
            val = fn(xa, *rest, **kw)
            g = torch.randn(val.shape, generator=gen)
            (grad,) = torch.autograd.grad(val, xa, g)
            xd = x.double().clone().requires_grad_()
            val64 = fn(xd, *[r.double() for r in rest], **kw)
            (grad64,) = torch.autograd.grad(val64, xd, g.double())
            assert val.dtype == torch.float32 and val64.dtype == torch.float64
            pre = "%s/%s/" % (fname, tag)
            out[pre + "kw_names"] = np.array(list(kw))
            out[pre + "kw_values"] = np.array([float(v) for v in kw.values()], dtype=np.float64)
            out[pre + "g"] = t2n(g)
            out[pre + "value"], out[pre + "grad"] = t2n(val.detach()), t2n(grad)
            out[pre + "value64"], out[pre + "grad64"] = t2n(val64.detach()), t2n(grad64)
            out[pre + "e_ref_value"] = np.float64((val.detach().double() - val64.detach()).abs().max().item())
            out[pre + "e_ref_grad"] = np.float64((grad.double() - grad64).abs().max().item())
            # the neighbours the reference's selection amounts to (ascending by (distance, index), column 0 dropped)
            out[pre + "knn_idx"] = t2n(O.knn_points(table_cloud.permute(0, 2, 1), table_cloud.permute(0, 2, 1), k + 1)[1]
                                       [:, :, 1:]).astype(np.int16)
            tags.append(tag)
        out["%s/cases" % fname] = np.array(tags)
    out["api/names"] = np.array(NAMES)

    path = os.path.join(HERE, "geoa3_golden_reg.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d KB)" % (path, os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()
