"""The inputs of the isolated tests of the PointNet forward's trunk kernels (tests/test_gpu_pointnet_fwd.py runs them on the
GPU, tests/test_pointnet_fwd_ref.py shows on the CPU that each case's bound notices a defect, that a plain fp32 evaluation
stays inside it and that it leaves at most 0.5 % of a case's gate bits open).  Plain torch, fp32 values, deterministic; the
float64 references are evaluations of exactly these values.

Kinds (the three chain kernels, and stage by stage the single-layer forms they replace):
    c1   cloud -> first layer -> 128                      conv_chain_kernel<1,true,128>   (T-Net 3's conv1 + conv2)
    c3   cloud -> first layer -> 64 -> 64 -> 128          conv_chain_kernel<3,true,128>   (h2 stored, c1 bits only, c2 stored)
    x2   X [B,64,N] -> 64 (per-instance W) -> 128         conv_chain_kernel<2,false,128>  (h3 bits only, h4 stored)

Magnitudes.  The 64 input rows of the first stage are spread "asc" (the per-wave activation scale has to shrink at a later
16-row chunk and rescale its sums), "desc" (the scale is kept), or "flush" (first chunk ~1e-30, second ~1e+10: the rescale
factor underflows and the sums are flushed).  X-fed: rows x logspace(-4, 3); cloud-fed: the rows of w1 / b1 over five decades.
Instance 2 is all zero, instance 3 scaled by 1e-12.  x2's per-instance weights differ by 1e-3 / 1e3 / 1 / 1 (instances 0 and
1 carry the inverse factor in X, so every instance's output stays comparable with the shared biases).  Biases are about 1 % of
the stage's largest activation.  The rows of ONE weight block share a magnitude: the split product scales a 64-row block by
its own maximum and keeps 2^-38 of it, so a row 1e-7 of its block's maximum would lose its low pieces by design.
"""
from __future__ import annotations

import functools

import torch

from tests import _pointnet_fwd_ref as R

B = 4
CHAIN_N = [1, 63, 64, 65, 77, 256, 257, 300]      # 77: two dead wavefronts in the only column block; 257 / 300: two blocks
KINDS = ("c1", "c3", "x2")
STORED = {"c1": (True,), "c3": (True, False, True), "x2": (False, True)}
STAGE_NAMES = {"c1": ("a2",), "c3": ("h2", "c1", "c2"), "x2": ("h3", "h4")}
OPEN_CAP = 0.005                                   # share of a case's gate bits the bound may leave open

# the large launches: a chain whose workgroups walk two column blocks, a single layer on more than 512 workgroups
LARGE_B = 257
LARGE_CHAIN_N = 513                                # 3 column blocks x 257 > 768: two workgroups per instance, one walks two
LARGE_CONV_N = 256                                 # split kernel: 2 x 1 x 257 = 514 workgroups
LARGE_ROWS = [0, 1, 2, 128, 129, 130, 254, 255, 256]


def variants(kind):
    """(row spread, with T3) of the cloud-fed kinds, (row spread,) of x2"""
    if kind == "x2":
        return [("asc",), ("desc",), ("flush",)]
    return [("asc", True), ("asc", False), ("desc", True), ("flush", False)]


def _spread(how, lo, hi):
    if how == "flush":
        return torch.cat([torch.full((16,), 1e-30), torch.full((16,), 1e10), torch.logspace(8, 10, 32)])
    s = torch.logspace(lo, hi, 64)
    return s if how == "asc" else s.flip(0)


def _bias_for(h64, W, gen):
    """randn x 1 % of the largest activation of relu(W h), fp32"""
    top = float(R.stage(h64, W.double(), torch.zeros(W.shape[-2], dtype=torch.float64))["y"].max())
    return (torch.randn(W.shape[-2], generator=gen) * (0.01 * max(top, 1e-30))).float()


def chain_case(kind, N, variant, batch=B):
    """-> dict: either X, or x3 / T3 (None) / w1 / b1; stages = [(W, bias), ...] (x2's first W is [batch,64,64])"""
    how = variant[0]
    seed = 100000 * KINDS.index(kind) + 100 * N + 10 * ("asc", "desc", "flush").index(how) + (len(variant) > 1 and variant[1])
    gen = torch.Generator().manual_seed(int(seed) + 7 * batch)
    rn = lambda *s: torch.randn(*s, generator=gen)
    c = {"kind": kind, "N": N, "B": batch}
    if kind == "x2":
        X = rn(batch, 64, N) * _spread(how, -4, 3).view(1, 64, 1)
        inst = torch.ones(batch)
        inst[0], inst[1] = 1e-3, 1e3
        X = X / inst.view(-1, 1, 1)
        X[2] = 0.0
        X[3] *= 1e-12
        c["X"] = X.contiguous()
        h = X.double()
        W0 = rn(batch, 64, 64) * 0.1 * inst.view(-1, 1, 1)
        shapes = [None, (128, 64)]
    else:
        x3 = rn(batch, 3, N) * 0.5
        x3[2] = 0.0
        x3[3] *= 1e-12
        rows = _spread(how, -2, 3)
        c["x3"] = x3.contiguous()
        c["T3"] = (torch.eye(3) + 0.5 * rn(batch, 3, 3)).contiguous() if variant[1] else None
        c["w1"] = (rn(64, 3) * rows.view(64, 1)).contiguous()
        c["b1"] = (rn(64) * 0.3 * rows).contiguous()
        h = R.first_layer(x3.double(), c["w1"].double(), c["b1"].double(), None if c["T3"] is None else c["T3"].double())["y"]
        W0 = None
        shapes = [(128, 64)] if kind == "c1" else [(64, 64), (64, 64), (128, 64)]
    stages = []
    for i, shp in enumerate(shapes):
        W = (W0 if shp is None else rn(*shp) * 0.1).contiguous()
        bias = _bias_for(h, W, gen)
        stages.append((W, bias))
        h = R.stage(h, W.double(), bias.double())["y"]
    c["stages"] = stages
    return c


def select(c, rows):
    """the case restricted to the instances `rows`"""
    pick = lambda t: None if t is None else t[rows].contiguous()
    out = dict(c, B=len(rows))
    for k in ("X", "x3", "T3"):
        if k in c:
            out[k] = pick(c[k])
    out["stages"] = [(pick(W) if W.dim() == 3 else W, b) for (W, b) in c["stages"]]
    return out


def reference_of(c, defect=None, dtype=torch.float64):
    """(layers, first) of tests/_pointnet_fwd_ref.chain on the case's values in `dtype`"""
    d = lambda t: None if t is None else t.to(dtype)
    stages = [(d(W), d(b)) for (W, b) in c["stages"]]
    if "X" in c:
        return R.chain(stages, X=d(c["X"]), defect=defect)
    return R.chain(stages, cloud=(d(c["x3"]), d(c["T3"]), d(c["w1"]), d(c["b1"])), defect=defect)


@functools.lru_cache(maxsize=None)
def case_and_reference(kind, N, variant):
    """the case and its float64 reference, computed once per session and shared (read only) by the tests"""
    c = chain_case(kind, N, variant)
    return c, reference_of(c)


def all_cases():
    return [(kind, N, v) for kind in KINDS for N in CHAIN_N for v in variants(kind)]


@functools.lru_cache(maxsize=None)
def large_chain_case():
    """c3 at N = 513, B = 257 with a per-instance T3, and the float64 reference of LARGE_ROWS"""
    c = chain_case("c3", LARGE_CHAIN_N, ("asc", True), batch=LARGE_B)
    return c, reference_of(select(c, LARGE_ROWS))


@functools.lru_cache(maxsize=None)
def large_conv_case():
    """one 64 -> 128 layer on X [257,64,256] (rows ascending), and the float64 reference of LARGE_ROWS"""
    gen = torch.Generator().manual_seed(257256)
    X = torch.randn(LARGE_B, 64, LARGE_CONV_N, generator=gen) * torch.logspace(-4, 3, 64).view(1, 64, 1)
    X[2] = 0.0
    X[3] *= 1e-12
    W = (torch.randn(128, 64, generator=gen) * 0.1).contiguous()
    bias = _bias_for(X[:4].double(), W, gen)
    c = {"kind": "x1", "N": LARGE_CONV_N, "B": LARGE_B, "X": X.contiguous(), "stages": [(W, bias)]}
    return c, reference_of(select(c, LARGE_ROWS))
