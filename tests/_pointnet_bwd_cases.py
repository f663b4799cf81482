"""The inputs of the isolated tests of the PointNet backward kernels (tests/test_gpu_pointnet_bwd.py runs them on the GPU,
tests/test_pointnet_bwd_ref.py shows on the CPU that each case's bound would notice a single lost term).  Plain torch, fp32
values, deterministic; the float64 references are evaluations of exactly these values.

The seeds of the cases that recompute the first layer's gate were searched on the CPU so that no pre-activation lies
within the fp32 rounding of zero (R.gate_margin_ok): the CPU test asserts it for every such case, none excluded.
"""
from __future__ import annotations

import torch

from tests import _pointnet_bwd_ref as R

B = 3

# ---------------------------------------------------------------------------------------------------------------------
# sparse arg-max backward (wide_bwd, wide_bwd_conv)
# ---------------------------------------------------------------------------------------------------------------------
SPARSE_SHAPES = [(taps, N) for taps in (1, 3) for N in (64, 77, 130, 200)]
STRESS_SHAPE = (3, 77)      # the stress sibling (g over twelve decades) of the ("uniform") case of this shape


def sparse_patterns(taps, N):
    """arg-max patterns: uniform; every channel on ONE column (column 0 / N - 1: with three taps one tap falls outside
    [0, N); 63 / 64: the taps cross the tile boundary; every wave's share starts inside the column: side rows); hits in
    one tile only (the others walk empty lists); fewer than eight hits in a tile (waves without a share)."""
    cols = sorted({c for c in (0, 63, 64, N - 1) if c < N})
    return ["uniform"] + ["col%d" % c for c in cols] + ["onetile", "few"]


def sparse_case(taps, N, pattern, stress=False, batch=B):
    gen = torch.Generator().manual_seed(1000 * taps + N + 7 * len(pattern) + (int(pattern[3:]) if pattern[:3] == "col" else 0))
    r = lambda *s: torch.rand(*s, generator=gen)
    W = torch.randn(1024, taps * 128, generator=gen) * 0.05
    W2t = torch.randn(64, 128, generator=gen) * 0.1
    g = (0.5 + r(batch, 1024)) * torch.where(r(batch, 1024) < 0.5, -1.0, 1.0)
    g[r(batch, 1024) < 0.25] = 0.0                       # zeros and both signs
    arg = torch.randint(0, N, (batch, 1024), generator=gen)
    if pattern.startswith("col"):
        arg[:] = int(pattern[3:])
    elif pattern == "onetile":
        t = 1 if N > 64 else 0
        lo, hi = 64 * t, min(64 * t + 64, N)
        arg = torch.randint(lo + taps // 2, hi - taps // 2, (batch, 1024), generator=gen)
    elif pattern == "few":
        keep = torch.zeros(batch, 1024, dtype=torch.bool)
        for b in range(batch):
            p = torch.randperm(1024, generator=gen)
            keep[b, p[:5]] = True
            arg[b, p[:5]] = torch.randint(1, 62, (5,), generator=gen)
            if N > 64 + 2:
                keep[b, p[5:8]] = True
                arg[b, p[5:8]] = torch.randint(65, N - 1, (3,), generator=gen)
        g = torch.where(keep, torch.where(g == 0, torch.ones_like(g), g), torch.zeros_like(g))
    if stress:
        g = g * 10.0 ** (12.0 * r(batch, 1024) - 6.0)
    gate128 = r(batch, 128, N) < 0.5
    gate64 = r(batch, 64, N) < 0.5
    if batch > 1:
        gate128[1, 7] = False                            # an all-zero gate row
        gate64[1, 3] = False
    return dict(taps=taps, N=N, pattern=pattern, stress=stress, g=g, arg=arg.to(torch.int32), W=W, W2t=W2t,
                gate128=gate128, gate64=gate64)


FIRST_SHAPES = [(64, "uniform"), (77, "uniform"), (77, "col76"), (200, "uniform"), (200, "col64")]
FIRST_SEEDS = {(64, "uniform"): 0, (77, "uniform"): 0, (77, "col76"): 0, (200, "uniform"): 0, (200, "col64"): 0}


def first_case(N, pattern, seed=None):
    """the first-layer form: a sparse case with one tap, the cloud, the 3 -> 64 layer and a prefilled dx3"""
    c = sparse_case(1, N, pattern)
    gen = torch.Generator().manual_seed(50000 + 131 * N + (FIRST_SEEDS[(N, pattern)] if seed is None else seed))
    c["x3"] = torch.randn(B, 3, N, generator=gen)
    c["w1"] = torch.randn(64, 3, generator=gen)
    c["b1"] = torch.randn(64, generator=gen) * 0.5
    c["dx3_in"] = torch.randn(B, 3, N, generator=gen)
    return c


# ---------------------------------------------------------------------------------------------------------------------
# Gram product
# ---------------------------------------------------------------------------------------------------------------------
GRAM_N = [1, 63, 64, 65, 129, 200, 385, 512, 897]     # parts 1 / 4 (385, 512) / 8 (897); ragged half-chunks and chunks


def gram_variants(N):
    v = ["uniform", "inst_zero", "inst_tiny"]
    if N > 128:
        v += ["chunk_big", "chunk_zero"]
    return v


def gram_case(N, variant):
    """stress variants (exempt from the sensitivity condition; "uniform" is their sibling at the same shape): chunk_big
    -- the second 128-column chunk of A at 1e6 times the others; inst_tiny -- instance 1 of A scaled by 1e-30."""
    gen = torch.Generator().manual_seed(7000 + N)
    A = torch.randn(B, 64, N, generator=gen)
    G = torch.randn(B, 64, N, generator=gen)
    if variant == "inst_zero":
        A[1] = 0
        G[1] = 0
    elif variant == "inst_tiny":
        A[1] *= 1e-30
    elif variant == "chunk_big":
        A[:, :, 128:256] *= 1e6
    elif variant == "chunk_zero":
        lo = 128 * ((N - 1) // 128)
        A[:, :, lo:] = 0
        G[:, :, lo:] = 0
    return dict(N=N, variant=variant, A=A, G=G, stress=variant in ("chunk_big", "inst_tiny"))


# ---------------------------------------------------------------------------------------------------------------------
# backward chain
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_N = [64, 77, 256, 257, 300, 1000]   # one / several 256-column workgroups; 257: three dead waves and one with one column
CHAIN_SEEDS = {64: 0, 77: 0, 256: 0, 257: 0, 300: 0, 1000: 1}


def chain_case(N, seed=None):
    gen = torch.Generator().manual_seed(90000 + 17 * N + (CHAIN_SEEDS[N] if seed is None else seed))
    rn = lambda *s: torch.randn(*s, generator=gen)
    c = dict(N=N, Xa=rn(B, 64, N), Xb=rn(B, 64, N), Wa=rn(B, 64, 64) * 0.1, Wb=rn(64, 64) * 0.1, W2t=rn(64, 64) * 0.1,
             x3=rn(B, 3, N), T3=torch.eye(3).expand(B, 3, 3) + 0.3 * rn(B, 3, 3), w1=rn(64, 3), b1=rn(64) * 0.5)
    c["gate_h2"] = torch.rand(B, 64, N, generator=gen) < 0.5
    c["gate_h2"][2, 11] = False
    return c


# ---------------------------------------------------------------------------------------------------------------------
# fully connected layers
# ---------------------------------------------------------------------------------------------------------------------
FC_SHAPES = [(512, 1024), (256, 512), (40, 256), (9, 256), (4096, 256),        # (Nout, K): the forward heads ...
             (256, 40), (256, 9), (512, 256), (1024, 512), (256, 4096)]         # ... and the backward's
FC_M = [1, 5, 17, 33]


def fc_case(M, Nout, K, mode):
    """mode "z": no bias, gated by Z > 0 (the backward's layers); "br": bias + relu (the forward's)"""
    gen = torch.Generator().manual_seed(M * 100003 + Nout * 17 + K)
    c = dict(M=M, Nout=Nout, K=K, mode=mode, X=torch.randn(M, K, generator=gen), W=torch.randn(Nout, K, generator=gen) * 0.1)
    c["bias"] = torch.randn(Nout, generator=gen) if mode == "br" else None
    c["Z"] = torch.randn(M, Nout, generator=gen) if mode == "z" else None
    return c


def fc_reference(c, **defects):
    return R.fc(c["X"].double(), c["W"].double(), None if c["bias"] is None else c["bias"].double(), c["mode"] == "br",
                None if c["Z"] is None else c["Z"] > 0, **defects)


# ---------------------------------------------------------------------------------------------------------------------
# references and bounds of the cases: (ref, tol) in float64
# ---------------------------------------------------------------------------------------------------------------------
def d(c, *names):
    return [c[n].double() if c[n].is_floating_point() else c[n] for n in names]


def sparse_terms(c):
    return R.column_terms(c["g"], c["arg"], c["N"], c["taps"])


def wide_bwd_reference(c, dtype=torch.float64, **defects):
    """n = the most terms in one column's sum"""
    ref, mag = R.wide_bwd(c["g"].to(dtype), c["arg"], c["W"].to(dtype), c["gate128"], c["taps"], **defects)
    return ref, R.tolerance(ref.double(), mag.double(), max(1, sparse_terms(c)))


def wide_bwd_conv_reference(c, dtype=torch.float64, **defects):
    """n = the column's sum, then the 128-term product with W2t on top of it"""
    ref, mag = R.wide_bwd_conv(c["g"].to(dtype), c["arg"], c["W"].to(dtype), c["gate128"], c["taps"], c["W2t"].to(dtype),
                               c["gate64"], **defects)
    return ref, R.tolerance(ref.double(), mag.double(), sparse_terms(c) + 128)


def first_reference(c, dtype=torch.float64, **defects):
    """n = column sum + 128 (W2t) + 64 (w1^T) + 1 (the value dx3 held)"""
    gate = R.first_layer_pre(*d(c, "x3", "w1", "b1"))[0] > 0
    ref, mag = R.wide_bwd_conv_first(c["g"].to(dtype), c["arg"], c["W"].to(dtype), c["gate128"], c["W2t"].to(dtype),
                                     c["x3"].to(dtype), c["w1"].to(dtype), c["b1"].to(dtype), c["dx3_in"].to(dtype),
                                     gate_first=gate, **defects)
    return ref, R.tolerance(ref.double(), mag.double(), sparse_terms(c) + 128 + 64 + 1)


GRAM_SPLIT = 2.0 ** -21     # see test_gram_against_float64 (tests/test_gpu_pointnet_bwd.py)


def gram_reference(c, dtype=torch.float64, **defects):
    ref, mag = R.gram(c["A"].to(dtype), c["G"].to(dtype), **defects)
    return ref, R.tolerance(ref.double(), mag.double(), c["N"], extra=GRAM_SPLIT)


CHAIN_DX_TERMS = 64 + 64 + 64 + 64 + 3     # Wa^T Xa + Wb^T Xb, W2t, w1^T, T3


def chain_reference(c, dtype=torch.float64, **defects):
    """-> (dx, tol_dx, dT, tol_dT); the gates are the float64 ones whatever the dtype"""
    gate = R.first_layer_pre(*d(c, "x3", "w1", "b1", "T3"))[0] > 0
    t = lambda n: c[n].to(dtype)
    dx, mdx, dT, mdT = R.bwd_chain(t("Xa"), t("Wa"), t("Xb"), t("Wb"), c["gate_h2"], t("W2t"), t("x3"), t("T3"), t("w1"),
                                   t("b1"), gate_first=gate, **defects)
    return (dx, R.tolerance(dx.double(), mdx.double(), CHAIN_DX_TERMS), dT, R.tolerance(dT.double(), mdT.double(), c["N"]))
