"""The inputs of the cases tests/test_gpu_pn2_kernels.py runs on the GPU and tests/test_pn2_native_ref.py runs through the
CPU emulation (tests/_pn2_native_ref.py), with each case's float64 reference and bound.  Seeded: a case is the same tensors
in both files.  Index tables only ever hold indices inside their tables."""
from __future__ import annotations

import functools

import numpy as np
import torch

from tests import _pn2_native_ref as R

# ---------------------------------------------------------------------------------------------------------------------
# frag_image
# ---------------------------------------------------------------------------------------------------------------------
FRAG_CASES = [(32, 16, "random"), (128, 128, "random"), (256, 128, "random"), (1024, 512, "random"),
              (128, 128, "zeros"), (128, 128, "spike")]


def frag_case(Rw, K, variant):
    g = torch.Generator().manual_seed(1000 + Rw + K)
    W = torch.randn(Rw, K, generator=g) / (K ** 0.5)
    if variant == "zeros":
        W.zero_()
    elif variant == "spike":          # a single entry 2^20 times the rest: their low pieces are fp16 subnormals
        W[Rw // 2 + 1, K // 2 + 3] = float(W.abs().max()) * 2.0 ** 20
    return W


# ---------------------------------------------------------------------------------------------------------------------
# sa2_pre
# ---------------------------------------------------------------------------------------------------------------------
# (P, Np): Np = 0 point-major, else channel-major [P / Np][128][Np].  P = 32: one wavefront; 96: a partial workgroup; 544 =
# 17 tiles: five workgroups, the last with one tile.  The launcher gives every four tiles a workgroup of their own up to 512
# workgroups, so a wavefront takes a SECOND tile only beyond 2048 tiles: 65568 points = 2049 tiles.
PRE_SHAPES = [(32, 0), (96, 0), (544, 0), (65568, 0), (64, 32), (1024, 512)]
PRE_STRESS = ["point_big", "zero_feat_tile"]
WX_RATIOS = [1.0 / 64, 1.0, 3.0, 16.0, 256.0]
PRE_TERMS = 128 + 3


@functools.lru_cache(maxsize=None)
def pre_case(P, Np=0, variant="random", ratio=None):
    """-> dict f (the layout Np names), xyz [P][3], Wf [128][128], Wx [128][3] (float32)"""
    g = torch.Generator().manual_seed(2000 + P + 7 * Np + (0 if ratio is None else int(ratio * 64)))
    X = torch.randn(P, 128, generator=g).clamp_min(0)            # level 1's features: after a relu
    xyz = torch.rand(P, 3, generator=g) * 0.8 - 0.4
    Wf = torch.randn(128, 128, generator=g) / 128 ** 0.5
    Wx = torch.randn(128, 3, generator=g) * 0.5
    if variant == "point_big":        # one point 2^12 times its 31 tile neighbours
        X[P // 32 // 2 * 32 + 5] *= 2.0 ** 12
    elif variant == "zero_feat_tile":  # a tile whose scale comes from its coordinates alone
        X[P - 32:] = 0
    if ratio is not None:
        Wx = Wx * (ratio * float(Wf.abs().max()) / float(Wx.abs().max()))
    f = X if Np == 0 else X.reshape(P // Np, Np, 128).permute(0, 2, 1).contiguous()
    return dict(f=f, xyz=xyz, Wf=Wf.contiguous(), Wx=Wx.contiguous(), channel_major=Np != 0, Np=Np, P=P)


def pre_reference(c, with_xyz=True, **defects):
    ref, mag = R.sa2_pre(c["f"].double(), c["xyz"].double() if with_xyz else None, c["Wf"].double(), c["Wx"].double(),
                         channel_major=c["channel_major"], **defects)
    return ref, R.tolerance(ref, mag, PRE_TERMS if with_xyz else 128, extra=R.SPLIT)


# ---------------------------------------------------------------------------------------------------------------------
# sa2_fwd
# ---------------------------------------------------------------------------------------------------------------------
FWD_SHAPES = [(1, 8, 40), (3, 16, 200)]


@functools.lru_cache(maxsize=None)
def fwd_case(B, M, N1, stress=False):
    """gidx from the oracle's ball query on a small cloud (ascending, padded with the first index), with three rows forced:
    centre 1 of cloud 0 a ball of ONE live sample, centre 2 a FULL ball (min(64, N1) distinct points), and in every cloud two
    points of centre 0's ball with identical rows of rT (an exact tie: arg must be the lower sample).
    -> dict rT [B][N1][128], gidx [B][M][64] int32, live [B][M] (distinct samples of a ball), shift [B][128][M], W1, b1, W2, b2,
    tie [B] = (sample position of the tie's second point in centre 0's ball)."""
    from oracle import pointnet2_oracle as O
    g = torch.Generator().manual_seed(3000 + B + M + N1)
    xyz = torch.rand(B, N1, 3, generator=g)
    gidx = O.ball_query(xyz[:, :M].contiguous(), xyz, 0.45, 64).clone()
    gidx[0, 1, :] = gidx[0, 1, 0]
    full = min(64, N1)
    gidx[0, 2, :] = gidx[0, 2, 0] * 0
    gidx[0, 2, :full] = torch.arange(full, dtype=torch.int32)
    live = torch.zeros(B, M, dtype=torch.long)
    for b in range(B):
        for m in range(M):
            row = gidx[b, m]
            n = 1
            while n < 64 and int(row[n]) > int(row[n - 1]):
                n += 1
            live[b, m] = n
    rT = torch.randn(B, N1, 128, generator=g) * 0.5
    tie = torch.zeros(B, dtype=torch.long)
    for b in range(B):
        assert int(live[b, 0]) >= 3
        pos = int(live[b, 0]) - 1                      # the ball's last live sample repeats its second one
        rT[b, int(gidx[b, 0, pos])] = rT[b, int(gidx[b, 0, 1])]
        tie[b] = pos
    shift = torch.randn(B, 128, M, generator=g) * 0.5
    if stress:      # centre 0's gathered rows 2^10 times those of centre 1, its partner in the workgroup's pair
        assert B == 1 and N1 >= 40
        gidx[0, 0, :] = 0
        gidx[0, 0, :20] = torch.arange(20, dtype=torch.int32)
        gidx[0, 1, :] = 20
        gidx[0, 1, :20] = torch.arange(20, 40, dtype=torch.int32)
        live[0, 0] = live[0, 1] = 20
        rT[0, :20] *= 2.0 ** 10
        shift[0, :, 0] *= 2.0 ** 10
        rT[0, 19] = rT[0, 1]
        tie[0] = 19
    W1 = torch.randn(128, 128, generator=g) * (2.0 / 128) ** 0.5
    b1 = torch.randn(128, generator=g) * 0.1
    W2 = torch.randn(256, 128, generator=g) * (2.0 / 128) ** 0.5
    b2 = torch.randn(256, generator=g) * 0.1
    assert int(gidx.min()) >= 0 and int(gidx.max()) < N1
    return dict(B=B, M=M, N1=N1, rT=rT, gidx=gidx.contiguous(), live=live, shift=shift, W1=W1, b1=b1, W2=W2, b2=b2, tie=tie)


@functools.lru_cache(maxsize=None)
def fwd_reference(B, M, N1, stress=False):
    c = fwd_case(B, M, N1, stress)
    r = R.sa2_fwd(c["rT"], c["gidx"], c["shift"], c["W1"], c["b1"], c["W2"], c["b2"])
    r["tol_z1"], r["tol_y2"], r["tol_out"] = R.sa2_fwd_tolerances(r, c["W2"])
    return r


def fwd_checks(c, r, out, arg, m0, m1, z1=None):
    """Everything tests hold a forward's results to (out [B][256][M] float, arg [B][256][M], m0 / m1 [B M][64][4] words):
    -> dict of printed figures.  Raises AssertionError."""
    B, M = c["B"], c["M"]
    res = {}
    gate0 = R.unpack_gate_words(m0.reshape(B, M, 64, 4))
    assert torch.equal(gate0, r["a0"] > 0), "m0 differs from the float32 a0 > 0"
    gate1 = R.unpack_gate_words(m1.reshape(B, M, 64, 4))
    clear = r["z1"].abs() > r["tol_z1"]
    res["band"] = 1.0 - float(clear.double().mean())
    assert res["band"] <= 1e-3, "too many z1 entries inside their own tolerance of zero: %g" % res["band"]
    assert torch.equal(gate1[clear], (r["z1"] > 0)[clear]), "m1 differs from sign(z1) outside the band"
    res["out"] = R.worst_ratio(out, r["out"], r["tol_out"])
    assert res["out"] <= 1.0, "out: worst err / tol = %g" % res["out"]
    a = arg.long()
    assert int(a.min()) >= 0 and int(a.max()) < 64
    assert bool((a < c["live"].view(B, 1, M)).all()), "arg names a padded sample"
    at = torch.gather(r["y2"], 3, a.unsqueeze(-1)).squeeze(-1)
    top = r["y2"].max(-1).values
    assert bool((at >= top - 2 * r["tol_out"]).all()), "arg is not a maximal sample"
    assert bool((a[:, :, 0] != c["tie"].view(B, 1)).all()), "an exact tie went to the higher sample"
    return res


# ---------------------------------------------------------------------------------------------------------------------
# sa2b: the level's backward (128 centres, 64 samples, 512 points; three clouds per launch)
# ---------------------------------------------------------------------------------------------------------------------
# pattern of each cloud of a launch:
#   random   arg uniform over a ball's live samples
#   sample0  every channel of every centre points at sample 0: 128 rows of 256 entries
#   full     all 64 samples of every ball hit: 8192 rows, the scratch's maximum
#   zero     dout == 0: no rows, dr exactly 0, dnx2 untouched
#   one      exactly one live channel: one hit row in the cloud
#   shared   point 0 lies in all 128 balls and every centre has a channel at it: a destination of 128 rows, two tiles
#   rows65 / rows33   hit rows with pairwise distinct destinations, 260 / 132 of them: every part holds exactly 65 / 33 rows
#   repeat   a 512-point cloud made of 100 distinct points (what a 100-point victim feeds the level)
SA2B_LAUNCHES = [("random", "sample0", "full"), ("zero", "one", "shared"), ("rows65", "rows33", "repeat")]


def _live_counts(gidx):
    live = torch.ones(gidx.shape[0], dtype=torch.long)
    for m in range(gidx.shape[0]):
        n = 1
        while n < 64 and int(gidx[m, n]) > int(gidx[m, n - 1]):
            n += 1
        live[m] = n
    return live


def _sa2b_cloud(pattern, g):
    """-> (dout, out, arg [256][128], gidx [128][64]) of one cloud"""
    from oracle import pointnet2_oracle as O
    xyz = torch.rand(512, 3, generator=g)
    radius = 0.4
    if pattern == "full":        # points along a line: every ball holds far more than 64 of them
        xyz = torch.stack([torch.arange(512) / 512.0, torch.zeros(512), torch.zeros(512)], 1)
        radius = 0.3
    elif pattern == "shared":    # a cube of side 0.4: its centre (point 0) is within 0.4 of every point
        xyz = xyz * 0.4
        xyz[0] = 0.2
    elif pattern == "repeat":
        xyz = xyz[torch.arange(512) % 100]
    centres = xyz[torch.arange(128) * 4 + 1].contiguous()
    gidx = O.ball_query(centres.unsqueeze(0), xyz.unsqueeze(0).contiguous(), radius, 64)[0].contiguous()
    live = _live_counts(gidx)
    u = torch.rand(256, 128, generator=g)
    arg = (u * live.view(1, 128)).long().clamp_max(63)
    arg = torch.minimum(arg, live.view(1, 128) - 1)
    dout = torch.randn(256, 128, generator=g)
    out = torch.randn(256, 128, generator=g) + 0.5                     # about a third not positive: those channels are dead
    z = torch.rand(256, 128, generator=g)
    dout[z < 0.1] = 0.0
    dout[(z >= 0.1) & (z < 0.15)] = -0.0
    if pattern == "sample0":
        arg.zero_()
        out, dout = out.abs() + 0.1, torch.where(dout == 0, torch.ones_like(dout), dout)
    elif pattern == "full":
        assert int(live.min()) == 64
        arg = (torch.arange(256) % 64).view(256, 1).expand(256, 128).contiguous()
        out, dout = out.abs() + 0.1, torch.where(dout == 0, torch.ones_like(dout), dout)
    elif pattern == "zero":
        dout.zero_()
    elif pattern == "one":
        keep = float(dout[77, 45]) or 1.0
        dout.zero_()
        dout[77, 45], out[77, 45] = keep, 1.0
    elif pattern == "shared":
        assert bool((gidx[:, 0] == 0).all())
        arg[::7] = 0
        out[::7], dout[::7] = out[::7].abs() + 0.1, torch.where(dout[::7] == 0, torch.ones_like(dout[::7]), dout[::7])
    elif pattern in ("rows65", "rows33"):
        want = 260 if pattern == "rows65" else 132
        used, chosen = set(), [[] for _ in range(128)]
        total = 0
        for s in range(64):                   # sample by sample over the centres: the rows spread over many centres
            for m in range(128):
                j = int(gidx[m, s])
                if total < want and s < int(live[m]) and j not in used:
                    used.add(j)
                    chosen[m].append(s)
                    total += 1
        assert total == want
        for m in range(128):
            if chosen[m]:
                arg[:, m] = torch.tensor(chosen[m])[torch.arange(256) % len(chosen[m])]
                out[:len(chosen[m]), m] = out[:len(chosen[m]), m].abs() + 0.1        # every chosen row keeps a live channel
                dout[:len(chosen[m]), m] = torch.where(dout[:len(chosen[m]), m] == 0, torch.tensor(1.0), dout[:len(chosen[m]), m])
            else:
                dout[:, m] = 0.0
    assert int(gidx.min()) >= 0 and int(gidx.max()) < 512 and int(arg.min()) >= 0 and bool((arg < live.view(1, 128)).all())
    return dout, out, arg.to(torch.int32), gidx


@functools.lru_cache(maxsize=None)
def sa2b_case(launch):
    """-> dict of the launch's three clouds: dout, out [3][256][128], arg int32, gidx int32 [3][128][64], gate0 / gate1 bool
    [3][128][64][128] (random, a tenth of the rows all-closed), W1 [128 k][128 i], W2 [256][128], Wx [128][3], dnx2_in [3][128][3]"""
    pats = SA2B_LAUNCHES[launch]
    g = torch.Generator().manual_seed(4000 + launch)
    clouds = [_sa2b_cloud(p, g) for p in pats]
    dout, out, arg, gidx = (torch.stack([c[i] for c in clouds]).contiguous() for i in range(4))
    gates = []
    for _ in range(2):
        gt = torch.rand(3, 128, 64, 128, generator=g) < 0.6
        gt[torch.rand(3, 128, 64, generator=g) < 0.1] = False
        gates.append(gt)
    W1 = torch.randn(128, 128, generator=g) * (2.0 / 128) ** 0.5
    W2 = torch.randn(256, 128, generator=g) * (2.0 / 128) ** 0.5
    Wx = torch.randn(128, 3, generator=g) * 0.5
    dnx2_in = torch.randn(3, 128, 3, generator=g)
    return dict(patterns=pats, dout=dout, out=out, arg=arg, gidx=gidx, gate0=gates[0], gate1=gates[1], W1=W1, W2=W2, Wx=Wx,
                dnx2_in=dnx2_in)


def sa2b_reference(c, rows=None, **defects):
    """(restatement, tolerances) in float64; rows: a subset of the clouds"""
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    r = R.sa2_bwd(sel(c["dout"]).double(), sel(c["out"]).double(), sel(c["arg"]), sel(c["gidx"]), sel(c["gate0"]),
                  sel(c["gate1"]), c["W1"].double(), c["W2"].double(), c["Wx"].double(), sel(c["dnx2_in"]).double(), **defects)
    return r, R.sa2_bwd_tolerances(r)
