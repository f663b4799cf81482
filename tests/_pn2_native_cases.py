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


# ---------------------------------------------------------------------------------------------------------------------
# sa1 backward: sa1_bwd_kernel + sa1_scatter_kernel (64 samples; any B, M, N)
# ---------------------------------------------------------------------------------------------------------------------
# (B, M, N): 3 centroids = fewer than the 8 wavefronts of a workgroup; 3 x 40 on 300 points = the real ball query at radius
# 0.25 with a duplicated point; 5 x 512 = 2560 centroids, just over the 2048 the grid's 256 workgroups of 8 wavefronts take in
# one pass: 512 wavefronts take a second centroid through the prefetch.
SA1B_SHAPES = [(1, 3, 40), (3, 40, 300), (5, 512, 128)]
# variants of a shape (the same seed: a variant is the random case with the named change)
#   padding      centroid 0 a ball of ONE real point (63 repeats), centroid 1 a FULL ball, centroid 2 a ball whose repeats
#                begin at sample 32 (the column-block boundary)
#   padding_arg  padding, with arg naming a REPEAT of sample 0 for some channels whose maximum sits at sample 0
#   zeros        centroid 1 with every out <= 0, centroid 2 with g == 0
#   band         b1 and b2 nudged so that one z1 and one z2 of a row that carries gradient sit inside their bands
#   g_channel    one channel's g 2^12 times the rest;     g_centroid   one centroid's g 2^20 times its workgroup neighbours
#   w1_small / w1_big   max|W1| = 2^-6 / 2^6 max|b1|;     coincide     a ball whose points all coincide with the centroid
SA1B_STRESS = ["g_channel", "g_centroid", "w1_small", "w1_big", "coincide"]
# the ball query's radius: 0.25, but 0.6 for the 2560 centroids -- mostly full balls, where half the rows are nobody's arg-max
# and carry neither gradient nor allowance (at 0.25 every row of a ball of ~8 points does, and ~1.5e-3 of them have one of
# their 128 gates in its band: over the cap however the case is seeded)
SA1B_RADIUS = {(5, 512, 128): 0.6}
SA1B_BAND = (2, 40, 300, "band")      # (about 1200 non-padded rows: the cap admits the ONE row the case puts into its bands)
SA1B_SHARE = 1e-3          # at most this part of a case's non-padded dp rows may carry an allowance (the share 8b uses for m1)


def _sa1_fwd64(c, b, layers=None):
    L = layers if layers is not None else c["layers"]
    return R.sa1_fwd(c["xyz"][b], c["nx"][b], c["gidx"][b], [(w.double(), v.double()) for w, v in L])


@functools.lru_cache(maxsize=None)
def sa1b_case(B, M, N, variant="random"):
    """-> dict B, M, N, xyz [B][N][3], nx [B][M][3], gidx [B][M][64] int32, layers = ((W1, b1), (W2, b2), (W3, b3)) float32, out
    [B][M][128] float32 and arg [B][M][128] uint8 from the FLOAT64 forward restatement (the backward is tested apart from the
    forward kernel), g [B][M][128]; band: the nudged (layer, cloud, m, s, channel) gates of the variant of that name."""
    from oracle import pointnet2_oracle as O
    g = torch.Generator().manual_seed(6000 + B + M + N)
    xyz = torch.rand(B, N, 3, generator=g) - 0.5
    xyz[:, 7] = xyz[:, 3]                                          # a duplicated point
    nx = xyz[:, (torch.arange(M) * 7) % N].clone()
    if M > N:                                                      # more centroids than points: given directly, no sampler
        nx[:, N:] += 0.02 * torch.randn(B, M - N, 3, generator=g)
    gidx = O.ball_query(nx.contiguous(), xyz, SA1B_RADIUS.get((B, M, N), 0.25), 64).clone()
    layers = [[torch.randn(co, ci, generator=g) * (2.0 / ci) ** 0.5, torch.randn(co, generator=g) * 0.1]
              for ci, co in ((3, 64), (64, 64), (64, 128))]
    grad = torch.randn(B, M, 128, generator=g)
    if variant in ("padding", "padding_arg"):
        assert M >= 3 and N >= 64
        gidx[0, 0, :] = gidx[0, 0, 0]
        gidx[0, 1, :] = torch.arange(64, dtype=torch.int32)
        gidx[0, 2, :32] = torch.arange(8, 40, dtype=torch.int32)
        gidx[0, 2, 32:] = 8
    elif variant == "g_channel":
        grad[:, :, 5] *= 2.0 ** 12
    elif variant == "g_centroid":
        grad[:, 1] *= 2.0 ** 20
    elif variant in ("w1_small", "w1_big"):
        want = 2.0 ** (-6 if variant == "w1_small" else 6)
        layers[0][0] *= want * float(layers[0][1].abs().max()) / float(layers[0][0].abs().max())
    elif variant == "coincide":
        gidx[:, 0, :] = 11
        nx[:, 0] = xyz[:, 11]
    c = dict(B=B, M=M, N=N, xyz=xyz.contiguous(), nx=nx.contiguous(), gidx=gidx.contiguous(), g=grad, band=[])
    if variant == "band":
        # a row that carries gradient: the arg-max sample of channel 0 at centroid 1 of cloud 0.  First b1 (z2 depends on it),
        # then b2: the nudged z is what float32 rounding of the bias leaves, far inside tol(z).
        f = _sa1_fwd64(c, 0, layers)
        m, s = 1, int(f["arg"][1, 0])
        layers[0][1][9] -= float(f["z1"][m, s, 9])
        f = _sa1_fwd64(c, 0, layers)
        s = int(f["arg"][1, 0])
        layers[1][1][21] -= float(f["z2"][m, s, 21])
        f = _sa1_fwd64(c, 0, layers)
        s2 = int(f["arg"][1, 0])
        c["band"] = [(1, 0, m, s, 9), (2, 0, m, s, 21)] if s2 == s else []
    c["layers"] = tuple((w.contiguous(), v.contiguous()) for w, v in layers)
    fw = [_sa1_fwd64(c, b) for b in range(B)]
    c["out"] = torch.stack([f["out"].float() for f in fw]).contiguous()
    arg = torch.stack([f["arg"] for f in fw])
    if variant in ("padding", "padding_arg"):
        # (the backward routes a channel's gradient to whatever sample arg names: every fourth channel of centroid 2 is SENT to
        # sample 0, so that the ball with real points and repeats has channels there)
        arg[0, 2, 0::4] = 0
    if variant == "padding_arg":
        assert int(arg[0, 0].max()) == 0
        arg[0, 0, 0::3], arg[0, 0, 1::3] = 63, 33
        at0 = arg[0, 2] == 0
        arg[0, 2][at0] = 40
        c["renamed"] = int(at0.sum())
    elif variant == "zeros":
        c["out"][0, 1, 0::2], c["out"][0, 1, 1::2] = 0.0, -1.0
        grad[0, 2] = 0.0
    c["arg"] = arg.to(torch.uint8).contiguous()
    return c


@functools.lru_cache(maxsize=None)
def sa1b_reference(B, M, N, variant="random"):
    """the float64 restatement of every cloud of the case: a list of R.sa1_bwd results"""
    c = sa1b_case(B, M, N, variant)
    L64 = [(w.double(), v.double()) for w, v in c["layers"]]
    return [R.sa1_bwd(c["xyz"][b], c["nx"][b], c["gidx"][b], L64, c["out"][b], c["arg"][b], c["g"][b]) for b in range(B)]


def sa1b_checks(refs, dp, dnew, dxyz, what, allowance=True):
    """dp [B][M][64][3], dnew [B][M][3], dxyz [B][N][3] (CPU) held to bound + allowance, cloud by cloud; padded rows of dp
    exactly zero; dp None (the float-atomic form writes none): the other two.  -> {name: worst err / tol}.  Raises
    AssertionError."""
    worst = {"dnew": 0.0, "dxyz": 0.0} if dp is None else {"dp": 0.0, "dnew": 0.0, "dxyz": 0.0}
    for b, r in enumerate(refs):
        assert dp is None or not bool(dp[b][r["pad"]].any()), "%s: a padded row of dp is not zero" % what
        for name, got in (("dp", dp), ("dnew", dnew), ("dxyz", dxyz)):
            if got is None:
                continue
            got = got[b]
            ref, _, tol, allow = r[name]
            worst[name] = max(worst[name], R.worst_ratio(got, ref, tol + allow if allowance else tol))
    print("worst err/tol %-44s " % what + " ".join("%s %.4f" % kv for kv in worst.items()))
    assert max(worst.values()) <= 1.0, (what, worst)
    return worst


def sa1b_share(refs):
    """the part of a case's non-padded dp rows that carries an allowance"""
    return sum(r["share"][0] for r in refs) / max(1, sum(r["share"][1] for r in refs))


def sa1b_emulate(c, **kw):
    """the CPU emulation of the kernels' arithmetic on every cloud of a case -> dp [B][M][64][3], dnew, dxyz"""
    outs = [R.sa1_bwd_split(c["xyz"][b], c["nx"][b], c["gidx"][b], c["layers"], c["out"][b], c["arg"][b], c["g"][b],
                            flip=[f[:1] + f[2:] for f in kw.get("flip", ()) if f[1] == b],
                            **{k: v for k, v in kw.items() if k != "flip"}) for b in range(c["B"])]
    return tuple(torch.stack([o[i] for o in outs]) for i in range(3))
