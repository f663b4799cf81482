"""The sparse arg-max backward kernels (csrc/pointnet_wide_bwdconv.hip) ALONE at the list lengths where their load
pipelines change phase.  A wave walks its share of a tile's hit list (an eighth of it, rounded up) holding 64 entries at a time
and keeps D = 16 weight rows in flight (two batches of eight), so one tile is given exactly h hits for h in

    0; 1, 7 (waves without a share); 8; 8 D - 1, 8 D, 8 D + 1; 8 * 64 - 1, 8 * 64, 8 * 64 + 1 (a share longer than one load of
    entries); every channel on one column (1024 hits, three taps 3072: every share starts inside a column)

-- one h per instance, three instances a case -- on N in {64, 65, 130, 1024}, for one tap, three taps and the first-layer
form; and column runs that lie across two, three and four consecutive shares; target tiles include the ragged last one.

Asserted for every case: the fused kernel with the forward's lists (PRE) == without them == wide_max_bwd2_kernel + the split
128 -> 64 convolution, bit for bit; the float64 bound of tests/test_gpu_pointnet_bwd.py; row 1 of the batch == the batch-1 run of
instance 1.  The file pins behaviour, not an implementation: it holds for any walk that adds a column's terms in list order."""
import functools

import pytest
import torch

from tests import _pointnet_bwd_cases as C
from tests import _pointnet_bwd_ref as R

pytestmark = pytest.mark.gpu

D = 16                      # list entries a wave keeps in flight (pointnet_wide_bwdconv.hip: U * NB)
ALL = "all"                 # every channel's arg-max on one column
GROUPS = {"none-1-7": (0, 1, 7), "0-7-8": (0, 7, 8), "8-D": (8, 8 * D - 1, 8 * D), "D-64": (8 * D + 1, 8 * 64 - 1, 8 * 64),
          "64-all": (8 * 64 + 1, ALL, 8)}


def lib_stream():
    from geoa3_amd import _lib
    return _lib, _lib.load(), torch.cuda.current_stream().cuda_stream


def P(t):
    return None if t is None else t.data_ptr()


def check_bound(got, ref, tol, what):
    ratio = R.worst_ratio(got.cpu(), ref, tol)
    print("worst err/tol %-50s %.4f" % (what, ratio))
    assert ratio <= 1.0, "%s: worst err / tol = %g" % (what, ratio)


# ---------------------------------------------------------------------------------------------------------------------
# cases: arg-max tables with an exact number of hits in one tile
# ---------------------------------------------------------------------------------------------------------------------
def tile_hits(c, b, tile):
    """hits of instance b that fall into the tile, counted from the tables themselves"""
    m0, N, taps = 64 * tile, c["N"], c["taps"]
    n = 0
    for tap in range(taps):
        m = c["arg"][b].long() + tap - taps // 2
        n += int(((m >= m0) & (m < min(m0 + 64, N)) & (c["g"][b] != 0)).sum())
    return n


def exact_case(taps, N, tile, specs):
    """C.sparse_case(taps, N, "uniform") with g and arg rewritten: instance b gets exactly specs[b]["h"] hits in `tile`
    (ALL: every channel on one of its columns); specs[b]["runs"] = [(column of the tile, channels), ...] are placed first, the
    rest on random columns of the tile.  The channels left over go to columns whose taps all miss the tile (their g keeps its
    zeros and signs), or get g = 0 where there is no such column."""
    c = C.sparse_case(taps, N, "uniform")
    gen = torch.Generator().manual_seed(77000 + 1000 * taps + 13 * N + tile)
    m0 = 64 * tile
    ncol = min(64, N - m0)
    assert ncol >= 1 and len(specs) == C.B
    g, arg = c["g"].clone(), c["arg"].clone()
    gnz = torch.where(g == 0, torch.ones_like(g), g)
    far = [m for m in range(N) if all(not (m0 <= m + t - taps // 2 < m0 + ncol) for t in range(taps))]
    inside = lambda m: sum(1 for t in range(taps) if m0 <= m + t - taps // 2 < m0 + ncol and 0 <= m + t - taps // 2 < N)
    by_hits = {k: [m for m in range(max(0, m0 - 1), min(N, m0 + ncol + 1)) if inside(m) == k] for k in (1, 2, 3)}
    rnd = lambda pool, n: [pool[i] for i in torch.randint(0, len(pool), (n,), generator=gen).tolist()] if n else []
    for b, spec in enumerate(specs):
        chans = torch.randperm(1024, generator=gen).tolist()
        put = []                                     # arg-max columns of the channels that hit the tile
        if spec["h"] == ALL:
            put = [(by_hits[taps] or by_hits[1])[len(by_hits[taps] or by_hits[1]) // 2]] * 1024
        else:
            left = spec["h"]
            for col, nch in spec.get("runs", ()):
                assert inside(m0 + col) == taps
                put += [m0 + col] * nch
                left -= taps * nch
            assert left >= 0
            if taps == 1:
                runcols = {m0 + col for col, _ in spec.get("runs", ())}
                put += rnd([m for m in by_hits[1] if m not in runcols], left)
            else:
                # left = 3 a + 2 b + c from the positions this tile has (a ragged tile of two columns has no 3-hit position)
                for cnt1 in ((0, 1) if by_hits[1] else (0,)):
                    sol = [(a3, b2) for b2 in range(0, (left - cnt1) // 2 + 1) for a3 in [(left - cnt1 - 2 * b2) // 3]
                           if 3 * a3 + 2 * b2 + cnt1 == left and (a3 == 0 or by_hits[3]) and (b2 == 0 or by_hits[2])]
                    if sol:
                        a3, b2 = sol[0] if by_hits[3] else sol[-1]
                        put += rnd(by_hits[3], a3) + rnd(by_hits[2], b2) + rnd(by_hits[1], cnt1)
                        break
                else:
                    raise AssertionError("no arg-max table gives %d hits in tile %d of N = %d" % (spec["h"], tile, N))
        assert len(put) <= 1024
        hit_ch, rest = chans[:len(put)], chans[len(put):]
        g[b, hit_ch] = gnz[b, hit_ch]
        arg[b, hit_ch] = torch.tensor(put, dtype=arg.dtype)
        if rest:
            if far:
                arg[b, rest] = torch.tensor(rnd(far, len(rest)), dtype=arg.dtype)
            else:
                g[b, rest] = 0.0
    c["g"], c["arg"] = g, arg
    for b, spec in enumerate(specs):
        want = (1024 * inside(int(arg[b, 0]))) if spec["h"] == ALL else spec["h"]
        assert tile_hits(c, b, tile) == want, (b, spec, tile_hits(c, b, tile))
    return c


@functools.lru_cache(maxsize=None)
def first_layer(N):
    """the cloud, the 3 -> 64 layer and the prefilled dx3 of the first-layer form: the first seed whose pre-activations all keep
    the margin of R.gate_margin_ok (the kernel recomputes the gate in fp32)"""
    for seed in range(64):
        gen = torch.Generator().manual_seed(61000 + 131 * N + seed)
        x3, w1 = torch.randn(C.B, 3, N, generator=gen), torch.randn(64, 3, generator=gen)
        b1, dx3 = torch.randn(64, generator=gen) * 0.5, torch.randn(C.B, 3, N, generator=gen)
        if R.gate_margin_ok(x3.double(), w1.double(), b1.double()):
            return dict(x3=x3, w1=w1, b1=b1, dx3_in=dx3)
    raise AssertionError("no seed keeps the first layer's gates away from zero at N = %d" % N)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------------------------------------------------
class Driver:
    """a case on the device; rows: the instances taken"""

    def __init__(self, c, rows=None):
        from geoa3_amd.pointnet import pack_wide_split
        sel = (lambda t: t) if rows is None else (lambda t: t[rows].contiguous())
        self.taps, self.N = c["taps"], c["N"]
        self.g, self.arg = sel(c["g"]).cuda(), sel(c["arg"]).cuda()
        self.B = self.g.shape[0]
        self.W, self.W2t = c["W"].cuda(), c["W2t"].cuda()
        w2th, self.uns = pack_wide_split(c["W2t"])
        self.W2th = w2th.cuda()
        self.gate128, self.gate64 = sel(c["gate128"]), sel(c["gate64"])
        self.m128 = R.pack_gate_bits(self.gate128, tail_ones=True).cuda()
        self.m64 = R.pack_gate_bits(self.gate64, tail_ones=True).cuda()
        hits, hoff = R.build_hits(sel(c["arg"]), sel(c["g"]) != 0, self.N, self.taps)
        self.hits, self.hoff = hits.cuda(), hoff.cuda()
        if "x3" in c:
            self.x3, self.w1, self.b1 = sel(c["x3"]).cuda(), c["w1"].cuda(), c["b1"].cuda()
            self.dx3_in = sel(c["dx3_in"]).cuda()

    def wide_bwd(self):
        _lib, lib, s = lib_stream()
        Z = torch.where(self.gate128, 1.0, -1.0).cuda()
        dX = torch.full((self.B, 128, self.N), float("nan"), device="cuda")
        _lib.check(lib.geoa3_debug_wide_bwd(P(self.g), P(self.arg), P(self.W), P(Z), P(dX), self.B, self.N, self.taps, s),
                   "geoa3_debug_wide_bwd")
        return dX

    def fused(self, pre, first=False):
        _lib, lib, s = lib_stream()
        if first:
            out = self.dx3_in.clone()
            extra = (None, None, P(self.x3), P(self.w1), P(self.b1), P(out))
        else:
            out = torch.full((self.B, 64, self.N), float("nan"), device="cuda")
            extra = (P(self.m64), P(out), None, None, None, None)
        _lib.check(lib.geoa3_debug_wide_bwd_conv(P(self.g), P(self.arg), P(self.W), P(self.m128), P(self.W2t), P(self.W2th),
                                                 self.uns, *extra, P(self.hits) if pre else None,
                                                 P(self.hoff) if pre else None, self.B, self.N, self.taps, s),
                   "geoa3_debug_wide_bwd_conv")
        return out

    def two_kernels(self, dX):
        _lib, lib, s = lib_stream()
        Z = torch.where(self.gate64, 1.0, -1.0).cuda()
        Y = torch.full((self.B, 64, self.N), float("nan"), device="cuda")
        _lib.check(lib.geoa3_debug_conv_cm(P(dX), P(self.W2t), None, P(Z), P(Y), self.B, self.N, 128, 64, 0, 1, s),
                   "geoa3_debug_conv_cm")
        return Y


def check_case(c, tag, first):
    dev, one = Driver(c), Driver(c, rows=[1])
    ref, tol = C.wide_bwd_conv_reference(c)
    plain, pre = dev.fused(False), dev.fused(True)
    check_bound(plain, ref, tol, "wide_bwd_conv " + tag)
    assert torch.equal(plain, pre), tag
    assert torch.equal(plain, dev.two_kernels(dev.wide_bwd())), tag
    assert torch.equal(one.fused(True)[0], plain[1]) and torch.equal(one.fused(False)[0], plain[1]), tag
    if first:
        ref, tol = C.first_reference(c)
        plain, pre = dev.fused(False, first=True), dev.fused(True, first=True)
        check_bound(plain, ref, tol, "first-layer form " + tag)
        assert torch.equal(plain, pre), tag
        assert torch.equal(one.fused(True, first=True)[0], plain[1]), tag
        assert torch.equal(one.fused(False, first=True)[0], plain[1]), tag


# (N, target tile, group): every group on two N, every N with two groups; tiles: the only one, the first of two, the ragged last
# one (N = 65: one column; N = 130: two columns), an inner one and the last of sixteen
ONE_TAP = [(64, 0, "none-1-7"), (130, 2, "none-1-7"), (65, 0, "8-D"), (1024, 15, "8-D"), (64, 0, "D-64"), (1024, 3, "D-64"),
           (65, 1, "64-all"), (130, 1, "64-all")]
# three taps: a tile's count is 3 a + 2 b + c (c: an arg-max one column outside the tile) -- N = 64 has no such column, so
# h = 1 is taken on the other sizes; the ragged tile of N = 130 has two columns (2 b + c)
THREE_TAPS = [(64, 0, "0-7-8"), (130, 1, "none-1-7"), (65, 0, "8-D"), (1024, 15, "8-D"), (130, 2, "D-64"), (1024, 7, "D-64"),
              (64, 0, "64-all"), (1024, 8, "64-all")]


@pytest.mark.parametrize("N,tile,group", ONE_TAP)
def test_one_tap_and_first_layer_form_at_the_pipeline_boundaries(N, tile, group):
    c = exact_case(1, N, tile, [dict(h=h) for h in GROUPS[group]])
    c.update(first_layer(N))
    check_case(c, "taps 1 N %d tile %d h %s" % (N, tile, GROUPS[group]), first=True)


@pytest.mark.parametrize("N,tile,group", THREE_TAPS)
def test_three_taps_at_the_pipeline_boundaries(N, tile, group):
    c = exact_case(3, N, tile, [dict(h=h) for h in GROUPS[group]])
    check_case(c, "taps 3 N %d tile %d h %s" % (N, tile, GROUPS[group]), first=False)


@pytest.mark.parametrize("taps,N,tile", [(1, 130, 1), (3, 1024, 5), (1, 65, 0)])
def test_column_runs_across_two_three_and_four_shares(taps, N, tile):
    """h = 128: shares of 16.  Columns are listed in order, so (one tap) runs of 10, 11, 9, 20 entries on columns 0 .. 3 put the
    second across shares 0-1 and the fourth across shares 1-3 when nothing else lands on them; instance 1: one run of 60 from
    the list's start (shares 0-3); instance 2: 513 hits with a run of 140 on one column (shares of 65: 64 entries and one more,
    the run across three of them).  Three taps: a run on column c is a run on c - 1, c and c + 1."""
    if taps == 1:
        specs = [dict(h=128, runs=[(0, 10), (1, 11), (2, 9), (3, 20)]), dict(h=128, runs=[(0, 60)]), dict(h=513, runs=[(5, 140)])]
    else:
        specs = [dict(h=128, runs=[(1, 36)]), dict(h=128, runs=[(1, 12), (5, 20)]), dict(h=513, runs=[(9, 50)])]
    c = exact_case(taps, N, tile, specs)
    if taps == 1:
        c.update(first_layer(N))
    check_case(c, "runs taps %d N %d tile %d" % (taps, N, tile), first=taps == 1)
