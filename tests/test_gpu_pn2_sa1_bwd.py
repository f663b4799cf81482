"""Level 1's backward of the PointNet++ SSG native path ALONE -- sa1_bwd_kernel and sa1_scatter_kernel (csrc/pointnet2_sa.hip)
through geoa3_pn2_sa1_backward, which leaves dp [B][M][64][3] readable in its scratch, and geoa3_debug_pn2_sa1_scatter --
against the float64 restatement R.sa1_bwd and the integer model R.sa1_scatter_fixed (tests/_pn2_native_ref.py), at the cases
of tests/_pn2_native_cases.py.  out and arg come from the float64 forward restatement, idx and new_xyz are given directly:
the backward is tested apart from the forward kernel and from the sampler.

Bound.  The bound of tests/test_gpu_pn2_kernels.py per product -- 4 sqrt(n) 2^-24 mag + 2^-22 |ref|, + 2^-21 mag for a product of
split-fp16 operands -- composed as there: dh2 = W3^T dz3 (n = 128, split), dh1 = W2^T dz2 (n = 64, split) + tol(dh2) through
|W2^T|, dp = W1^T dz1 (n = 64, float32 operands) + tol(dh1) through |W1^T|; dnew + its 64-term sum; sample 0 + the merge's sum;
dxyz the sum of its entries' tolerances + the scatter's own bound (fixed point: cnt 2^(Ex - 41) + 2^-24 |ref|; float atomics: a
plain float32 sum of cnt terms).

Scale floor.  The operand of the first backward product, dz3, is scaled by 2^kg from its MEASURED maximum, kg = 140 - E(max |g|
of the centroid's live channels).  The operand of the second, dz2, is scaled from BOUNDS: the accumulators hold 2^(k3 + kg) dh2
(W3 at 2^k3), |dh2| < 2^(EW3T + 14 - kg) with 2^EW3T above the largest column l1 norm of W3, and kd = -k3 - EW3T takes them below
2^14 whatever the data: the operand is dz2 2^(kg - EW3T), possibly far below 2^14.  A scaled value v is carried as hi = fp16(v),
lo = fp16(v - hi).  fp16's normal numbers end at 2^-14 and its subnormals step by 2^-24: once lo (or hi itself) is subnormal it
is rounded to a multiple of 2^-24, so v - hi - lo is up to 2^-25 ABSOLUTE instead of 2^-23 |v|.  Unscaled, an element of dz2
carries up to fd = 2^(-25 - kg + EW3T), an element of dz3 up to fg = 2^(-25 - kg).  fg enters tol(dh2) through |W3^T| (the
one-hot entries), fd enters tol(dh1) through |W2^T| (the gates that are open or in band) and from there tol(dp) through |W1^T|.
Both use kg WITHOUT the kernel's clamp: the reference and its bound are scale-free, a clamp that costs precision shows.

Margin scheme.  The kernel's gates are the signs of its own recomputed z1 and z2 (bias included).  A gate with |z| <= tol(z)
(t1, t2 of R.sa1_fwd) may differ from the float64 sign.  To first order an in-band z2 gate j toggles |dh2[j]| in dz2, which
reaches dp through |W2[j, :]|, the z1 gates that are open or in band themselves (the cross term) and |W1|; an in-band z1 gate i
toggles |dh1[i]|, which reaches dp through |W1[i, :]|.  That is the ALLOWANCE of the row's dp, carried into dnew and dxyz like
a tolerance; everywhere else the plain bound holds.  At most 1e-3 of a case's non-padded rows carry one, asserted on the CPU
from the reference alone (tests/test_pn2_native_ref.py), where the bounds are also shown to notice one lost term and the
kernel's own defects, and to hold an emulation of its arithmetic.  Every test prints its worst err / tol."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _pn2_native_cases as C
from tests import _pn2_native_ref as R

pytestmark = pytest.mark.gpu


def P(t):
    return None if t is None else t.data_ptr()


def sa1_backward(c, scratch=True, rows=None):
    """geoa3_pn2_sa1_backward on a case (rows: a subset of its clouds) -> (dp or None, dnew, dxyz) on the CPU.  dp is the
    scratch, pre-filled with NaN: the float-atomic form leaves it untouched."""
    from geoa3_amd import _lib
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    d = {k: sel(c[k]).cuda().contiguous() for k in ("xyz", "nx", "gidx", "out", "arg", "g")}
    B, M, N = d["xyz"].shape[0], c["M"], c["N"]
    assert d["gidx"].dtype == torch.int32 and d["arg"].dtype == torch.uint8
    assert int(d["gidx"].min()) >= 0 and int(d["gidx"].max()) < N and int(d["arg"].max()) < 64
    wt = [t.cuda().contiguous() for pair in c["layers"] for t in pair]
    w = _lib.Sa1Weights(*[t.data_ptr() for t in wt])
    assert int(lib.geoa3_pn2_sa1_scratch_bytes(B, M)) == B * M * 64 * 3 * 4
    dp = torch.full((B, M, 64, 3), float("nan"), device="cuda") if scratch else None
    dxyz = torch.full((B, N, 3), float("nan"), device="cuda")
    dnew = torch.full((B, M, 3), float("nan"), device="cuda")
    _lib.check(lib.geoa3_pn2_sa1_backward(P(d["xyz"]), P(d["nx"]), P(d["gidx"]), ctypes.byref(w), B, N, M, P(d["out"]), P(d["arg"]),
                                          P(d["g"]), P(dxyz), P(dnew), P(dp), s), "geoa3_pn2_sa1_backward")
    torch.cuda.synchronize()
    return (None if dp is None else dp.cpu()), dnew.cpu(), dxyz.cpu()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def model_of(c, dp, rows=None):
    """the integer model of the scatter applied to the GPU's own dp"""
    gidx = c["gidx"] if rows is None else c["gidx"][rows]
    return torch.from_numpy(np.stack([R.sa1_scatter_fixed(dp[b].numpy(), gidx[b].numpy(), c["N"]) for b in range(dp.shape[0])]))


def scaled(refs, f):
    """the references of a case whose gradient is f times as large (f a power of two: exact in float64)"""
    return [dict(r, **{k: tuple(t * f for t in r[k]) for k in ("dp", "dnew", "dxyz")}) for r in refs]


@pytest.mark.parametrize("B,M,N", C.SA1B_SHAPES)
def test_sa1_bwd_shapes_against_float64(B, M, N):
    """fewer centroids than a workgroup's wavefronts; the real ball query with a duplicated point; 2560 centroids, where 512
    wavefronts take a second centroid through the prefetch.  dp, dnew, dxyz under bound + allowance; dxyz == the integer
    model of the GPU's own dp; the same bits on a second launch and in a batch-1 run of one instance."""
    c, refs = C.sa1b_case(B, M, N), C.sa1b_reference(B, M, N)
    dp, dnew, dxyz = sa1_backward(c)
    C.sa1b_checks(refs, dp, dnew, dxyz, "sa1_bwd B %d M %d N %d" % (B, M, N))
    assert same_bits(dxyz, model_of(c, dp))
    again = sa1_backward(c)
    assert all(same_bits(x, y) for x, y in zip((dp, dnew, dxyz), again))
    b = B - 1
    one = sa1_backward(c, rows=[b])
    assert same_bits(one[0][0], dp[b]) and same_bits(one[1][0], dnew[b]) and same_bits(one[2][0], dxyz[b])


def test_sa1_bwd_padding():
    """a ball of one real point (63 repeats), a full ball, a ball whose repeats begin at sample 32; padded rows of dp exactly
    zero (sa1b_checks); with arg naming a REPEAT of sample 0 for some channels, the results stay within the bound of the run
    where it names sample 0"""
    sh = (1, 8, 80)
    c, refs = C.sa1b_case(*sh, "padding"), C.sa1b_reference(*sh, "padding")
    live = C._live_counts(c["gidx"][0])
    assert [int(live[m]) for m in range(3)] == [1, 64, 32]
    got = sa1_backward(c)
    C.sa1b_checks(refs, *got, "sa1_bwd padding")
    assert same_bits(got[2], model_of(c, got[0]))
    ca = C.sa1b_case(*sh, "padding_arg")
    assert ca["renamed"] > 0 and bool((ca["arg"][0, 0] != 0).any())
    gota = sa1_backward(ca)
    C.sa1b_checks(refs, *gota, "sa1_bwd padding, arg at a repeat")
    C.sa1b_checks(C.sa1b_reference(*sh, "padding_arg"), *gota, "sa1_bwd padding, arg at a repeat (own reference)")
    assert same_bits(gota[2], model_of(ca, gota[0]))
    _, dnew, dxyz = sa1_backward(ca, scratch=False)          # the float-atomic form merges the duplicates in its own lines
    C.sa1b_checks(refs, None, dnew, dxyz, "sa1_bwd padding, arg at a repeat, atomics")
    assert same_bits(dnew, gota[1])


def test_sa1_bwd_dead_and_zero_centroids():
    """a centroid with every out <= 0 and a centroid with g == 0: their dp and dnew are exactly zero, and every other centroid
    has the bits of the run without them"""
    sh = (1, 8, 80)
    c = C.sa1b_case(*sh, "zeros")
    assert bool((c["out"][0, 1] <= 0).all()) and not bool(c["g"][0, 2].any())
    dp, dnew, dxyz = sa1_backward(c)
    C.sa1b_checks(C.sa1b_reference(*sh, "zeros"), dp, dnew, dxyz, "sa1_bwd zeros")
    for m in (1, 2):
        assert not dp[0, m].any() and not dnew[0, m].any()
    base = sa1_backward(C.sa1b_case(*sh))
    others = [m for m in range(8) if m not in (1, 2)]
    assert same_bits(dp[0, others], base[0][0, others]) and same_bits(dnew[0, others], base[1][0, others])
    assert same_bits(dxyz, model_of(c, dp))


def test_sa1_bwd_in_band_gates():
    """one z1 and one z2 of a row that carries gradient inside their bands (b1 / b2 nudged): bound + allowance holds whichever
    way the kernel's gates fall (the CPU emulation shows that the plain bound cannot: test_pn2_native_ref.py)"""
    c, refs = C.sa1b_case(*C.SA1B_BAND), C.sa1b_reference(*C.SA1B_BAND)
    assert len(c["band"]) == 2 and C.sa1b_share(refs) <= C.SA1B_SHARE
    C.sa1b_checks(refs, *sa1_backward(c), "sa1_bwd band")


@pytest.mark.parametrize("variant", C.SA1B_STRESS)
def test_sa1_bwd_magnitude_stress(variant):
    """one channel's g 2^12 times the rest of its centroid; one centroid's g 2^20 times its workgroup neighbours (the scales
    are per centroid: every entry keeps its OWN bound); max|W1| = 2^-6 and 2^6 max|b1|; a ball whose points all coincide with
    the centroid"""
    sh = (1, 8, 80)
    c, refs = C.sa1b_case(*sh, variant), C.sa1b_reference(*sh, variant)
    got = sa1_backward(c)
    C.sa1b_checks(refs, *got, "sa1_bwd " + variant)
    assert same_bits(got[2], model_of(c, got[0]))


def test_sa1_bwd_power_of_two_equivariance():
    """every scale in the file is a power of two: grad_out times 2^-s gives dp, dnew and dxyz times 2^-s EXACTLY (s = 3, 10: every
    centroid's maximum stays far above 2^-17), and so does (xyz, new_xyz) times 2^t with W1 times 2^-t (t = 2, 3, -2)"""
    c = C.sa1b_case(3, 40, 300)
    base = sa1_backward(c)
    assert all(bool(torch.isfinite(t).all()) for t in base)
    for s in (3, 10):
        got = sa1_backward(dict(c, g=c["g"] * 2.0 ** -s))
        assert all(same_bits(a * 2.0 ** -s, b) for a, b in zip(base, got)), s
    (W1, b1), l2, l3 = c["layers"]
    for t in (2, 3, -2):
        got = sa1_backward(dict(c, xyz=c["xyz"] * 2.0 ** t, nx=c["nx"] * 2.0 ** t, layers=((W1 * 2.0 ** -t, b1), l2, l3)))
        assert all(same_bits(a * 2.0 ** -t, b) for a, b in zip(base, got)), t


def clamp_sweep(c, refs, steps):
    """-> [(s, worst err / tol of dp, of dnew, every entry finite)] of the case with grad_out times 2^-s"""
    rows = []
    for s in steps:
        dp, dnew, dxyz = sa1_backward(dict(c, g=c["g"] * 2.0 ** -s))
        r = scaled(refs, 2.0 ** -s)[0]
        rd = R.worst_ratio(dp[0], r["dp"][0], r["dp"][2] + r["dp"][3])
        rn = R.worst_ratio(dnew[0], r["dnew"][0], r["dnew"][2] + r["dnew"][3])
        rows.append((s, rd, rn, bool(torch.isfinite(dp).all() and torch.isfinite(dnew).all())))
        assert same_bits(dxyz, model_of(c, dp)), s
    return rows


def test_sa1_bwd_small_gradients():
    """grad_out times 2^-s, s = 20, 24, ...: below a centroid maximum of 2^-17 and down to where the kernel's own unscale factor
    leaves float32's normal numbers.  The factor is f1 = 2^-(k2 + kd + k3 + kg) = 2^-(k2 - EW3T + kg), with W2 at 2^k2, kd = -k3 -
    EW3T and kg = 140 - E, E the exponent field of the centroid's largest live |g|.  f1 is a normal number while k2 - EW3T + 140 -
    E <= 126, and 2^kg is one while kg <= 127: E >= Emin = max(13, 14 + k2 - EW3T), i.e. a centroid maximum of 2^(Emin - 127) or
    more (2^-104 with these weights).  Down to there the float64 reference, which is scale-free, must be met at the bound of s = 0
    times 2^-s; dxyz equals the integer model of the kernel's own dp at every step (the scatter's exponent is clamped at -80 by
    design: below 2^-80 its step is absolute, so dxyz is not held to the scale-free bound here).  Below Emin the kernel says so:
    every entry of a centroid that carries gradient is NaN -- never a finite value that is silently wrong.
    (With the scale's exponent field clamped at 110, as it was: err / tol of dp 0.2 at s = 32, 2.6 at 36, 22 at 40, and from s = 52
    on every result an exact, silent zero: NOTEBOOK 14.)"""
    sh = (1, 8, 80)
    c, refs = C.sa1b_case(*sh), C.sa1b_reference(*sh)
    (_, _), (W2, _), (W3, _) = c["layers"]
    k2, EW3T = R.sa_k(float(W2.abs().max())), R.l1_exponent(float(W3.abs().sum(0).max()))
    Emin = max(13, 14 + k2 - EW3T)
    g0 = torch.where(c["out"][0] > 0, c["g"][0], torch.zeros(()))
    Es = [R.biased_exponent(float(v)) for v in g0.abs().max(1).values]
    steps = [s for s in range(20, 256, 4) if min(Es) - s >= Emin]
    assert len(steps) > 15 and max(Es) - steps[0] < 110
    rows = clamp_sweep(c, refs, steps)
    for s, rd, rn, fin in rows:
        print("small gradients: 2^-%-3d  dp err/tol %-10.4g dnew err/tol %-10.4g finite %d" % (s, rd, rn, fin))
    assert all(rd <= 1.0 and rn <= 1.0 and fin for _, rd, rn, fin in rows), rows
    below = max(Es) - Emin + 4                           # every centroid's maximum below 2^(Emin - 127)
    dp, dnew, dxyz = sa1_backward(dict(c, g=c["g"] * 2.0 ** -below))
    carries = refs[0]["dp"][1].sum(-1) > 0                # rows with gradient behind them
    assert bool(torch.isnan(dp[0][carries]).all()) and bool(torch.isnan(dnew[0]).all())
    assert not dp[0][refs[0]["pad"]].any()
    hit = torch.zeros(c["N"], dtype=torch.bool)
    hit[c["gidx"][0].long()[carries]] = True
    assert bool(torch.isnan(dxyz[0][hit]).all())


def scatter_fits(N):
    """the launcher's own LDS formula: 3 N 64-bit sums, 16 floats, a bit per point, in 160 KiB less 512 bytes"""
    return 3 * N * 8 + 16 * 4 + (N + 31) // 32 * 4 <= 160 * 1024 - 512


def test_sa1_bwd_atomic_path_without_scratch():
    """scratch = NULL: float atomics.  dxyz and dnew under the bound; dnew has the deterministic run's bits"""
    sh = (3, 40, 300)
    c, refs = C.sa1b_case(*sh), C.sa1b_reference(*sh)
    det = sa1_backward(c)
    none, dnew, dxyz = sa1_backward(c, scratch=False)
    assert none is None
    C.sa1b_checks(refs, None, dnew, dxyz, "sa1_bwd atomics, no scratch")
    assert same_bits(dnew, det[1])


def test_sa1_bwd_atomic_path_beyond_lds():
    """M 8 at the largest N whose sums fit LDS (deterministic: dxyz == the integer model) and at N + 1 (scratch given but left
    untouched: float atomics, dxyz under the bound, dnew under it too)"""
    Nmax = max(n for n in range(6000, 7000) if scatter_fits(n))
    assert scatter_fits(Nmax) and not scatter_fits(Nmax + 1)
    for N in (Nmax, Nmax + 1):
        sh = (1, 8, N)
        c, refs = C.sa1b_case(*sh), C.sa1b_reference(*sh)
        dp, dnew, dxyz = sa1_backward(c)
        if N == Nmax:
            C.sa1b_checks(refs, dp, dnew, dxyz, "sa1_bwd N %d (fits)" % N)
            assert same_bits(dxyz, model_of(c, dp))
        else:
            assert bool(torch.isnan(dp).all()), "the scratch was written: not the atomic path"
            C.sa1b_checks(refs, None, dnew, dxyz, "sa1_bwd N %d (atomics)" % N)


def scatter(dp, gidx, N):
    from geoa3_amd import _lib
    lib, s = _lib.load(), torch.cuda.current_stream().cuda_stream
    B, M = gidx.shape[:2]
    d, i = dp.cuda().contiguous(), gidx.cuda().contiguous()
    out = torch.full((B, N, 3), 7.0, device="cuda")
    _lib.check(lib.geoa3_debug_pn2_sa1_scatter(P(d), P(i), B, N, M, P(out), s), "geoa3_debug_pn2_sa1_scatter")
    torch.cuda.synchronize()
    return out.cpu()


def test_sa1_scatter_alone():
    """sa1_scatter_kernel on chosen dp, N = 77 (not a multiple of 32): instance 0 with a hub every ball references and a
    destination that only receives contributions 2^-30 of the instance's maximum (exact against the model; within cnt 2^(Ex - 41)
    + 2^-24 |sum| of float64: an ABSOLUTE step, not the destination's own magnitude); instance 1 all zero; instance 2 random.
    One NaN: its destination alone is NaN.  One infinity: its instance alone is NaN."""
    from geoa3_amd import _lib
    g = torch.Generator().manual_seed(8)
    B, M, N = 3, 8, 77
    gidx = torch.stack([torch.stack([torch.randperm(N - 2, generator=g)[:64] + 2 for _ in range(M)]) for _ in range(B)]).to(torch.int32)
    gidx[0, :, 0] = 0                                     # the hub: sample 0 of every ball
    gidx[0, :, 5] = 1                                     # point 1: referenced by sample 5 of every ball, nowhere else
    gidx[2, 3, 40:] = gidx[2, 3, 0]                       # a padded ball
    dp = torch.randn(B, M, 64, 3, generator=g)
    dp[0, :, 5] *= 2.0 ** -30
    dp[1] = 0.0
    dp[2, 3, 40:] = 0.0
    lib, keep = _lib.load(), torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")       # (a real buffer behind every pointer)
    assert lib.geoa3_debug_pn2_sa1_scatter(None, P(keep), B, N, M, P(keep), None) == -1
    assert lib.geoa3_debug_pn2_sa1_scatter(P(keep), P(keep), B, 0, M, P(keep), None) == -1
    assert lib.geoa3_debug_pn2_sa1_scatter(P(keep), P(keep), 1, 7000, M, P(keep), None) == -3     # beyond LDS: not supported

    def check(dp, what):
        got = scatter(dp, gidx, N)
        want = torch.from_numpy(np.stack([R.sa1_scatter_fixed(dp[b].numpy(), gidx[b].numpy(), N) for b in range(B)]))
        assert same_bits(got, want), what
        return got
    got = check(dp, "finite")
    assert not got[1].any()
    for b in (0, 2):
        ref, bound, Ex = R.sa1_scatter_bound(dp[b].numpy(), gidx[b].numpy(), N)
        ratio = R.worst_ratio(got[b], ref, bound)
        print("worst err/bound scatter alone, instance %d: %.4f (Ex %d; destination 1: |sum| %.3g, bound %.3g)"
              % (b, ratio, Ex, float(ref[1].abs().max()), float(bound[1].max())))
        assert ratio <= 1.0
    nan = dp.clone()
    nan[0, 2, 9, 1] = float("nan")
    got = check(nan, "nan")
    bad = torch.zeros(N, dtype=torch.bool)
    bad[int(gidx[0, 2, 9])] = True
    assert bool(torch.isnan(got[0][bad]).all()) and bool(torch.isfinite(got[0][~bad]).all()) and bool(torch.isfinite(got[1:]).all())
    inf = dp.clone()
    inf[0, 2, 9, 1] = float("inf")
    got = check(inf, "inf")
    assert bool(torch.isnan(got[0]).all()) and bool(torch.isfinite(got[1:]).all())
