"""The kernels of csrc/geom_uniform.hip alone against float64: geoa3_uniform_loss through ops.uniform_loss(..., want_idx=True)
with the device's own indices handed to the pair-by-pair restatement (tests/_uniform_ref.py: uniform_ref_parts), and
geoa3_uniform_fold.

Gradient bound, per element, from reference quantities only:
    |err| <= 2^-24 (C1 A_i + C2 |ref_i|) + n_i 2^-33 gscale,   C1 = K + 16, C2 = 1, gscale = 1 / (P B npoint)
n_i fixed-point adds of at most half a unit (2^-33) each; A_i = the sum over the point's pairs of the pair term's magnitude
with |u - e| replaced by u + e.  The float32 roundings of uniform_row behind C1, in units of 2^-24 relative:
    a squared distance (geoa3_sqdist: three differences, three squares, two sums)           5
    sqrt(|d| + 1e-12): the sum 1, the root halves the 6 to 3, its own rounding 1              4   per root
    the sum of the K - 1 roots: K - 2 additions of positive terms                            K - 2
    the division by K - 1                                                                    1   -> u: K + 3
    u - e: its rounding, on top of u's error -- both relative to u + e                       1   -> K + 4
    g = 2 diff / den * cp / km: den, the quotient, cp (float32 of a double), the product, the quotient by km   5
    c = g / sqrt(|d| + 1e-12): the root again 4, the quotient 1                                  5
    c * (p_r - p_n): the difference 1, the product 1                                         2   -> K + 16
C2: the float32 rounding of the finished sum.
Loss bound: 2^-24 (2 K + 12) U.  The row terms (u - e)^2 / den are float32 and non-negative (sum |row terms| / rows is the
loss itself), their sum is double: u - e squared 2 (K + 4), the product 1, den 1, the quotient 1, the float32 result 1.

No case has a near-tie row (uniform_ref_parts reports them; asserted, no row is left out): the seeds are the first of
their sequence for which that holds.

geoa3_uniform_fold: g (+)= w (sum_b c_b / B) dU: the float32 sum of B terms c_b / B and two more roundings:
(B + 3) 2^-24 |w| (sum |c_b| / B) |dU| + 2^-24 |old|; constrain (+)= w U: one product and one sum, 2^-23 (|old| + |w U|).

Largest err / bound on the MI355X (gradient, loss): n20 0.012 0.069; n200 k = 1, 2, 3, 8: 0.349 0.013, 0.046 0.047, 0.051
0.048, 0.048 0.024; n1600 0.088 0.060; n1625 0.060 0.034; n2048 0.057 0.061; p8 0.054 0.078; blob 0.068 0.112; dup 0.048
0.047; n4459 0.494 0.073; n4460 0.161 0.054; n8192 0.054 0.004; geoa3_uniform_fold: g 0.928, constrain 0.697."""
import os

import numpy as np
import pytest
import torch

from geoa3_amd import _lib
from oracle import geoa3_oracle as O
from tests import _uniform_ref as R

pytestmark = pytest.mark.gpu
REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
U24 = 2.0 ** -24
LDS, WORKSPACE = 0, 1
DEFAULT = R.PCTS
EIGHT = (0.004, 0.006, 0.008, 0.010, 0.012, 0.014, 0.016, 0.018)
RATIOS = {}

# name: (B, N, percentages, k, seed, kind)
CASES = {
    "n20": (2, 20, (0.05, 0.1), 2, 0, "plain"),                # npoint = 1: seven wavefronts without a centre
    "n200k1": (2, 200, (0.0125, 0.03), 1, 0, "plain"),        # npoint = 10; ns = 10, 24
    "n200k2": (2, 200, (0.0125, 0.03), 2, 0, "plain"),
    "n200k3": (2, 200, (0.0125, 0.03), 3, 0, "plain"),
    "n200k8": (2, 200, (0.0125, 0.03), 8, 0, "plain"),        # ns = 10 >= k + 1 = 9
    "n1600": (2, 1600, (0.01,), 2, 0, "plain"),               # ns = 64: one full wavefront of rows
    "n1625": (2, 1625, (0.01,), 2, 0, "plain"),               # ns = 65
    "n2048": (2, 2048, (0.0625,), 2, 0, "plain"),             # ns = 512, the limit
    "p8": (2, 1024, EIGHT, 2, 0, "plain"),
    "blob": (2, 1024, DEFAULT, 2, 0, "blob"),                 # balls with more hits than ns: truncated in index order
    "dup": (None, None, None, None, None, "fixture"),         # the fixture's cloud of repeated points
    "n4459": (2, 4459, (0.004,), 2, 0, "plain"),              # the last cloud with the sums in LDS
    "n4460": (2, 4460, (0.004,), 2, 0, "plain"),              # the first with the sums in the workspace
    "n8192": (2, 8192, DEFAULT, 2, 0, "plain"),
}
ROUTES = {"n4459": LDS, "n4460": WORKSPACE, "n8192": WORKSPACE}


def make_case(name):
    """-> (x [B,3,N] float32 on the host, percentages, radius, k)"""
    B, N, pcts, k, seed, kind = CASES[name]
    if kind == "fixture":
        gu = np.load(os.path.join(REPO, "tests", "golden", "geoa3_golden_uniform.npz"), allow_pickle=False)
        pre = "uni/dupzero/"
        return (torch.from_numpy(gu[pre + "x"]), [float(p) for p in gu[pre + "percentages"]], float(gu[pre + "radius"]),
                int(gu[pre + "k"]))
    gen = torch.Generator().manual_seed(1000 * seed + N)
    ori, _ = O.make_synthetic_clouds(B, N, seed=500 + 1000 * seed + N)
    x = ori + 0.01 * torch.randn(ori.shape, generator=gen)
    if kind == "blob":      # half the points within 0.02 of the first one
        v = torch.randn(B, 3, N // 2, generator=gen)
        v = v / v.norm(dim=1, keepdim=True) * (0.02 * torch.rand(B, 1, N // 2, generator=gen) ** (1 / 3))
        x[:, :, 1::2] = x[:, :, :1] + v
    return x.contiguous(), pcts, 1.0, k


def route(B, N, pcts, k, radius=1.0):
    import ctypes
    arr = (ctypes.c_double * len(pcts))(*pcts)
    return _lib.load().geoa3_debug_uniform_route(B, N, arr, len(pcts), radius, k)


def run_case(x, pcts, radius, k):
    """the device's result (outputs pre-filled with NaN) and the restatement on the device's indices"""
    from geoa3_amd import ops
    B, _, N = x.shape
    xc = x.cuda()
    out = (torch.full((), float("nan"), device="cuda"), torch.full((B, 3, N), float("nan"), device="cuda"))
    loss, g, fps, rows = ops.uniform_loss(xc, pcts, radius, k, out=out, want_idx=True)
    ref = R.uniform_ref_parts(xc, pcts, radius, k, idx=(fps.long(), [r.long() for r in rows]))
    return loss, g, fps, rows, ref


def check(name, x, pcts, radius, k, loss, g, ref):
    B, _, N = x.shape
    K, P, npoint = k + 1, len(pcts), int(N * 0.05)
    assert ref["near"].shape[0] == 0, "near-tie rows: %s" % ref["near"][:5].tolist()
    gscale = 1.0 / (P * B * npoint)
    bound = U24 * ((K + 16) * ref["A"] + ref["grad"].abs()) + ref["n"].unsqueeze(1) * 2.0 ** -33 * gscale
    err = (g.double() - ref["grad"]).abs()
    assert not torch.isnan(err).any()
    q = torch.where(err == 0, torch.zeros_like(err), err / bound)
    rg = float(q.max())
    lerr, lb = abs(float(loss) - float(ref["loss"])), U24 * (2 * K + 12) * abs(float(ref["loss"]))
    RATIOS[name] = (rg, lerr / lb)
    print("%-10s grad err/bound %.3f   loss err/bound %.3f   (points without a pair: %d)"
          % (name, rg, lerr / lb, int((ref["n"] == 0).sum())))
    assert float(ref["grad"].abs().max()) > 0 and rg <= 1.0 and lerr <= lb, (name, rg, lerr, lb)


@pytest.mark.parametrize("name", list(CASES))
def test_value_and_gradient_per_element(name):
    x, pcts, radius, k = make_case(name)
    B, _, N = x.shape
    if name in ROUTES:
        assert route(B, N, pcts, k, radius) == ROUTES[name]
    else:
        assert route(B, N, pcts, k, radius) == LDS
    loss, g, fps, rows, ref = run_case(x, pcts, radius, k)
    check(name, x, pcts, radius, k, loss, g, ref)
    if name == "n20":
        assert fps.shape[1] == 1
    if name == "blob":      # a ball that holds the blob has more hits than slots: the first ns in index order
        ns, r2 = int(N * (pcts[0] * 4)), pcts[0] * 4 * radius
        x64 = x.cuda().double()
        centre = torch.gather(x64, 2, fps.long().unsqueeze(1).expand(-1, 3, -1))
        d = ((x64.unsqueeze(2) - centre.unsqueeze(3)) ** 2).sum(1)             # [B,npoint,N]
        inside, shell = d < r2 * (1 - 1e-5), (d - r2).abs() <= r2 * 1e-5
        full = (inside.sum(2) > ns) & ~shell.any(2)                            # (no point the float32 test could see otherwise)
        assert full.any()
        want = torch.sort(torch.where(inside, torch.arange(N, device="cuda").expand_as(inside), N), dim=2)[0][:, :, :ns]
        assert torch.equal(rows[0].long()[full], want[full])


# (n200k1..3 share n200k8's cloud and percentages, so its indices; dup is the fixture case test_gpu_uniform.py already compares)
@pytest.mark.parametrize("name", ["n20", "n200k8", "n1600", "n1625", "n2048", "p8", "blob", "n4459", "n4460", "n8192"])
def test_indices_equal_oracle_and_entry_points(name):
    """the sampler's and the ball queries' indices of the new shapes against the CPU oracle and the stand-alone entry points"""
    from geoa3_amd import ops
    from geoa3_amd.pointnet2 import ext
    x, pcts, radius, k = make_case(name)
    B, _, N = x.shape
    xc = x.cuda()
    _, _, fps, rows = ops.uniform_loss(xc, pcts, radius, k, want_idx=True)
    f2, r2 = R.indices(x, pcts, radius)
    assert torch.equal(fps.cpu().long(), f2)
    pm = xc.permute(0, 2, 1).contiguous()
    assert torch.equal(fps, ext.furthest_point_sampling(pm, int(N * 0.05)).int())
    centres = torch.gather(pm, 1, fps.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    for i, p in enumerate(pcts):
        assert torch.equal(rows[i].cpu().long(), r2[i]), i
        assert torch.equal(rows[i], ext.ball_query(centres, pm, float(np.sqrt(p * 4 * radius)), int(N * (p * 4))).int()), i


def test_nan_instance():
    """B = 3 with a NaN in instance 1: its gradient is NaN, the loss is NaN, and the other instances have the bits of the
    clean run (gscale depends on B only)."""
    from geoa3_amd import ops
    ori, _ = O.make_synthetic_clouds(3, 256, seed=77)
    clean = ops.uniform_loss(ori.cuda())
    for v in (float("nan"), float("inf")):
        x = ori.clone()
        x[1, 2, 17] = v
        loss, g = ops.uniform_loss(x.cuda())
        assert torch.isnan(loss) and torch.isnan(g[1]).all() and torch.isfinite(clean[0])
        assert torch.equal(g[[0, 2]].view(torch.int32), clean[1][[0, 2]].view(torch.int32))


@pytest.mark.parametrize("B,N", [(1, 33), (3, 33), (257, 33), (22, 8192)])
def test_uniform_fold_alone(B, N):
    """B = 257: the sum over scale_const strides by 256; B = 22, N = 8192: the grid-stride loop (2048 blocks)."""
    from geoa3_amd import ops
    gen = torch.Generator().manual_seed(B + N)
    w, PAD = 0.73, 64
    U = torch.tensor(0.831, device="cuda")
    dU, sc = torch.randn(B * 3 * N, generator=gen).cuda(), (torch.rand(B, generator=gen) * 20 - 6).cuda()
    old_c, old_g = torch.randn(B, generator=gen).cuda(), torch.randn(B * 3 * N, generator=gen).cuda()
    wf = float(np.float32(w))
    for add in (False, True):
        for use_c, use_g in ((True, True), (True, False), (False, True)):
            cbuf, gbuf = torch.full((B + 2 * PAD,), 7.5, device="cuda"), torch.full((B * 3 * N + 2 * PAD,), 7.5, device="cuda")
            c, g = cbuf[PAD:PAD + B], gbuf[PAD:PAD + B * 3 * N]
            c.copy_(old_c if add else torch.full_like(old_c, float("nan")))
            g.copy_(old_g if add else torch.full_like(old_g, float("nan")))
            before_c, before_g = cbuf.clone(), gbuf.clone()
            ops.uniform_fold(U, dU if use_g else None, sc if use_g else None, w, B, N, constrain=c if use_c else None,
                             constrain_add=add, g=g if use_g else None, g_add=add)
            assert torch.equal(cbuf[:PAD], before_c[:PAD]) and torch.equal(cbuf[PAD + B:], before_c[PAD + B:])
            assert torch.equal(gbuf[:PAD], before_g[:PAD]) and torch.equal(gbuf[PAD + B * 3 * N:], before_g[PAD + B * 3 * N:])
            oc = old_c.double() if add else torch.zeros(B, dtype=torch.float64, device="cuda")
            og = old_g.double() if add else torch.zeros(B * 3 * N, dtype=torch.float64, device="cuda")
            if use_c:
                ref = oc + wf * U.double()
                err, bound = (c.double() - ref).abs(), 2 * U24 * (oc.abs() + abs(wf) * U.double().abs())
            else:
                assert torch.equal(cbuf.view(torch.int32), before_c.view(torch.int32))
                err, bound = torch.zeros(1), torch.ones(1)
            rc = float((err / bound).max())
            if use_g:
                coef = wf * float(sc.double().sum()) / B
                ref = og + coef * dU.double()
                bound = (B + 3) * U24 * abs(wf) * (float(sc.double().abs().sum()) / B) * dU.double().abs() + U24 * og.abs()
                err = (g.double() - ref).abs()
                assert not torch.isnan(err).any()
                rg = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
            else:
                assert torch.equal(gbuf.view(torch.int32), before_g.view(torch.int32))
                rg = 0.0
            RATIOS["fold B%d N%d add%d c%d g%d" % (B, N, add, use_c, use_g)] = (rg, rc)
            print("uniform_fold B%d N%d add%d c%d g%d   g err/bound %.3f  constrain err/bound %.3f" % (B, N, add, use_c, use_g, rg, rc))
            assert rg <= 1.0 and rc <= 1.0
