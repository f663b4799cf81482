"""CPU-only: the float64 restatements of the PointNet backward kernels (tests/_pointnet_bwd_ref.py) against torch autograd of
the forward each one differentiates, and two conditions on the cases tests/test_gpu_pointnet_bwd.py runs
(tests/_pointnet_bwd_cases.py): the bound of every case notices a kernel that loses ONE term, and no case asks the kernels
to recompute a relu gate that fp32 rounding could flip."""
import pytest
import torch
import torch.nn.functional as F

from tests import _pointnet_bwd_cases as C
from tests import _pointnet_bwd_ref as R

D = torch.float64


def close(a, b, rel=1e-12):
    return float((a - b).abs().max()) <= rel * float(b.abs().max()) + 1e-300


def wide_forward(X, W, taps):
    """relu -> conv (taps, zero padded) -> max over the points"""
    conv = F.conv1d(X.relu(), W.view(1024, taps, 128).permute(0, 2, 1), padding=taps // 2)
    return conv.max(dim=2)


# ---------------------------------------------------------------------------------------------------------------------
# the restatements against autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taps", [1, 3])
def test_wide_bwd_restatement_is_autograd(taps):
    gen = torch.Generator().manual_seed(taps)
    N = 77
    X = torch.randn(3, 128, N, generator=gen, dtype=D).requires_grad_()
    W = torch.randn(1024, taps * 128, generator=gen, dtype=D)
    g = torch.randn(3, 1024, generator=gen, dtype=D)
    out, arg = wide_forward(X, W, taps)
    (dX,) = torch.autograd.grad((out * g).sum(), X)
    ref, mag = R.wide_bwd(g, arg, W, X.detach() > 0, taps)
    assert close(ref, dX) and bool((mag >= ref.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("taps", [1, 3])
def test_wide_bwd_conv_restatement_is_autograd(taps):
    gen = torch.Generator().manual_seed(10 + taps)
    N = 70
    Y = torch.randn(2, 64, N, generator=gen, dtype=D).requires_grad_()
    W2 = torch.randn(128, 64, generator=gen, dtype=D)
    W = torch.randn(1024, taps * 128, generator=gen, dtype=D)
    g = torch.randn(2, 1024, generator=gen, dtype=D)
    X = torch.einsum("co,bon->bcn", W2, Y.relu())
    out, arg = wide_forward(X, W, taps)
    (dY,) = torch.autograd.grad((out * g).sum(), Y)
    ref, mag = R.wide_bwd_conv(g, arg, W, X.detach() > 0, taps, W2.t().contiguous(), Y.detach() > 0)
    assert close(ref, dY) and bool((mag >= ref.abs() * (1 - 1e-12)).all())


def test_first_layer_form_restatement_is_autograd():
    gen = torch.Generator().manual_seed(5)
    N = 70
    x = torch.randn(2, 3, N, generator=gen, dtype=D).requires_grad_()
    w1, b1 = torch.randn(64, 3, generator=gen, dtype=D), torch.randn(64, generator=gen, dtype=D)
    W2 = torch.randn(128, 64, generator=gen, dtype=D)
    W = torch.randn(1024, 128, generator=gen, dtype=D)
    g = torch.randn(2, 1024, generator=gen, dtype=D)
    held = torch.randn(2, 3, N, generator=gen, dtype=D)
    h = (torch.einsum("kc,bcn->bkn", w1, x) + b1.view(1, -1, 1)).relu()
    X = torch.einsum("co,bon->bcn", W2, h)
    out, arg = wide_forward(X, W, 1)
    (dx,) = torch.autograd.grad((out * g).sum() + (held * x).sum(), x)      # dx3 is ADDED into: the value it held
    ref, _ = R.wide_bwd_conv_first(g, arg, W, X.detach() > 0, W2.t().contiguous(), x.detach(), w1, b1, held)
    assert close(ref, dx)


def test_gram_restatement_is_autograd():
    gen = torch.Generator().manual_seed(6)
    A, G = torch.randn(2, 64, 50, generator=gen, dtype=D), torch.randn(2, 64, 50, generator=gen, dtype=D)
    M = torch.randn(2, 64, 64, generator=gen, dtype=D).requires_grad_()       # out = M A, upstream G: d/dM[o][i] = P[i][o]
    (dM,) = torch.autograd.grad((torch.einsum("boi,bin->bon", M, A) * G).sum(), M)
    assert close(R.gram(A, G)[0], dM.transpose(1, 2))


@pytest.mark.parametrize("with_T", [True, False])
def test_bwd_chain_restatement_is_autograd(with_T):
    gen = torch.Generator().manual_seed(7)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=D)
    Bn, N = 2, 300
    x, T = rn(Bn, 3, N).requires_grad_(), (torch.eye(3, dtype=D) + 0.3 * rn(Bn, 3, 3)).requires_grad_()
    w1, b1, W2, b2, Wa, Wb, Xa, Xb = rn(64, 3), rn(64), rn(64, 64), rn(64), rn(Bn, 64, 64), rn(64, 64), rn(Bn, 64, N), rn(Bn, 64, N)
    p = torch.einsum("bdc,bdn->bcn", T, x) if with_T else x
    h1 = (torch.einsum("kc,bcn->bkn", w1, p) + b1.view(1, -1, 1)).relu()
    h2 = (torch.einsum("ik,bkn->bin", W2, h1) + b2.view(1, -1, 1)).relu()
    loss = (torch.einsum("boi,bin->bon", Wa, h2) * Xa).sum() + (torch.einsum("oi,bin->bon", Wb, h2) * Xb).sum()
    dx, dT = torch.autograd.grad(loss, (x, T), allow_unused=True)
    rdx, _, rdT, _ = R.bwd_chain(Xa, Wa, Xb, Wb, h2.detach() > 0, W2.t().contiguous(), x.detach(),
                                 T.detach() if with_T else None, w1, b1)
    assert close(rdx, dx)
    if with_T:
        assert close(rdT, dT)


def test_fc_restatement_is_torch_linear():
    gen = torch.Generator().manual_seed(8)
    X, W, b, Z = (torch.randn(*s, generator=gen, dtype=D) for s in ((5, 40), (9, 40), (9,), (5, 9)))
    assert close(R.fc(X, W, b, True)[0], F.linear(X, W, b).relu())
    assert close(R.fc(X, W, None, False, Z > 0)[0], torch.where(Z > 0, F.linear(X, W), torch.zeros(5, 9, dtype=D)))
    assert close(R.fc(X, W, skip_k=3)[0], F.linear(X, W) - X[:, 3:4] * W[:, 3].unsqueeze(0))


@pytest.mark.parametrize("taps,N", [(1, 77), (3, 77), (3, 130)])
def test_hit_list_builder_follows_the_documented_order(taps, N):
    """include/geoa3_hip_debug.h: by column; inside a column by (chunk of 64 channels, tap, channel); a tap outside [0, N)
    and a relu-dead channel have no entry -- restated here as four nested loops."""
    gen = torch.Generator().manual_seed(N + taps)
    arg = torch.randint(0, N, (2, 1024), generator=gen)
    arg[1, :700] = N - 1
    arg[1, 700:] = 0
    live = torch.rand(2, 1024, generator=gen) < 0.7
    hits, hoff = R.build_hits(arg, live, N, taps)
    for b in range(2):
        want, offs = [], [0]
        by_col = {}
        for co in range(1024):
            if live[b, co]:
                for tap in range(taps):
                    m = int(arg[b, co]) + tap - taps // 2
                    if 0 <= m < N:
                        by_col.setdefault(m, []).append((co // 64, tap, co))
        for m in range(N):
            want += [(co * taps + tap) | (m << 16) for (_, tap, co) in sorted(by_col.get(m, []))]
            offs.append(len(want))
        assert hoff[b].tolist() == offs
        assert hits[b, :len(want)].tolist() == want and bool((hits[b, len(want):] == -1).all())


def test_gate_bit_packing():
    gen = torch.Generator().manual_seed(3)
    gate = torch.rand(2, 5, 70, generator=gen) < 0.5
    for tail in (False, True):
        w = R.pack_gate_bits(gate, tail)
        assert w.shape == (2, 2, 5)
        for (b, c, n) in [(0, 0, 0), (1, 4, 63), (1, 2, 64), (0, 3, 69)]:
            assert bool((int(w[b, n // 64, c]) >> (n % 64)) & 1) == bool(gate[b, c, n])
        assert all(bool((int(w[0, 1, 0]) >> j) & 1) == tail for j in range(6, 64))


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the GPU cases
# ---------------------------------------------------------------------------------------------------------------------
def moved(base, tol, other):
    return bool(((other - base).abs() > tol).any())


def sparse_defects(c):
    """One instance of each defect that applies to a sparse case, placed where the lost term is largest:
    the last tap of one channel; the first entry of one wave's share of a tile's list; the last column of a tile."""
    taps, N, g, arg = c["taps"], c["N"], c["g"], c["arg"].long()
    out = {}
    co = int(g[0].abs().argmax())
    last = max(t for t in range(taps) if 0 <= int(arg[0, co]) + t - taps // 2 < N)     # (the last tap that has a column)
    out["last tap of a channel"] = dict(skip_entries=[(0, co, last)])
    hits, hoff = R.build_hits(arg, g != 0, N, taps)
    starts = [e for t in range((N + 63) // 64) for e in R.share_starts(hits, hoff, 0, t, N)]
    e = max(starts, key=lambda e: abs(float(g[0, (e & 0xffff) // taps])))
    out["first entry of a wave's share"] = dict(skip_entries=[(0, (e & 0xffff) // taps, (e & 0xffff) % taps)])
    ends = [m for m in sorted({min(64 * t + 63, N - 1) for t in range((N + 63) // 64)}) if hoff[0, m + 1] > hoff[0, m]]
    if ends:      # (a case without a hit in any tile's last column has nothing there to lose)
        out["last column of a tile"] = dict(zero_cols=[(0, m) for m in ends])
    return out


@pytest.mark.parametrize("taps,N", C.SPARSE_SHAPES)
def test_sparse_bounds_notice_one_lost_term(taps, N):
    applied = set()
    for pattern in C.sparse_patterns(taps, N):
        c = C.sparse_case(taps, N, pattern)
        for ref_fn in (C.wide_bwd_reference, C.wide_bwd_conv_reference):
            base, tol = ref_fn(c)
            for name, defect in sparse_defects(c).items():
                assert moved(base, tol, ref_fn(c, **defect)[0]), (ref_fn.__name__, pattern, name)
                applied.add(name)
    assert len(applied) == 3


@pytest.mark.parametrize("N,pattern", C.FIRST_SHAPES)
def test_first_layer_cases_gate_margin_and_lost_term(N, pattern):
    c = C.first_case(N, pattern)
    assert R.gate_margin_ok(c["x3"], c["w1"], c["b1"])
    base, tol = C.first_reference(c)
    for name, defect in sparse_defects(c).items():
        assert moved(base, tol, C.first_reference(c, **defect)[0]), name


def test_stress_sibling_exists():
    taps, N = C.STRESS_SHAPE
    assert (taps, N) in C.SPARSE_SHAPES and "uniform" in C.sparse_patterns(taps, N)
    s = C.sparse_case(taps, N, "uniform", stress=True)["g"].abs()
    assert float(s[s > 0].min()) < 1e-5 and float(s.max()) > 1e5


@pytest.mark.parametrize("N", C.GRAM_N)
def test_gram_bounds_notice_a_lost_column(N):
    assert "uniform" in C.gram_variants(N)          # the sibling of the stress variants
    for variant in C.gram_variants(N):
        c = C.gram_case(N, variant)
        if c["stress"]:
            continue
        base, tol = C.gram_reference(c)
        assert moved(base, tol, C.gram_reference(c, skip_cols=[(0, min(127, N - 1))])[0]), variant


@pytest.mark.parametrize("N", C.CHAIN_N)
def test_chain_cases_gate_margin_and_lost_terms(N):
    c = C.chain_case(N)
    assert R.gate_margin_ok(c["x3"], c["w1"], c["b1"], c["T3"])
    dx, tdx, dT, tdT = C.chain_reference(c)
    for defect in (dict(skip_k=5), dict(zero_cols=[(0, min(255, N - 1))]), dict(omit_dt_block=(0, (N - 1) // 256))):
        ox, _, oT, _ = C.chain_reference(c, **defect)
        if "omit_dt_block" in defect:
            assert moved(dT, tdT, oT), defect
        else:
            assert moved(dx, tdx, ox) and moved(dT, tdT, oT), defect


@pytest.mark.parametrize("Nout,K", C.FC_SHAPES)
def test_fc_bounds_notice_one_lost_k(Nout, K):
    for M in C.FC_M:
        for mode in ("z", "br"):
            c = C.fc_case(M, Nout, K, mode)
            ref, mag = C.fc_reference(c)
            tol = R.tolerance(ref, mag, K + 1)
            assert moved(ref, tol, C.fc_reference(c, skip_k=K - 1)[0]), (M, mode)


# ---------------------------------------------------------------------------------------------------------------------
# the constant c = 4 of the bound: a plain fp32 evaluation on the CPU stays inside it
# ---------------------------------------------------------------------------------------------------------------------
def test_plain_fp32_evaluation_meets_the_bounds():
    worst = {}
    for taps, N in [(1, 77), (3, 200)]:
        for pattern in ("uniform", "col63"):
            c = C.sparse_case(taps, N, pattern)
            for fn in (C.wide_bwd_reference, C.wide_bwd_conv_reference):
                ref, tol = fn(c)
                worst[fn.__name__] = max(worst.get(fn.__name__, 0), R.worst_ratio(fn(c, dtype=torch.float32)[0], ref, tol))
    c = C.first_case(77, "uniform")
    ref, tol = C.first_reference(c)
    worst["first"] = R.worst_ratio(C.first_reference(c, dtype=torch.float32)[0], ref, tol)
    for N in (65, 897):
        c = C.gram_case(N, "uniform")
        ref, tol = C.gram_reference(c)
        worst["gram"] = max(worst.get("gram", 0), R.worst_ratio(C.gram_reference(c, dtype=torch.float32)[0], ref, tol))
    for N in (77, 1000):
        c = C.chain_case(N)
        dx, tdx, dT, tdT = C.chain_reference(c)
        fx, _, fT, _ = C.chain_reference(c, dtype=torch.float32)
        worst["chain dx"] = max(worst.get("chain dx", 0), R.worst_ratio(fx, dx, tdx))
        worst["chain dT"] = max(worst.get("chain dT", 0), R.worst_ratio(fT, dT, tdT))
    print(worst)
    assert all(v < 1 for v in worst.values()), worst
