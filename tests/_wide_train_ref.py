"""Plain torch restatements (CPU, float64) of the fused train-mode wide layer of geoa3_amd/pointnet_train.py --
conv(128 -> 1024, T taps, zero padding) -> BatchNorm(batch statistics) -> [relu] -> max over points -- its forward and each
piece of its backward, with the rounding bounds the GPU tests hold the kernels to, and the inputs of the cases.  No project
code.  tests/test_wide_train_ref.py pins the restatements to torch autograd of conv1d -> batch_norm(training) -> relu -> max.

Every restatement returns (value, mag) as tests/_pointnet_bwd_ref.py does: mag = the sum of the absolute values of the
products behind an entry.  skip_* / omit_* / shift_* keyword arguments restate a DEFECTIVE layer:
  skip_min        the minimum branch lost (gamma < 0 channels take the maximum),
  omit_k2         the k2 term of dW and dU lost,
  skip_relu_gate  the relu gate of the upstream gradient lost,
  shift_fold      the tap fold of dU -> dX shifted by one point.

Shapes: X [B,128,N], W [1024, T*128] with k = tap*128 + ci, g / out / arg [B,1024].

Bounds (u = 2^-24; `tolerance` of _pointnet_bwd_ref.py with c = 4 and extra = 0: the kernels use the fp32 matrix core, an
exact fmaf chain, no split operands).  First order throughout, in the manner of DESIGN.md 8a:
  y     tol_y  = tolerance(y, |W||U|, K)                                   the MFMA pass, K = T*128 terms
  mu    tol_mu = mean_{b,p} tol_y + tolerance(0, mean|d|, 64)              mean of the errors + the fp32 tile sums of d = y - shift
                                                                            (64 terms; the sums across tiles are double)
  var   tol_v  = mean(2 |d| (tol_y + u |d|)) + 4 sqrt(64) u mean(d^2) + 2 |mean d| tol_mu,   |d| <= |y - mu| + tol_shift
  sigma tol_s  = tol_v / (2 sigma)
  xhat  tol_x  = (max_p tol_y + tol_mu) / sigma + |xhat| tol_s / sigma + 2 u |xhat|
        (max_p tol_y covers a flipped selection: acc[a_k] >= acc[a*] >= y[a*] - tol and acc[a_k] <= y[a_k] + tol <= y[a*] + tol)
  out   tol_o  = |gamma| tol_x + 2 u (|gamma xhat| + |beta|)               relu is 1-Lipschitz
The backward bounds carry these through coef, k1, k2 (wide_train_backward's docstring).
"""
from __future__ import annotations

import math

import torch

from _pointnet_bwd_ref import U24, tolerance

CO, CI = 1024, 128


def unfold(X, taps):
    """U [B, taps*128, N]: U[b, tap*128 + ci, p] = X[b, ci, p + tap - taps//2], zeros past the ends"""
    B, _, N = X.shape
    h = taps // 2
    Xp = torch.zeros(B, CI, N + 2 * h, dtype=X.dtype)
    Xp[:, :, h:h + N] = X
    return torch.cat([Xp[:, :, t:t + N] for t in range(taps)], 1)


def fold(dU, taps, shift_fold=False):
    """dX[b,i,q] = sum_t dU[b, t*128 + i, q - t + taps//2] (terms whose point lies outside [0, N) do not exist)"""
    B, _, N = dU.shape
    h = taps // 2 + (1 if shift_fold else 0)
    dX = torch.zeros(B, CI, N, dtype=dU.dtype)
    for t in range(taps):
        for q in range(N):
            p = q - t + h
            if 0 <= p < N:
                dX[:, :, q] += dU[:, t * CI:(t + 1) * CI, p]
    return dX


def select(y, gamma, skip_min=False):
    """a [B,1024]: first maximum where gamma > 0, first minimum where gamma < 0, point 0 where gamma == 0"""
    first = lambda v, ext: (v == ext.unsqueeze(-1)).to(torch.int64).argmax(-1)      # the lowest index holding the extremum
    amax, amin = first(y, y.max(-1).values), first(y, y.min(-1).values)
    if skip_min:
        amin = amax
    g = gamma.view(1, -1)
    return torch.where(g > 0, amax, torch.where(g < 0, amin, torch.zeros_like(amax)))


def wide_train_forward(X, W, bias, gamma, beta, eps, relu, taps, arg=None, skip_min=False):
    """-> dict: out, arg, xhat, z (before the relu), mean (with the bias), var (biased), y0 = W U, tol_out, tol_xhat, tol_y
    (max over the points), tol_mu, tol_sigma, sigma.  arg: evaluate at these points instead of the extrema."""
    dt = X.dtype
    B, _, N = X.shape
    K, M = taps * CI, B * N
    U = unfold(X, taps)
    y0 = torch.einsum("ck,bkn->bcn", W, U)
    mag = torch.einsum("ck,bkn->bcn", W.abs(), U.abs())
    m0 = y0.mean((0, 2))
    d = y0 - m0.view(1, -1, 1)
    var = (d * d).mean((0, 2))
    sigma = torch.sqrt(var + eps)
    if arg is None:
        arg = select(y0, gamma, skip_min=skip_min)
    ysel = torch.gather(y0, 2, arg.long().unsqueeze(-1)).squeeze(-1)
    xhat = (ysel - m0) / sigma
    z = gamma * xhat + beta
    out = z.clamp_min(0) if relu else z
    # bounds
    tol_y = tolerance(y0, mag, K)
    mU = U.mean((0, 2))
    tol_shift = tolerance(W @ mU, W.abs() @ mU.abs(), K)
    da = d.abs() + tol_shift.view(1, -1, 1)
    tol_mu = tol_y.mean((0, 2)) + tolerance(torch.zeros_like(m0), da.mean((0, 2)), 64)
    tol_v = (2 * da * (tol_y + U24 * da)).mean((0, 2)) + 4 * 8 * U24 * (da * da).mean((0, 2)) + 2 * tol_shift * tol_mu
    tol_s = tol_v / (2 * sigma)
    ty = tol_y.max(-1).values
    tol_x = (ty + tol_mu) / sigma + xhat.abs() * tol_s / sigma + 2 * U24 * xhat.abs()
    tol_o = gamma.abs() * tol_x + 2 * U24 * ((gamma * xhat).abs() + beta.abs())
    return dict(out=out, arg=arg, xhat=xhat, z=z, mean=m0 + bias, var=var, y0=y0, sigma=sigma, tol_out=tol_o, tol_xhat=tol_x,
                tol_y=ty, tol_y_full=tol_y, tol_mu=tol_mu, tol_sigma=tol_s, tol_var=tol_v)


def wide_train_backward(X, W, bias, gamma, beta, eps, relu, taps, g, arg, omit_k2=False, skip_relu_gate=False,
                        shift_fold=False):
    """The closed form of the layer's backward at the points `arg`:
      g~ = g [z_sel > 0] (relu) or g;  dbeta = sum_b g~;  dgamma = sum_b g~ xhat_sel;  coef = g~ gamma / sigma;
      k1 = gamma dbeta / (sigma M);  k2 = gamma dgamma / (sigma^2 M);  m = mean(W U)
      dW = sum_b coef U[b,:,a] - k1 S1 - k2 (W G - m S1);   dU = scatter(coef W) - (W^T diag(k2) W) U - W^T (k1 - k2 m)
      dX = fold(dU);  dbias = 0.
    -> dict name -> (value, tol).  Bounds: each sum by `tolerance` with n = its longest sum (B for dbeta / dgamma; B + M + K
    for dW: the gather, the M-term sums S1 / G, the K-term product; 1024 T + K + 1024 for dX), plus, to first order, what the
    forward's errors carry in:  rel = tol_sigma / sigma + 4u (coef),  dk1 = |gamma| / (sigma M) (tol_dbeta + |dbeta| tol_sigma / sigma),
    dk2 = |gamma| / (sigma^2 M) (tol_dgamma + 2 |dgamma| tol_sigma / sigma),  dm = tol_mu:
      dgamma += sum_b |g~| tol_xhat
      dW     += rel sum_b |coef U| + dk1 |S1| + dk2 |W G - m S1| + |k2| dm |S1|
      dX     += fold(scatter(rel |coef W|) + |W|^T (dk2 |W U|) + |W|^T (dk1 + dk2 |m| + |k2| dm))"""
    dt = X.dtype
    B, _, N = X.shape
    K, M = taps * CI, B * N
    f = wide_train_forward(X, W, bias, gamma, beta, eps, relu, taps, arg=arg)
    U, sigma, xhat = unfold(X, taps), f["sigma"], f["xhat"]
    m = f["mean"] - bias
    gt = g * (f["z"] > 0).to(dt) if (relu and not skip_relu_gate) else g
    dbeta, mag_db = gt.sum(0), gt.abs().sum(0)
    dgamma, mag_dg = (gt * xhat).sum(0), (gt * xhat).abs().sum(0)
    tol_db = tolerance(dbeta, mag_db, B)
    tol_dg = tolerance(dgamma, mag_dg, B) + (gt.abs() * f["tol_xhat"]).sum(0)
    coef = gt * (gamma / sigma)
    k1 = gamma * dbeta / (sigma * M)
    k2 = gamma * dgamma / (sigma * sigma * M)
    if omit_k2:
        k2 = torch.zeros_like(k2)
    rs = f["tol_sigma"] / sigma
    rel = rs + 4 * U24
    dk1 = gamma.abs() / (sigma * M) * (tol_db + dbeta.abs() * rs)
    dk2 = gamma.abs() / (sigma * sigma * M) * (tol_dg + 2 * dgamma.abs() * rs)
    dm = f["tol_mu"]
    # dW
    Usel = torch.gather(U, 2, arg.long().view(B, 1, CO).expand(B, K, CO))            # [B,K,CO]: U[b,:,a_bc]
    gath = torch.einsum("bc,bkc->ck", coef, Usel)
    mag_g = torch.einsum("bc,bkc->ck", coef.abs(), Usel.abs())
    Uf = U.permute(1, 0, 2).reshape(K, M)
    S1, S1a = Uf.sum(1), Uf.abs().sum(1)
    G, Ga = Uf @ Uf.t(), Uf.abs() @ Uf.abs().t()
    inner = W @ G - m.view(-1, 1) * S1.view(1, -1)
    inner_a = W.abs() @ Ga + m.abs().view(-1, 1) * S1a.view(1, -1)
    dW = gath - k1.view(-1, 1) * S1 - k2.view(-1, 1) * inner
    mag_W = mag_g + k1.abs().view(-1, 1) * S1a + k2.abs().view(-1, 1) * inner_a
    tol_W = (tolerance(dW, mag_W, B + M + K) + rel.view(-1, 1) * mag_g + dk1.view(-1, 1) * S1.abs()
             + dk2.view(-1, 1) * inner.abs() + (k2.abs() * dm).view(-1, 1) * S1.abs())
    # dU -> dX
    sc = torch.zeros(B, K, N, dtype=dt)
    sc_a = torch.zeros(B, K, N, dtype=dt)
    sc_r = torch.zeros(B, K, N, dtype=dt)
    for b in range(B):
        term = (W * coef[b].view(-1, 1)).t()                                          # [K, CO]
        sc[b].index_add_(1, arg[b].long(), term)
        sc_a[b].index_add_(1, arg[b].long(), term.abs())
        sc_r[b].index_add_(1, arg[b].long(), term.abs() * rel.view(1, -1))
    P = W.t() @ (k2.view(-1, 1) * W)
    Pa = W.abs().t() @ (k2.abs().view(-1, 1) * W.abs())
    v = W.t() @ (k1 - k2 * m)
    va = W.abs().t() @ (k1.abs() + (k2 * m).abs())
    dU = sc - torch.einsum("kj,bjn->bkn", P, U) - v.view(1, -1, 1)
    mag_U = sc_a + torch.einsum("kj,bjn->bkn", Pa, U.abs()) + va.view(1, -1, 1)
    car_U = (sc_r + torch.einsum("ck,bcn->bkn", W.abs(), dk2.view(1, -1, 1) * f["y0"].abs())
             + (W.abs().t() @ (dk1 + dk2 * m.abs() + k2.abs() * dm)).view(1, -1, 1))
    dX, mag_X, car_X = fold(dU, taps, shift_fold=shift_fold), fold(mag_U, taps), fold(car_U, taps)
    tol_X = tolerance(dX, mag_X, CO * taps + K + CO) + car_X
    return dict(dbeta=(dbeta, tol_db), dgamma=(dgamma, tol_dg), dW=(dW, tol_W), dX=(dX, tol_X),
                dbias=(torch.zeros(CO, dtype=dt), torch.zeros(CO, dtype=dt)), gate_margin=(f["z"], f["tol_out"]))


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_wide_train.py
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 64), (3, 33), (2, 200))      # one full tile; ragged, both padded ends of T = 3 in one tile; four tiles, the last ragged
CASES = [(B, N, T, relu) for (B, N) in SHAPES for T in (1, 3) for relu in (True, False)]
OFFSET_CH = 5                               # the input channel that carries a constant offset of 32 standard deviations
NEG_GAMMA = slice(0, 256)                   # channels with gamma < 0
ZERO_GAMMA = 300
DEAD = slice(400, 464)                      # channels the relu kills (beta very negative)


def make_case(B, N, taps, relu, seed=0):
    """float64 inputs of one case (the float32 values the kernel gets, exactly): X with one offset channel and exact
    duplicate points (point N-1 = point 0's neighbourhood copy, point 7 = point 3 in every instance, T = 1; for T = 3 whole
    runs are repeated so that the unfolded columns coincide), gamma with negative and one zero entry, beta with dead channels."""
    gen = torch.Generator().manual_seed(1000 * seed + 100 * B + 10 * N + taps + (5 if relu else 0))
    r = lambda *s: torch.randn(*s, generator=gen)
    X = r(B, CI, N)
    X[:, OFFSET_CH] += 32.0
    # exact duplicates: points 20..24 repeat points 10..14 (the unfolded columns of 11..13 and 21..23 coincide for T = 3,
    # every column of the run for T = 1): the lower index must win
    X[:, :, 20:25] = X[:, :, 10:15]
    W = r(CO, taps * CI) * (1.0 / math.sqrt(taps * CI))
    bias = r(CO) * 0.1
    gamma = 0.5 + torch.rand(CO, generator=gen)
    gamma[NEG_GAMMA] *= -1
    gamma[ZERO_GAMMA] = 0.0
    beta = r(CO) * 0.5 + 1.0
    beta[DEAD] = -50.0
    g = r(B, CO)
    f32 = lambda t: t.float().double()
    return dict(X=f32(X), W=f32(W), bias=f32(bias), gamma=f32(gamma), beta=f32(beta), g=f32(g), eps=float(torch.tensor(1e-3, dtype=torch.float32)), relu=relu, taps=taps,
                B=B, N=N)
