"""Plain torch restatements (CPU, float64) of the train-mode EdgeConv layer of geoa3_amd/dgcnn_train.py -- the neighbour half:
z = U0[idx] + V0 -> BatchNorm(batch statistics over the M = B N K edges) -> LeakyReLU(0.2) -> max over the K neighbours -- its
forward and each piece of its backward, with the rounding bounds the GPU tests hold the kernels to, and the inputs of the
cases.  No project code.  tests/test_edge_train_ref.py pins the restatements to torch autograd of the materialised composition.

Every restatement returns (value, mag) or a dict name -> (value, tol) as tests/_wide_train_ref.py does.  skip_* / omit_*
keyword arguments restate a DEFECTIVE layer:
  skip_min          the minimum branch lost (gamma < 0 channels take the maximum),
  omit_dgamma_term  the (dgamma / M) r (...) term of dV0 and dU0 lost,
  omit_list_v       the sum of V0[i] over the destination list lost from dU0.

Shapes: U0, V0, S1, dU0, dV0 [B,N,C]; arg [B,N,C] (slot); idx [B,N,K]; y, g [B,C,N]; gamma, beta, mean, var [C].

Bounds.  u = 2^-24; tol(ref, mag, n) = 4 sqrt(n) u mag + 2^-22 |ref| is `tolerance` of _pointnet_bwd_ref.py with n = the
number of float32 roundings in the sum behind the entry and mag = the sum of the absolute values of its terms.  The kernels
round to float32 in four places only: the sequential sums S1 (K terms), A and Bv (the destination list of j: indeg(j) terms),
g' = fl(0.2f g) where y <= 0, and ONCE when an output is stored.  Everything else is double: the statistics are double
sums of the EXACT values u + v, and each output is formed in double from float32 inputs and those sums.  The store is the
2^-22 |ref| of tol with n = 0.  A double sum of M terms is off by at most M 2^-53 times the sum of the absolute values;
`dbl` = 4 M 2^-53 covers the sums, the divisions and the square root.  So, to first order:
  mean   tol(mean, ., 0) + dbl mean|z|
  var    tol(var, ., 0) + dbl mean z^2       (var = mean z^2 - mean^2 in double: the cancellation is paid in double)
  r      only double: rel_r = dbl mean z^2 / (2 (var + eps));  mu_err = dbl mean|z|
  zhat   only double: tol_zhat = r mu_err + |zhat| rel_r
  y      tol(y, ., 0) + dbl (|gamma zhat| + |beta|) + |gamma| tol_zhat        (LeakyReLU is 1-Lipschitz)
  S1     tol(S1, sum_s |u|, K)
  g'     y > 0: exact; else fl(0.2f g): the rounding and the constant 0.2f, tol_gp = 2 u |g'|
  dbeta  tol(dbeta, ., 0) + dbl sum|g'| + Tdb,   Tdb = sum tol_gp
  dgamma tol(dgamma, ., 0) + dbl sum|g' zhat| + Tdg,   Tdg = sum tol_gp |zhat| + sum |g'| tol_zhat
  dV0    tol(dV0, ., 0) + dbl mag + |gamma r| (tol_gp + K Tdb / M + Tdg / M r |inner| + |dgamma| / M r tol_S1),
         mag = |gamma r| (|g'| + K |dbeta| / M + |dgamma| / M r (|S1| + K |V0| + K |mean|)): what g', dbeta, dgamma (used
         unrounded) and S1 carry in
  dU0    tol(dU0, ., 0) + dbl mag + |gamma r| (tol_A + indeg Tdb / M + Tdg / M r |inner| + |dgamma| / M r tol_Bv) with the two
         sequential float32 sums over the destination list of j, whose bounds GROW WITH THE IN-DEGREE:
         tol_A = tol(A, sum |g'|, indeg) + sum tol_gp over the selected entries, tol_Bv = tol(Bv, sum |V0|, indeg).
         A destination nobody lists has every term zero: its dU0 is exactly zero.
"""
from __future__ import annotations

import torch

from _pointnet_bwd_ref import U24, tolerance

SLOPE = 0.2


def tolerance_n(ref, mag, n):
    """`tolerance` with a per-entry number of roundings n (a tensor)"""
    return 4.0 * torch.sqrt(n.to(mag.dtype)) * U24 * mag + 2.0 ** -22 * ref.abs()


def gather_rows(X, idx):
    """X [B,N,C], idx [B,N,K] -> X[b, idx[b,i,s], :] [B,N,K,C]"""
    B, N, C = X.shape
    K = idx.shape[2]
    return torch.gather(X, 1, idx.reshape(B, N * K, 1).expand(B, N * K, C)).view(B, N, K, C)


def select(Ug, gamma, skip_min=False):
    """arg [B,N,C] from Ug [B,N,K,C]: the first maximum over the slots where gamma > 0, the first minimum where gamma < 0,
    slot 0 where gamma == 0"""
    first = lambda ext: (Ug == ext.unsqueeze(2)).to(torch.int64).argmax(2)      # the lowest slot holding the extremum
    amax, amin = first(Ug.max(2).values), first(Ug.min(2).values)
    if skip_min:
        amin = amax
    g = gamma.view(1, 1, -1)
    return torch.where(g > 0, amax, torch.where(g < 0, amin, torch.zeros_like(amax)))


def edge_train_forward(U0, V0, idx, gamma, beta, eps, arg=None, skip_min=False):
    """-> dict: y [B,C,N], a (the pre-activation gamma zhat + beta, [B,N,C]), arg, S1, mean, var, r, zhat, usel and the
    bounds tol_y [B,C,N], tol_mean, tol_var, tol_S1, tol_zhat.  arg: evaluate at these slots instead of the extrema."""
    B, N, C = U0.shape
    K = idx.shape[2]
    M = B * N * K
    Ug = gather_rows(U0, idx)
    z = Ug + V0.unsqueeze(2)
    mean = z.mean((0, 1, 2))
    var = ((z - mean) ** 2).mean((0, 1, 2))
    r = 1.0 / torch.sqrt(var + eps)
    if arg is None:
        arg = select(Ug, gamma, skip_min=skip_min)
    usel = torch.gather(Ug, 2, arg.long().unsqueeze(2)).squeeze(2)
    zhat = (usel + V0 - mean) * r
    a = gamma * zhat + beta
    y = torch.where(a > 0, a, SLOPE * a)
    S1 = Ug.sum(2)
    # bounds
    dbl = 4.0 * M * 2.0 ** -53
    mabs, msq = z.abs().mean((0, 1, 2)), (z * z).mean((0, 1, 2))
    tol_mean = tolerance(mean, mabs, 0) + dbl * mabs
    tol_var = tolerance(var, msq, 0) + dbl * msq
    rel_r = dbl * msq / (2 * (var + eps))
    tol_zhat = r * dbl * mabs + zhat.abs() * rel_r
    mag_y = (gamma * zhat).abs() + beta.abs()
    tol_y = tolerance(y, mag_y, 0) + dbl * mag_y + gamma.abs() * tol_zhat
    tol_S1 = tolerance(S1, Ug.abs().sum(2), K)
    return dict(y=y.transpose(1, 2).contiguous(), a=a, arg=arg, S1=S1, mean=mean, var=var, r=r, zhat=zhat, usel=usel,
                tol_y=tol_y.transpose(1, 2).contiguous(), tol_a=tol_y, tol_mean=tol_mean, tol_var=tol_var, tol_S1=tol_S1,
                tol_zhat=tol_zhat)


def edge_train_backward(U0, V0, idx, gamma, beta, eps, g, arg, omit_dgamma_term=False, omit_list_v=False):
    """The closed form of the layer's backward at the slots `arg` (the module docstring's bounds):
      g' = a > 0 ? g : 0.2 g;  dbeta = sum_{b,i} g';  dgamma = sum_{b,i} g' zhat_sel
      dV0[i] = gamma r (g' - K dbeta / M - (dgamma / M) r (S1[i] + K V0[i] - K mean))
      dU0[j] = gamma r (sum_{(i,s)->j, s == arg[i]} g'[i] - indeg(j) dbeta / M
                        - (dgamma / M) r (indeg(j) (U0[j] - mean) + sum_{(i,s)->j} V0[i]))
    -> dict name -> (value, tol)."""
    B, N, C = U0.shape
    K = idx.shape[2]
    M = B * N * K
    f = edge_train_forward(U0, V0, idx, gamma, beta, eps, arg=arg)
    mean, r, zhat, S1 = f["mean"], f["r"], f["zhat"], f["S1"]
    gt = g.transpose(1, 2)                                                        # [B,N,C]
    pos = f["a"] > 0
    gp = torch.where(pos, gt, SLOPE * gt)
    tol_gp = torch.where(pos, torch.zeros_like(gp), 2 * U24 * gp.abs())
    dbeta, mag_db = gp.sum((0, 1)), gp.abs().sum((0, 1))
    dgamma, mag_dg = (gp * zhat).sum((0, 1)), (gp * zhat).abs().sum((0, 1))
    Tdb = tol_gp.sum((0, 1))
    Tdg = (tol_gp * zhat.abs()).sum((0, 1)) + (gp.abs() * f["tol_zhat"]).sum((0, 1))
    dbl = 4.0 * M * 2.0 ** -53
    tol_db = tolerance(dbeta, mag_db, 0) + dbl * mag_db + Tdb
    tol_dg = tolerance(dgamma, mag_dg, 0) + dbl * mag_dg + Tdg
    k2 = torch.zeros_like(dgamma) if omit_dgamma_term else dgamma / M * r
    gr = gamma * r
    # dV0
    inner = S1 + K * V0 - K * mean
    inner_a = S1.abs() + K * V0.abs() + K * mean.abs()
    dV = gr * (gp - K * dbeta / M - k2 * inner)
    mag_V = gr.abs() * (gp.abs() + K * dbeta.abs() / M + k2.abs() * inner_a)
    tol_V = tolerance(dV, mag_V, 0) + dbl * mag_V + gr.abs() * (tol_gp + K * Tdb / M + Tdg / M * r * inner.abs() + k2.abs() * f["tol_S1"])
    # dU0: the sums over the destination lists
    onehot = torch.zeros(B, N, K, C, dtype=U0.dtype).scatter_(2, arg.long().unsqueeze(2), 1.0)   # [s == arg[i]]
    flat = idx.reshape(B, N * K)
    scat = lambda t: torch.zeros(B, N, C, dtype=U0.dtype).index_put_(
        (torch.arange(B).view(B, 1).expand(B, N * K), flat), t.reshape(B, N * K, C), accumulate=True)
    A = scat(onehot * gp.unsqueeze(2))
    A_a = scat(onehot * gp.abs().unsqueeze(2))
    A_t = scat(onehot * tol_gp.unsqueeze(2))
    Vexp = V0.unsqueeze(2).expand(B, N, K, C)
    Bv, Bv_a = scat(Vexp), scat(Vexp.abs())
    deg = scat(torch.ones(B, N, K, C, dtype=U0.dtype))
    if omit_list_v:
        Bv = torch.zeros_like(Bv)
    innerU = deg * (U0 - mean) + Bv
    innerU_a = deg * (U0.abs() + mean.abs()) + Bv_a
    dU = gr * (A - deg * dbeta / M - k2 * innerU)
    mag_U = gr.abs() * (A_a + deg * dbeta.abs() / M + k2.abs() * innerU_a)
    tol_A = tolerance_n(A, A_a, deg) + A_t
    tol_B = tolerance_n(Bv, Bv_a, deg)
    tol_U = tolerance(dU, mag_U, 0) + dbl * mag_U + gr.abs() * (tol_A + deg * Tdb / M + Tdg / M * r * innerU.abs() + k2.abs() * tol_B)
    return dict(dbeta=(dbeta, tol_db), dgamma=(dgamma, tol_dg), dV0=(dV, tol_V), dU0=(dU, tol_U), indeg=deg[:, :, 0])


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_edge_train.py
# ---------------------------------------------------------------------------------------------------------------------
# the smallest that leave a ragged point tile, a ragged channel tile, a second channel tile and the workload's K
CASES = [(2, 33, 64, 4), (3, 40, 70, 5), (1, 64, 128, 20), (2, 200, 256, 20)]
OFFSET_CH = 3          # the channel that carries a constant offset of 32 standard deviations of z
ZERO_GAMMA = 2
NEG_GAMMA = slice(1, None, 3)
HUB, REPEAT_ROW, REPEATED = 1, 5, 7


def lonely(N):
    """the point nobody lists"""
    return N - 2


def make_case(B, N, C, K, seed=0):
    """float64 inputs of one case (the float32 values the kernel gets, exactly): channels with gamma < 0 (NEG_GAMMA), one with
    gamma == 0, one offset by 32 standard deviations; slot 0 of every row is the hub, row REPEAT_ROW lists REPEATED in
    every other slot (exact ties: the lower slot must win), nobody lists lonely(N)."""
    gen = torch.Generator().manual_seed(100000 * seed + 1000 * B + 10 * N + C + K)
    r = lambda *s: torch.randn(*s, generator=gen)
    U0, V0 = r(B, N, C), r(B, N, C)
    gamma = 0.5 + torch.rand(C, generator=gen)
    gamma[NEG_GAMMA] *= -1
    gamma[ZERO_GAMMA] = 0.0
    beta = r(C) * 0.5
    idx = torch.randint(0, N, (B, N, K), generator=gen)
    idx[idx == lonely(N)] = 0
    idx[:, :, 0] = HUB
    idx[:, REPEAT_ROW, 1:] = REPEATED
    zc = gather_rows(U0[:, :, OFFSET_CH:OFFSET_CH + 1], idx) + V0[:, :, None, OFFSET_CH:OFFSET_CH + 1]
    U0[:, :, OFFSET_CH] += 32.0 * float(zc.double().std(unbiased=False))     # the channel's z, 32 of its standard deviations up
    g = r(B, C, N)
    f32 = lambda t: t.float().double()
    return dict(U0=f32(U0), V0=f32(V0), idx=idx, gamma=f32(gamma), beta=f32(beta), g=f32(g),
                eps=float(torch.tensor(1e-5, dtype=torch.float32)), B=B, N=N, C=C, K=K)


def materialised(U0, V0, idx, gamma, beta, eps, arg):
    """The plain composition on the edge values, differentiable (torch autograd): z [B,C,N,K] = U0[idx] + V0 ->
    F.batch_norm(training=True) -> leaky_relu(0.2) -> the value at slot `arg` (the maximum over the slots when arg is the
    selection).  -> (y [B,C,N], full [B,C,N,K])"""
    import torch.nn.functional as F
    z = (gather_rows(U0, idx) + V0.unsqueeze(2)).permute(0, 3, 1, 2)
    full = F.leaky_relu(F.batch_norm(z, None, None, gamma, beta, True, 0.0, eps), SLOPE)
    y = torch.gather(full, 3, arg.long().permute(0, 2, 1).unsqueeze(3)).squeeze(3)
    return y, full
