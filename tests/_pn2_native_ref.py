"""Plain restatements (CPU; torch float64, numpy float16 where a kernel's output IS fp16) of what the kernels of the
PointNet++ SSG native path compute, one function per kernel.  No project code.  tests/test_pn2_native_ref.py pins them to
torch autograd / plain matrix products and shows that each bound of tests/test_gpu_pn2_kernels.py notices one lost term.

Level 3's first layer is two kernels -- the split convolution (image form) and affine3_add_kernel (+ W_x xyz + bias, relu, in
place): conv(..., xyz=, Wx=, bias=, relu=) restates the pair, affine3_add the second kernel on its own.

Every restatement of a sum returns (value, mag): mag[entry] = the sum of the absolute values of the products behind that
entry, nested all the way down (tests/_pointnet_bwd_ref.py).  Keywords named skip_* restate a DEFECTIVE kernel.

The *_split functions emulate the kernels' arithmetic -- operands scaled by a power of two per tile / centre / image and
carried as fp16 pieces hi = rn16(v), lo = rn16(v - hi); a w = a_hi w_hi + a_hi w_lo + a_lo w_hi accumulated in float32 -- in
numpy float32 / float16.  They are held to the same bounds as the kernels, against the float64 restatements: what justifies
the bounds is measured against the reference, never against the kernel.
"""
from __future__ import annotations

import numpy as np
import torch

from tests._pointnet_bwd_ref import tolerance, worst_ratio  # noqa: F401  (re-exported: one definition of the bound)

SPLIT = 2.0 ** -21      # per split-fp16 product layer, in units of mag (derivation: tests/test_gpu_pn2_kernels.py)
F16_INF = 65520.0       # the smallest magnitude fp16 rounds to infinity (65504 is its largest finite value)


# ---------------------------------------------------------------------------------------------------------------------
# the scale rule and the fragment image (csrc/mfma_split.h, frag_image_kernel)
# ---------------------------------------------------------------------------------------------------------------------
def scale_exponent(m) -> int:
    """E = the biased float32 exponent of m >= 0, clamped to [14, 254]: scale 2^(140 - E) takes m into [2^13, 2^14)."""
    bits = int(np.float32(m).view(np.uint32))
    return min(max((bits >> 23) & 0xFF, 14), 254)


def scale_of(E: int) -> np.float32:
    return np.float32(2.0 ** (140 - E))


def unscale_of(E: int) -> np.float32:
    return np.float32(2.0 ** (E - 140))


def split16(v):
    """float32 array -> (hi, lo) numpy float16: hi = rn16(v), lo = rn16(v - hi) (the difference is exact in float32)."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def frag_image(W):
    """W [R][K] float32 (R % 32 == 0, K % 16 == 0) -> (E, hi, lo, pos): the image's scale exponent, the pieces of W 2^(140 - E)
    as float16 [R][K], and pos [2][R][K] = where piece p of entry (row, k) sits in the image:
    [row >> 5][k >> 4][piece][32 ((k >> 3) & 1) + (row & 31)][k & 7]."""
    W = np.asarray(W, dtype=np.float32)
    R, K = W.shape
    assert R % 32 == 0 and K % 16 == 0
    E = scale_exponent(np.abs(W).max())
    hi, lo = split16(W * scale_of(E))
    row, k = np.meshgrid(np.arange(R), np.arange(K), indexing="ij")
    pos = np.stack([(((((row >> 5) * (K >> 4) + (k >> 4)) * 2 + p) * 64 + 32 * ((k >> 3) & 1) + (row & 31)) * 8 + (k & 7))
                    for p in (0, 1)])
    return E, hi, lo, pos


def frag_image_flat(W):
    """(un, img): un = 2^(E - 140) as float32, img = the 2 R K float16 of the image in memory order."""
    E, hi, lo, pos = frag_image(W)
    img = np.zeros(2 * hi.size, dtype=np.float16)
    img[pos[0].ravel()] = hi.ravel()
    img[pos[1].ravel()] = lo.ravel()
    return unscale_of(E), img


# ---------------------------------------------------------------------------------------------------------------------
# sa2_pre_kernel: the pre-transformed first layer per point
# ---------------------------------------------------------------------------------------------------------------------
def point_major(f, channel_major: bool):
    """[P][128] from either layout of f: point-major [P][128], or channel-major [P / Np][128][Np]"""
    return f.permute(0, 2, 1).reshape(-1, f.shape[1]) if channel_major else f


def sa2_pre(f, xyz, Wf, Wx, channel_major=False, skip_ninth=False, skip_k=None):
    """Y[p][co] = sum_k f[p][k] Wf[co][k] + sum_d Wx[co][d] xyz[p][d] (no coordinate term when xyz is None).
    skip_ninth: the coordinates' k-step lost; skip_k: feature k left out."""
    X = point_major(f, channel_major)
    if skip_k is not None:
        X = X.clone()
        X[:, skip_k] = 0
    y, mag = X @ Wf.t(), X.abs() @ Wf.abs().t()
    if xyz is not None:
        mag = mag + xyz.abs() @ Wx.abs().t()        # (a lost term is still part of what the bound scales with)
        if not skip_ninth:
            y = y + xyz @ Wx.t()
    return y, mag


def wx_saturates(Wf, Wx) -> bool:
    """W_x carried at the scale of W_f's image: does an entry reach fp16's infinity?"""
    E = scale_exponent(np.abs(np.asarray(Wf, dtype=np.float32)).max())
    return bool((np.abs(np.asarray(Wx, dtype=np.float32) * scale_of(E)) >= F16_INF).any())


def _mm3(ah, al, bh, bl):
    """a_hi b_hi + a_hi b_lo + a_lo b_hi over the shared last axis, float32 (a product of two fp16 values is exact there)"""
    f = lambda t: t.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return f(ah) @ f(bh).T + f(ah) @ f(bl).T + f(al) @ f(bh).T


def sa2_pre_split(f, xyz, Wf, Wx, channel_major=False, wx_in_image_always=False):
    """sa2_pre in the kernel's arithmetic: a tile of 32 points takes one scale from the maximum of its features AND
    coordinates; W_f as its fragment image; the coordinates as a ninth k-step against W_x at the IMAGE's scale, per column
    tile of 32 channels -- unless an entry of that tile's W_x would reach fp16's infinity there, then the tile's coordinate
    term is three float32 multiply-adds onto the unscaled sum.  wx_in_image_always: without that exception (the kernel as
    it was: Inf / NaN from max|W_x| >= ~4 max|W_f| on)."""
    X = point_major(f, channel_major).numpy().astype(np.float32)
    Wf = np.asarray(Wf, dtype=np.float32)
    P = X.shape[0]
    E, wh, wl, _ = frag_image(Wf)
    sw, unW = scale_of(E), unscale_of(E)
    have = xyz is not None
    if have:
        q = xyz.numpy().astype(np.float32)
        Wx = np.asarray(Wx, dtype=np.float32)
        big = np.array([(np.abs(Wx[32 * t:32 * t + 32] * sw) >= F16_INF).any() for t in range(4)])
        if wx_in_image_always:
            big[:] = False
        xh, xl = split16(np.where(np.repeat(big, 32)[:, None], np.float32(0), Wx) * sw)
    Y = np.zeros((P, 128), dtype=np.float32)
    for p0 in range(0, P, 32):
        a = X[p0:p0 + 32]
        mx = np.abs(a).max()
        if have:
            mx = max(mx, np.abs(q[p0:p0 + 32]).max())
        Ex = scale_exponent(mx)
        sx = scale_of(Ex)
        ah, al = split16(a * sx)
        acc = _mm3(ah, al, wh, wl)
        if have:
            qh, ql = split16(q[p0:p0 + 32] * sx)
            acc = acc + _mm3(qh, ql, xh, xl)
        y = acc * (unscale_of(Ex) * unW)
        if have:
            for t in np.nonzero(big)[0]:
                w = Wx[32 * t:32 * t + 32]
                for d in range(3):
                    y[:, 32 * t:32 * t + 32] += q[p0:p0 + 32, d:d + 1] * w[None, :, d]
        Y[p0:p0 + 32] = y
    return torch.from_numpy(Y)


# ---------------------------------------------------------------------------------------------------------------------
# sa2_fwd8_kernel: gather + shift + relu, W1, W2 max-pooled over the 64 samples of a ball
# ---------------------------------------------------------------------------------------------------------------------
def gather_a0(rT, gidx, shift):
    """a0 [B][M][64][128] in the dtype of rT and shift -- FLOAT32 for a kernel's float32 inputs: relu(rT[b][gidx[b][m][s]] +
    shift[b][:, m]) is one add and one relu, so the kernel's gate bits m0 must match bit for bit"""
    B, M, S = gidx.shape
    rows = torch.stack([rT[b][gidx[b].long().reshape(-1)].reshape(M, S, -1) for b in range(B)])
    return (rows + shift.permute(0, 2, 1).unsqueeze(2)).clamp_min(0)


def sa2_fwd(rT, gidx, shift, W1, b1, W2, b2, skip_k1=None, skip_k2=None):
    """-> dict: a0 (float32), z1 / mag_z1 [B][M][64][128] (float64 pre-activation of layer 1), y2 / mag_y2 [B][256][M][64]
    (pre-pool), out [B][256][M] = relu(max_s y2), maximal [B][256][M][64] (bool: the samples that attain the maximum),
    arg = the first of them.  skip_k1 / skip_k2: that k left out of the first / second product."""
    a0 = gather_a0(rT, gidx, shift)
    x0 = a0.double()
    if skip_k1 is not None:
        x0 = x0.clone()
        x0[..., skip_k1] = 0
    W1, b1, W2, b2 = W1.double(), b1.double(), W2.double(), b2.double()
    z1 = x0 @ W1.t() + b1
    mag_z1 = a0.double() @ W1.abs().t() + b1.abs()
    a1 = z1.clamp_min(0)
    x1 = a1
    if skip_k2 is not None:
        x1 = a1.clone()
        x1[..., skip_k2] = 0
    y2 = (x1 @ W2.t() + b2).permute(0, 3, 1, 2).contiguous()
    mag_y2 = ((mag_z1 * (z1 > 0)) @ W2.abs().t() + b2.abs()).permute(0, 3, 1, 2).contiguous()
    top = y2.max(-1, keepdim=True).values
    maximal = y2 == top
    return dict(a0=a0, z1=z1, mag_z1=mag_z1, y2=y2, mag_y2=mag_y2, out=top.squeeze(-1).clamp_min(0), maximal=maximal,
                arg=maximal.to(torch.uint8).argmax(-1))


def sa2_fwd_tolerances(r, W2):
    """(tol_z1, tol_y2, tol_out) of a sa2_fwd result r.  Layer 1 is one split product of 128 terms + bias.  Layer 2 is
    another one, of an a1 that is itself off by up to tol_z1 (relu is 1-Lipschitz): tol_y2 = bound(y2) + sum_k |W2| tol_z1.
    relu and max are 1-Lipschitz: tol_out = max_s tol_y2."""
    tol_z1 = tolerance(r["z1"], r["mag_z1"], 129, extra=SPLIT)
    carried = (tol_z1 @ W2.double().abs().t()).permute(0, 3, 1, 2)
    tol_y2 = tolerance(r["y2"], r["mag_y2"], 129, extra=SPLIT) + carried
    return tol_z1, tol_y2, tol_y2.max(-1).values


def pack_gate_words(gate):
    """bool [..., 128] -> int64 [..., 4]: bit c of word w = channel 32 w + c (the rows of m0 / m1)"""
    sh = torch.arange(32, dtype=torch.int64)
    return (gate.reshape(*gate.shape[:-1], 4, 32).to(torch.int64) << sh).sum(-1)


def unpack_gate_words(words):
    """int32 / int64 [..., 4] -> bool [..., 128]"""
    w = words.to(torch.int64) & 0xFFFFFFFF
    sh = torch.arange(32, dtype=torch.int64)
    return ((w.unsqueeze(-1) >> sh) & 1).bool().reshape(*words.shape[:-1], 128)


def sa2_fwd_split(rT, gidx, shift, W1, b1, W2, b2):
    """sa2_fwd in the kernel's arithmetic -> (z1, y2) float32, shapes as sa2_fwd: a0 and a1 take one scale per CENTRE from
    the maximum over the centre's 64 samples x 128 channels, W1 / W2 are fragment images."""
    a0 = gather_a0(rT, gidx, shift).numpy()
    B, M = a0.shape[:2]
    E1, w1h, w1l, _ = frag_image(W1.numpy())
    E2, w2h, w2l, _ = frag_image(W2.numpy())
    b1, b2 = b1.numpy().astype(np.float32), b2.numpy().astype(np.float32)
    z1 = np.zeros((B, M, 64, 128), dtype=np.float32)
    y2 = np.zeros((B, 256, M, 64), dtype=np.float32)
    for b in range(B):
        for m in range(M):
            Ea = scale_exponent(a0[b, m].max())
            ah, al = split16(a0[b, m] * scale_of(Ea))
            z = _mm3(ah, al, w1h, w1l) * (unscale_of(Ea) * unscale_of(E1)) + b1
            z1[b, m] = z
            a1 = np.maximum(z, np.float32(0))
            Eh = scale_exponent(a1.max())
            hh, hl = split16(a1 * scale_of(Eh))
            y2[b, :, m, :] = (_mm3(hh, hl, w2h, w2l) * (unscale_of(Eh) * unscale_of(E2)) + b2).T
    return torch.from_numpy(z1), torch.from_numpy(y2)


# ---------------------------------------------------------------------------------------------------------------------
# sa2b_prep_kernel / sa2b_bwd_kernel / affine3_grad_pm_kernel / sa2b_centre_kernel: the level's backward
# ---------------------------------------------------------------------------------------------------------------------
SB_M, SB_S, SB_N1, SB_C, SB_P = 128, 64, 512, 256, 4


def pooled_gradient(dout, out):
    """g = dout where out > 0, else 0; a channel is LIVE where g != 0 (-0.0 is not)"""
    return torch.where(out > 0, dout, torch.zeros_like(dout))


def sa2_bwd(dout, out, arg, gidx, gate0, gate1, W1, W2, Wx, dnx2_in, skip_last_entry=(), zero_rows=(), skip_k=None,
            skip_samples=()):
    """dout / out / arg [B][256][128], gidx [B][128][64], gate0 / gate1 bool [B][128][64][128] (a0 > 0, a1 > 0 per row = (centre,
    sample)), W1 [128 k][128 i], W2 [256][128 k], Wx [128 i][3], dnx2_in [B][128][3].  With g = dout where out > 0 else 0:
        da1[row] = gate1 . sum_{ch: arg = s, g != 0} g W2[ch]        da0[row] = gate0 . W1^T da1[row]
        dr[j] = sum_{rows with gidx = j} da0        y[row] = Wx^T da0[row]        dnx2 = dnx2_in - sum_s y        dnx1 = Wx^T dr
    -> dict of (value, mag) pairs dr [B][512][128], y [B][128][64][3], dnx2, dnx1 [B][512][3], and `terms` = (most entries of a
    row, most rows of a destination).
    Defects: skip_last_entry (b, m, s): the row's highest live channel lost; zero_rows (b, m, s): the row's da0 lost; skip_k: that
    k left out of W1^T da1; skip_samples (b, m, s): the sample left out of its centre's coordinate sum."""
    dt = W1.dtype
    B = dout.shape[0]
    g = pooled_gradient(dout, out).to(dt)
    res = {k: [] for k in ("dr", "mdr", "y", "my", "dnx2", "mdnx2", "dnx1", "mdnx1")}
    most_e = most_r = 0
    cm = torch.arange(SB_M).view(1, SB_M).expand(SB_C, SB_M)
    cc = torch.arange(SB_C).view(SB_C, 1).expand(SB_C, SB_M)
    for b in range(B):
        live = g[b] != 0
        A = torch.zeros(SB_M, SB_S, SB_C, dtype=dt)
        A[cm[live], arg[b].long()[live], cc[live]] = g[b][live]
        for (bb, m, s) in skip_last_entry:
            if bb == b:
                A[m, s, int(torch.nonzero(A[m, s]).max())] = 0
        cnt = (A != 0).sum(-1)
        most_e = max(most_e, int(cnt.max()))
        dest = gidx[b].long().reshape(-1)
        hit = (cnt > 0).reshape(-1)
        if bool(hit.any()):
            most_r = max(most_r, int(torch.bincount(dest[hit], minlength=SB_N1).max()))
        g1, g0 = gate1[b].to(dt), gate0[b].to(dt)
        da1, ma1 = (A @ W2) * g1, (A.abs() @ W2.abs()) * g1
        W1k = W1
        if skip_k is not None:
            W1k = W1.clone()
            W1k[skip_k] = 0
        da0, ma0 = (da1 @ W1k) * g0, (ma1 @ W1.abs()) * g0
        for (bb, m, s) in zero_rows:
            if bb == b:
                da0[m, s] = 0
        dr = torch.zeros(SB_N1, 128, dtype=dt).index_add_(0, dest, da0.reshape(-1, 128))
        mdr = torch.zeros(SB_N1, 128, dtype=dt).index_add_(0, dest, ma0.reshape(-1, 128))
        y, my = da0 @ Wx, ma0 @ Wx.abs()
        ys = y.clone()
        for (bb, m, s) in skip_samples:
            if bb == b:
                ys[m, s] = 0
        for k, v in (("dr", dr), ("mdr", mdr), ("y", y), ("my", my), ("dnx2", dnx2_in[b].to(dt) - ys.sum(1)),
                     ("mdnx2", dnx2_in[b].to(dt).abs() + my.sum(1)), ("dnx1", dr @ Wx), ("mdnx1", mdr @ Wx.abs())):
            res[k].append(v)
    out_ = {k: (torch.stack(res[k]), torch.stack(res["m" + k])) for k in ("dr", "y", "dnx2", "dnx1")}
    out_["terms"] = (most_e, most_r)
    return out_


def sa2_bwd_tolerances(r):
    """dr: a row's sparse fp32 product (its entries), the split W1^T product (128), the destination's running sum (its
    rows); y: + 128 more; dnx2: + the centre's 64 samples and the caller's value; dnx1: dr's + 128.  One split product."""
    e, rows = r["terms"]
    n = {"dr": e + 128 + rows, "y": e + 128 + 128, "dnx2": e + 128 + 128 + 64 + 1, "dnx1": e + 128 + rows + 128}
    return {k: tolerance(r[k][0], r[k][1], max(n[k], 1), extra=SPLIT) for k in n}


def sa2b_tables(dout, out, arg, gidx):
    """The tables sa2b_prep_kernel promises for ONE cloud (dout / out / arg [256][128], gidx [128][64]), as numpy arrays:
    hit uint64 [128]; keys int32 [R]; ec int32 [E]; eg float32 [E]; td int32 [T][4]; ptile int32 [5]; pb (part cuts, rows);
    rows [R][3] = (dest, centre, sample) in order; first [R + 1] = the rows' first entries."""
    g = pooled_gradient(dout, out).float().numpy()
    a = arg.numpy().astype(np.int64)
    dst = gidx.numpy().astype(np.int64)
    live = g != 0
    cnt = np.zeros((SB_M, SB_S), dtype=np.int64)
    ch_i, m_i = np.nonzero(live)
    np.add.at(cnt, (m_i, a[ch_i, m_i]), 1)
    hit = np.array([sum(1 << s for s in range(SB_S) if cnt[m, s] > 0) for m in range(SB_M)], dtype=np.uint64)
    rows = sorted((int(dst[m, s]), m, s) for m in range(SB_M) for s in range(SB_S) if cnt[m, s] > 0)
    assert len({(j, m) for j, m, _ in rows}) == len(rows), "two hit rows of one centre at one destination: outside the contract"
    Rn = len(rows)
    dstart = np.zeros(SB_N1 + 1, dtype=np.int64)
    for j, _, _ in rows:
        dstart[j + 1] += 1
    dstart = np.cumsum(dstart)
    keys = np.zeros(Rn, dtype=np.int64)
    first = np.zeros(Rn + 1, dtype=np.int64)
    for pos, (j, m, s) in enumerate(rows):
        last = pos == Rn - 1 or rows[pos + 1][0] != j
        keys[pos] = j | (s << 9) | (m << 15) | ((1 << 31) if last else 0)
        first[pos + 1] = first[pos] + cnt[m, s]
    pb = [0]
    for q in range(1, SB_P):
        target = Rn * q // SB_P
        lo = int(np.searchsorted(dstart[:SB_N1], target, side="left"))       # first destination starting at or behind the target
        pb.append(int(dstart[lo]))
    pb.append(Rn)
    ptile = [0]
    for p in range(SB_P):
        ptile.append(ptile[-1] + (pb[p + 1] - pb[p] + 63) // 64)
    td = []
    for p in range(SB_P):
        for t in range(ptile[p + 1] - ptile[p]):
            row0 = pb[p] + 64 * t
            n = min(64, pb[p + 1] - row0)
            e0, e1 = int(first[row0]), int(first[row0 + n])
            em = int(first[row0 + 32]) if n > 32 else e1
            td.append((row0, n, e0, (e1 - e0) | ((em - e0) << 16)))
    ec = np.zeros(int(first[Rn]), dtype=np.int64)
    eg = np.zeros(int(first[Rn]), dtype=np.float32)
    for pos, (j, m, s) in enumerate(rows):
        p = sum(1 for q in range(1, SB_P) if pos >= pb[q])
        col = (pos - pb[p]) & 63
        chs = np.nonzero(live[:, m] & (a[:, m] == s))[0]
        e = int(first[pos])
        ec[e:e + len(chs)] = chs | (col << 16)
        ec[e + len(chs) - 1] |= 1 << 31
        eg[e:e + len(chs)] = g[chs, m]
    i32 = lambda v: np.asarray(v, dtype=np.int64).astype(np.uint32).view(np.int32)
    return dict(hit=hit, keys=i32(keys), ec=i32(ec), eg=eg, td=i32(np.array(td, dtype=np.int64).reshape(-1, 4)),
                ptile=i32(ptile), pb=pb, rows=np.array(rows, dtype=np.int64).reshape(-1, 3), first=first)


def sa2b_scratch_layout():
    """byte offsets of the per-cloud scratch (include/geoa3_hip_debug.h) and its size"""
    off, o = {}, 0
    for name, nbytes in (("keys", 8192 * 4), ("ec", 32768 * 4), ("eg", 32768 * 4), ("td", (8192 // 64 + SB_P) * 16),
                         ("ptile", 32), ("hit", 128 * 8), ("y", 8192 * 12)):
        off[name] = o
        o += nbytes
    return off, (o + 255) // 256 * 256


def sa2_bwd_split(dout, out, arg, gidx, gate0, gate1, W1, W2, Wx, dnx2_in):
    """The backward in the kernels' arithmetic for ONE cloud -> (dr, y, dnx2, dnx1) float32: a row's d a1 as a float32 sum
    over its entries; the rows in the tiles of sa2b_tables, each tile's d a1 at one power-of-two scale from its maximum, split;
    W1^T as a fragment image; float32 sums over a destination's rows, a row's 128 i, a centre's samples."""
    f32 = np.float32
    tb = sa2b_tables(dout, out, arg, gidx)
    E1, wh, wl, _ = frag_image(W1.numpy().T.copy())
    W2n, Wxn = W2.numpy().astype(f32), Wx.numpy().astype(f32)
    g0, g1 = gate0.numpy(), gate1.numpy()
    dr = np.zeros((SB_N1, 128), dtype=f32)
    y = np.zeros((SB_M, SB_S, 3), dtype=f32)
    for (row0, n, _, _) in tb["td"]:
        rows = tb["rows"][row0:row0 + n]
        da1 = np.zeros((n, 128), dtype=f32)
        for i, (j, m, s) in enumerate(rows):
            e0, e1 = tb["first"][row0 + i], tb["first"][row0 + i + 1]
            acc = np.zeros(128, dtype=f32)
            for e in range(e0, e1):
                acc = acc + tb["eg"][e] * W2n[tb["ec"][e] & 0xFFFF]
            da1[i] = acc * g1[m, s]
        Ex = scale_exponent(np.abs(da1).max())
        xh, xl = split16(da1 * scale_of(Ex))
        da0 = _mm3(xh, xl, wh, wl) * (unscale_of(Ex) * unscale_of(E1))
        for i, (j, m, s) in enumerate(rows):
            v = (da0[i] * g0[m, s]).astype(f32)
            dr[j] += v
            y[m, s] = (v[:, None] * Wxn).sum(0, dtype=f32)
    dnx2 = dnx2_in.numpy().astype(f32) - y.sum(1, dtype=f32)
    dnx1 = dr @ Wxn
    return tuple(torch.from_numpy(t) for t in (dr, y, dnx2, dnx1))


# ---------------------------------------------------------------------------------------------------------------------
# the glue kernels of pointnet2_net.hip
# ---------------------------------------------------------------------------------------------------------------------
def planar_to_points(x):
    """[B][3][N] -> [B][N][3]"""
    return x.permute(0, 2, 1).contiguous()


def points_to_planar(p):
    return p.permute(0, 2, 1).contiguous()


def gather_rows3(src, idx):
    """out[b][m] = src[b][idx[b][m]] (rows of 3)"""
    return torch.stack([src[b][idx[b].long()] for b in range(src.shape[0])])


def scatter_rows3(src, idx, N, into=None):
    """dst[b][n] (+)= sum over m with idx[b][m] == n of src[b][m], ascending m -> (value, mag, most terms of a row)"""
    B = src.shape[0]
    dst = torch.zeros(B, N, 3, dtype=src.dtype) if into is None else into.clone()
    mag = dst.abs()
    most = 0
    for b in range(B):
        dst[b].index_add_(0, idx[b].long(), src[b])
        mag[b].index_add_(0, idx[b].long(), src[b].abs())
        most = max(most, int(torch.bincount(idx[b].long(), minlength=N).max()))
    return dst, mag, most + (0 if into is None else 1)


def affine3(Wx, bias, p, sign):
    """out[b][co][m] = bias[co] + sign <Wx[co], p[b][m]> -> (value, mag)"""
    d = torch.einsum("cd,bmd->bcm", Wx, p)
    return bias.view(1, -1, 1) + sign * d, bias.abs().view(1, -1, 1) + torch.einsum("cd,bmd->bcm", Wx.abs(), p.abs())


def affine3_grad(dY, Wx):
    """dp[b][n][d] = sum_co Wx[co][d] dY[b][co][n] (dY channel-major) -> (value, mag)"""
    return torch.einsum("cd,bcn->bnd", Wx, dY), torch.einsum("cd,bcn->bnd", Wx.abs(), dY.abs())


def affine3_add(Y, Wx, bias, p, relu):
    """affine3_add_kernel, in place on a convolution's output: act(Y[b][co][n] + <Wx[co], p[b][n]> + bias[co]) -> (value, mag),
    mag on top of |Y| (the caller adds the magnitude behind Y itself).  conv(..., xyz=, Wx=, bias=, relu=) below is the
    convolution and this kernel in one: level 3's h1."""
    d = torch.einsum("cd,bnd->bcn", Wx, p)
    y, mag = Y + d, Y.abs() + torch.einsum("cd,bnd->bcn", Wx.abs(), p.abs())
    if bias is not None:
        y, mag = y + bias.view(1, -1, 1), mag + bias.abs().view(1, -1, 1)
    return (y.clamp_min(0) if relu else y), mag


# ---------------------------------------------------------------------------------------------------------------------
# sa1_fwd_kernel: level 1's forward (its z1, z2 and their tolerances are also the gates and bands of sa1_bwd below)
# ---------------------------------------------------------------------------------------------------------------------
def sa1_fwd(xyz, nx, gidx, layers, skip_k2=None):
    """ONE cloud: xyz [N][3], nx [M][3] centroids, gidx [M][64], layers = ((W1 [64][3], b1), (W2 [64][64], b2), (W3 [128][64], b3)):
    d = xyz[gidx] - nx in the dtype of xyz (FLOAT32 for a kernel's inputs: one subtraction, the kernel's operand), then in the
    dtype of the weights z1 = W1 d + b1, z2 = W2 relu(z1) + b2, y3 = W3 relu(z2) + b3, out = relu(max_s y3).
    -> dict out [M][128], y3 [M][64][128], arg (first maximal sample), tol_y3, tol_out: every layer is a split-fp16 product, so
    as for level 2 tol(z1) = bound(z1, 3 + 1 terms), tol(z2) = bound(z2, 64 + 1) + |W2| tol(z1), tol(y3) = bound(y3, 64 + 1) +
    |W3| tol(z2), tol(out) = max_s tol(y3); also z1, z2 [M][64][64] and t1, t2 = tol(z1), tol(z2).  skip_k2: that k left out of
    the second product."""
    (W1, b1), (W2, b2), (W3, b3) = layers
    dt = W1.dtype
    M = nx.shape[0]
    d = (xyz[gidx.long().reshape(-1)].reshape(M, 64, 3) - nx.unsqueeze(1)).to(dt)
    z1, m1 = d @ W1.t() + b1, d.abs() @ W1.abs().t() + b1.abs()
    a1 = z1.clamp_min(0)
    if skip_k2 is not None:
        a1 = a1.clone()
        a1[..., skip_k2] = 0
    z2, m2 = a1 @ W2.t() + b2, (m1 * (z1 > 0)) @ W2.abs().t() + b2.abs()
    y3, m3 = z2.clamp_min(0) @ W3.t() + b3, (m2 * (z2 > 0)) @ W3.abs().t() + b3.abs()
    t1 = tolerance(z1, m1, 4, extra=SPLIT)
    t2 = tolerance(z2, m2, 65, extra=SPLIT) + t1 @ W2.abs().t()
    t3 = tolerance(y3, m3, 65, extra=SPLIT) + t2 @ W3.abs().t()
    top = y3.max(1, keepdim=True).values
    return dict(out=top.squeeze(1).clamp_min(0), y3=y3, arg=(y3 == top).to(torch.uint8).argmax(1), tol_y3=t3,
                tol_out=t3.max(1).values, z1=z1, z2=z2, t1=t1, t2=t2)


# ---------------------------------------------------------------------------------------------------------------------
# sa1_bwd_kernel + sa1_scatter_kernel: level 1's backward.  The kernel recomputes z1 and z2 and takes its relu gates from
# THEIR signs, so a gate whose |z| lies inside tol(z) may differ from the float64 sign: sa1_bwd returns, beside (value, mag,
# tol), an ALLOWANCE per entry = what the in-band gates behind that entry toggle, to first order.
# ---------------------------------------------------------------------------------------------------------------------
def biased_exponent(m) -> int:
    return (int(np.float32(m).view(np.uint32)) >> 23) & 0xFF


def l1_exponent(x) -> int:
    """E with x < 2^E, from the float32 exponent field, at least -100 (sa1_stage's kw[3..8])"""
    return max(biased_exponent(x) - 126, -100)


def pad_mask(gidx):
    """bool [M][64]: samples that repeat the row's first index (the ball query's padding)"""
    pad = gidx == gidx[:, :1]
    pad[:, 0] = False
    return pad


def merge_padding(v, pad):
    """v [M][64][3]: the padded samples' rows added into sample 0 and zeroed"""
    p = pad.unsqueeze(-1).to(v.dtype)
    out = v * (1 - p)
    out[:, 0] = out[:, 0] + (v * p).sum(1)
    return out


def sa1_bwd(xyz, nx, gidx, layers, out, arg, g, lose=None):
    """ONE cloud, inputs as sa1_fwd plus out [M][128] (the pooled output: a channel is live where out > 0), arg [M][128] (the
    sample the channel's maximum sits at) and g [M][128] (the upstream gradient):
        dz3[s][ch] = g[ch] [out[ch] > 0] [arg[ch] == s]     dh2 = W3^T dz3      dz2 = dh2 [z2 > 0]
        dh1 = W2^T dz2      dz1 = dh1 [z1 > 0]      dp = W1^T dz1 per (centroid, sample), then the padded samples merged into
        sample 0;      dnew = -sum_s dp;      dxyz = the scatter of dp by gidx.
    -> dict: dp, dnew, dxyz = (value, mag, tol, allowance); pad; share = (the non-padded rows of dp with a non-zero allowance,
    the non-padded rows); Ex = the scatter's exponent (2^Ex above the largest |dp|).
    tol composes like sa1_fwd's: each product's own bound (128 / 64 / 64 terms; + SPLIT for the two split products) + the
    tolerance of its operand through the absolute weights and the gates that are open OR in band, + the operand floors
    (tests/test_gpu_pn2_sa1_bwd.py), computed from the centroid's largest live |g| WITHOUT the kernel's clamp: the reference and
    its bound are scale-free.  lose = (what, index): one term left out of the value (never of mag) --
    ("ch", (m, s, ch)), ("k2", j), ("row", i), ("sample", (m, s)), ("dup", (m, s)), ("entry", (m, s))."""
    (W1, b1), (W2, b2), (W3, b3) = layers
    dt = W1.dtype
    what, where = lose if lose is not None else (None, None)
    f = sa1_fwd(xyz, nx, gidx, layers)
    z1, z2, t1, t2 = f["z1"], f["z2"], f["t1"], f["t2"]
    M, N = nx.shape[0], xyz.shape[0]
    g0 = torch.where(out > 0, g, torch.zeros_like(g)).to(dt)
    onehot = arg.long().unsqueeze(1) == torch.arange(64).view(1, 64, 1)                    # [M][64][128]
    A = onehot.to(dt) * g0.unsqueeze(1)
    Av = A
    if what == "ch":
        Av = A.clone()
        Av[where] = 0
    # the operand floors: an element scaled by 2^k whose lo piece is an fp16 subnormal is carried to 2^-25 (half the subnormal
    # step 2^-24) there, 2^(-25 - k) unscaled.  dz3 rides at kg = 140 - E(max |g0|); dz2 at kg - EW3T (the accumulators hold
    # 2^(k3 + kg) dh2 and are scaled by 2^kd, kd = -k3 - EW3T, 2^EW3T above the largest column l1 norm of W3).
    gmax = g0.abs().max(1).values.float()
    fg = torch.tensor([2.0 ** (biased_exponent(v) - 165) if v > 0 else 0.0 for v in gmax.tolist()], dtype=dt).view(M, 1, 1)
    EW3T = l1_exponent(W3.float().abs().sum(0).max())
    fd = fg * 2.0 ** EW3T
    dh2, mag2 = Av @ W3, A.abs() @ W3.abs()
    tol2 = tolerance(dh2, mag2, 128, extra=SPLIT) + ((A != 0).to(dt) * fg) @ W3.abs()
    open2, band2 = z2 > 0, z2.abs() <= t2
    ok2 = (open2 | band2).to(dt)
    dz2 = dh2 * open2
    if what == "k2":
        dz2 = dz2.clone()
        dz2[..., where] = 0
    dh1, mag1 = dz2 @ W2, (mag2 * open2) @ W2.abs()
    tol1 = tolerance(dh1, mag1, 64, extra=SPLIT) + ((tol2 + fd * (mag2 > 0)) * ok2) @ W2.abs()
    open1, band1 = z1 > 0, z1.abs() <= t1
    ok1 = (open1 | band1).to(dt)
    dz1 = dh1 * open1
    if what == "row":
        dz1 = dz1.clone()
        dz1[..., where] = 0
    dp, magp = dz1 @ W1, (mag1 * open1) @ W1.abs()
    tolp = tolerance(dp, magp, 64) + (tol1 * ok1) @ W1.abs()
    # what the in-band gates toggle: a z2 gate j moves dz2[j] by |dh2[j]|, through |W2[j, :]|, the z1 gates that are open or in
    # band themselves (the cross term) and |W1|; a z1 gate i moves dz1[i] by |dh1[i]|, through |W1[i, :]|
    allow = ((((dh2.abs() * band2) @ W2.abs()) * ok1) + dh1.abs() * band1) @ W1.abs()
    pad = pad_mask(gidx)
    npad = pad.sum(1)
    dnew_v = dp
    if what == "sample":
        dnew_v = dp.clone()
        dnew_v[where] = 0
    dnew, mnew = -dnew_v.sum(1), magp.sum(1)
    tnew = tolp.sum(1) + tolerance(dnew, mnew, 64)
    dpv = dp
    if what == "dup":
        assert bool(pad[where])
        dpv = dp.clone()
        dpv[where] = 0
    dpm, magm, allowm = merge_padding(dpv, pad), merge_padding(magp, pad), merge_padding(allow, pad)
    tolm = merge_padding(tolp, pad)
    tolm[:, 0] = tolm[:, 0] + (npad > 0).to(dt).view(M, 1) * tolerance(torch.zeros_like(magm[:, 0]), magm[:, 0], 64)
    keep = ~pad
    if what == "entry":
        assert bool(keep[where])
        keep = keep.clone()
        keep[where] = False
    dest = gidx.long()[~pad]
    sc = lambda v, sel: torch.zeros(N, 3, dtype=dt).index_add_(0, gidx.long()[sel], v[sel])
    dxyz, magx, allowx, carried = sc(dpm, keep), sc(magm, ~pad), sc(allowm, ~pad), sc(tolm, ~pad)
    cnt = torch.bincount(dest, minlength=N).to(dt).view(N, 1)
    top = float(dpm.abs().max())
    Ex = min(max(biased_exponent(top) - 126, -80), 80)
    # the fixed-point scatter rounds every contribution to 2^(Ex' - 40), Ex' the exponent of the KERNEL's largest |dp|: within
    # its tolerance of the reference's, so at most one binade above; the float atomics (no scratch) are a plain fp32 sum
    tolx = carried + torch.maximum(cnt * 2.0 ** (Ex + 1 - 41) + 2.0 ** -24 * dxyz.abs(), tolerance(dxyz, magx, max(int(cnt.max()), 1)))
    live = ~pad
    share = (int((allowm[live] > 0).any(-1).sum()), int(live.sum()))
    return dict(dp=(dpm, magm, tolm, allowm), dnew=(dnew, mnew, tnew, allow.sum(1)), dxyz=(dxyz, magx, tolx, allowx), pad=pad,
                share=share, Ex=Ex)


def sa1_scatter_fixed(dp32, gidx, N):
    """sa1_scatter_kernel bit for bit, ONE instance: dp32 float32 [M][64][3], gidx [M][64] -> float32 numpy [N][3].  The largest
    finite magnitude of ALL entries by bit pattern (NaNs skipped) -> Ex = its exponent field - 126, clamped to [-80, 80]; every
    non-padded, finite contribution x -> round-half-even(x 2^(40 - Ex)) as a 64-bit integer (saturating); the integer sum per
    destination (wrapping); one rounding to float32, times 2^(Ex - 40).  A row with a NaN / infinite component makes its
    destination NaN; an infinite maximum makes every destination NaN."""
    d = np.ascontiguousarray(np.asarray(dp32, dtype=np.float32)).reshape(-1, 3)
    idx = np.asarray(gidx).astype(np.int64).reshape(-1, 64)
    bits = d.view(np.uint32) & np.uint32(0x7FFFFFFF)
    ok = bits <= 0x7F800000
    m = int(bits[ok].max()) if ok.any() else 0
    finite = m < 0x7F800000
    Ex = min(max(((m >> 23) & 0xFF) - 126, -80), 80)
    pad = idx == idx[:, :1]
    pad[:, 0] = False
    keep = ~pad.reshape(-1)
    dest = idx.reshape(-1)[keep]
    rows, rbits = d[keep], bits[keep]
    bad_row = (rbits >= 0x7F800000).any(1)
    bad = np.zeros(N, dtype=bool)
    bad[dest[bad_row]] = True
    with np.errstate(over="ignore", invalid="ignore"):
        scaled = np.float32(2.0 ** (40 - Ex)) * rows[~bad_row]                      # (float32: exact, a power of two)
    q = np.clip(np.rint(scaled.astype(np.float64)), -2.0 ** 63, 2.0 ** 63 - 1024)
    qi = np.where(q >= 2.0 ** 63 - 1024, np.int64(2 ** 63 - 1), q.astype(np.int64))
    acc = np.zeros((N, 3), dtype=np.int64)
    with np.errstate(over="ignore"):
        np.add.at(acc, dest[~bad_row], qi)
    out = acc.astype(np.float32) * np.float32(2.0 ** (Ex - 40))
    if not finite:
        bad[:] = True
    out[bad] = np.float32("nan")
    return out


def sa1_scatter_bound(dp32, gidx, N):
    """-> (float64 sum [N][3], bound [N][3], Ex) of one finite instance: cnt 2^(Ex - 41) + 2^-24 |sum|, cnt = the entries landing
    at the destination (each rounded to half a step of 2^(Ex - 40); one float32 rounding of the sum)"""
    d = torch.as_tensor(np.asarray(dp32, dtype=np.float32)).double().reshape(-1, 64, 3)
    idx = torch.as_tensor(np.asarray(gidx)).long().reshape(-1, 64)
    keep = ~pad_mask(idx)
    ref = torch.zeros(N, 3, dtype=torch.float64).index_add_(0, idx[keep], d[keep])
    cnt = torch.bincount(idx[keep], minlength=N).double().view(N, 1)
    Ex = min(max(biased_exponent(float(d.abs().max())) - 126, -80), 80)
    return ref, cnt * 2.0 ** (Ex - 41) + 2.0 ** -24 * ref.abs(), Ex


def sa_k(m, lo=110, hi=254) -> int:
    """the kernels' scale rule of pointnet2_sa.hip: k with m 2^k in [2^13, 2^14), the exponent field clamped to [lo, hi]"""
    return 140 - min(max(biased_exponent(m), lo), hi)


def sa_perm(p):
    """channel held at position p of a k-permuted image (the 32x32 accumulator's row order)"""
    ks, h, j = p >> 4, (p >> 3) & 1, p & 7
    return 32 * (ks >> 1) + 16 * (ks & 1) + 4 * h + (j & 3) + 8 * (j >> 2)


def sa1_bwd_split(xyz, nx, gidx, layers, out, arg, g, defect=None, flip=(), kg_lo=None):
    """sa1_bwd in the kernels' arithmetic for ONE cloud -> (dp merged, dnew, dxyz) float32: per centroid the differences at
    2^kp split, layer 1 as one product with hi and lo pieces of both sides (bias against 2^kp), h1 at the scale kx the l1 bounds
    give, layer 2 with its bias as the accumulators' initial value; the gates are the signs of THESE accumulators; the live
    gradient at 2^kg one-hot against the W3^T image, the gated result at 2^kd against the W2^T image, the gated result against
    W1 in float32; then the merge, the float32 sums and the fixed-point scatter.
    defect: "no_ex" (the merged duplicates left out of sample 0), "mask_block0" (samples 32-63 read the one-hot mask of samples
    0-31), "skip_ks3" / "skip_ks2" (the last k-step of the W3^T / W2^T product lost), "no_hcb" (every lane keeps the second column
    block's result).  flip: (layer, m, s, channel) gates inverted.  kg_lo: the lowest exponent field the gradient's scale
    follows -- None: the kernel's, max(14 + k2 - EW3T, 13), below which a centroid with gradient comes out as NaN; 110:
    the kernel as it was, which kept the scale 2^30 below 2^-17 and returned what was left (in the end zeros)."""
    f32 = np.float32
    F = lambda t: t.astype(f32)
    p2 = lambda k: f32(2.0 ** k)
    (W1, b1), (W2, b2), (W3, _) = [(w.numpy().astype(f32), b.numpy().astype(f32)) for w, b in layers]
    xyz, nx, idx = xyz.numpy().astype(f32), nx.numpy().astype(f32), gidx.numpy().astype(np.int64)
    out, arg, g = out.numpy().astype(f32), arg.numpy().astype(np.int64), g.numpy().astype(f32)
    M, N = nx.shape[0], xyz.shape[0]
    k1 = sa_k(max(np.abs(W1).max(), np.abs(b1).max()))
    k2, k3 = sa_k(np.abs(W2).max()), sa_k(np.abs(W3).max())
    EW1, EB1 = l1_exponent(np.abs(W1).sum(1, dtype=f32).max()), l1_exponent(np.abs(b1).max())
    EW2, EB2 = l1_exponent(np.abs(W2).sum(1, dtype=f32).max()), l1_exponent(np.abs(b2).max())
    EW3T = l1_exponent(np.abs(W3).sum(0, dtype=f32).max())
    w1h, w1l = split16(W1 * p2(k1))
    b1h, b1l = split16(b1 * p2(k1))
    w2h, w2l = split16(W2 * p2(k2))
    w3h, w3l = split16(W3 * p2(k3))
    kd = -k3 - EW3T
    loud = kg_lo is None
    if loud:
        kg_lo = max(14 + k2 - EW3T, 13)
    dp = np.zeros((M, 64, 3), dtype=f32)
    flips = {}
    for (layer, m, s, c) in flip:
        flips.setdefault((layer, m), []).append((s, c))
    for m in range(M):
        d = xyz[idx[m]] - nx[m]
        kp = sa_k(np.abs(d).max(), 126, 154)
        ph, pl = split16(d * p2(kp))
        one = p2(kp)
        z1 = (F(ph) @ F(w1h).T + F(b1h) * one + F(pl) @ F(w1h).T + F(b1l) * one + F(ph) @ F(w1l).T + F(pl) @ F(w1l).T).astype(f32)
        e1 = max(EW1 + 14 - kp, EB1) + 1
        kx = 14 - e1 - k1 - kp
        ka = k1 + kp + kx + k2
        xh, xl = split16(np.maximum(z1, f32(0)) * p2(kx))
        a2 = (b2 * p2(ka) + _mm3(xh, xl, w2h, w2l)).astype(f32)
        gate1, gate2 = z1 > 0, a2 > 0
        for s, c in flips.get((1, m), []):
            gate1[s, c] = ~gate1[s, c]
        for s, c in flips.get((2, m), []):
            gate2[s, c] = ~gate2[s, c]
        g0 = np.where(out[m] > 0, g[m], f32(0)).astype(f32)
        kg = sa_k(np.abs(g0).max(), kg_lo)
        gh, gl = split16(g0 * p2(kg))
        hot = arg[m][None, :] == np.arange(64)[:, None]                       # [64 s][128 ch]
        if defect == "mask_block0":
            hot[32:] = hot[:32]
        if defect == "skip_ks3":
            hot[:, 112:] = False
        Bh, Bl = np.where(hot, gh[None, :], np.float16(0)), np.where(hot, gl[None, :], np.float16(0))
        d2 = np.where(gate2, _mm3(Bh, Bl, w3h.T, w3l.T), f32(0)).astype(f32)
        eh, el = split16(d2 * p2(kd))
        if defect == "skip_ks2":
            eh[:, 48:], el[:, 48:] = 0, 0                                      # positions 48-63 hold channels 48-63 (sa_perm)
        d1 = _mm3(eh, el, w2h.T, w2l.T)
        v = np.where(gate1, d1, f32(0)).astype(f32)
        r = (v @ W1).astype(f32) * p2(-(k2 + kd + k3 + kg))
        if defect == "no_hcb":
            r[:32] = r[32:]
        if loud and np.abs(g0).max() > 0 and biased_exponent(np.abs(g0).max()) < kg_lo:
            r[:] = np.nan
        dp[m] = r
    pad = idx == idx[:, :1]
    pad[:, 0] = False
    dnew = -dp.sum(1, dtype=f32)
    merged = np.where(pad[..., None], f32(0), dp)
    if defect != "no_ex":
        merged[:, 0] += np.where(pad[..., None], dp, f32(0)).sum(1, dtype=f32)
    return torch.from_numpy(merged), torch.from_numpy(dnew), torch.from_numpy(sa1_scatter_fixed(merged, idx, N))


# ---------------------------------------------------------------------------------------------------------------------
# level 3 and the head: the split convolutions (image / slice / pooled forms), the sparse arg-max backward, the FC layers
# ---------------------------------------------------------------------------------------------------------------------
from tests._pointnet_bwd_ref import column_terms, fc, wide_bwd  # noqa: E402,F401  (taps = 1; fc: both directions)


def conv(W, X, bias=None, gate=None, relu=False, xyz=None, Wx=None, skip_k=None):
    """Y[b][co][n] = act(sum_k W[co][k] X[b][k][n] (+ <Wx[co], xyz[b][n]>) + bias[co]), kept where gate -> (value, mag)"""
    if skip_k is not None:
        X = X.clone()
        X[:, skip_k] = 0
    y, mag = torch.einsum("ok,bkn->bon", W, X), torch.einsum("ok,bkn->bon", W.abs(), X.abs())
    if xyz is not None:
        y = y + torch.einsum("od,bnd->bon", Wx, xyz)
        mag = mag + torch.einsum("od,bnd->bon", Wx.abs(), xyz.abs())
    if bias is not None:
        y, mag = y + bias.view(1, -1, 1), mag + bias.abs().view(1, -1, 1)
    if relu:
        y = y.clamp_min(0)
    if gate is not None:
        y, mag = y * gate.to(y.dtype), mag * gate.to(y.dtype)
    return y, mag


def conv_pool(W, X, bias):
    """pooled[b][co] = relu(max_n (W X + bias)), arg = the first maximal point -> (pooled, arg, y, mag of y)"""
    y, mag = conv(W, X, bias)
    top = y.max(-1, keepdim=True).values
    return top.squeeze(-1).clamp_min(0), (y == top).to(torch.uint8).argmax(-1), y, mag
