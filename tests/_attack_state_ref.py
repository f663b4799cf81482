"""Plain numpy restatement of the nine entry points of geoa3_amd/csrc/attack_state.hip (no project code, no torch).

One function per entry, a direct statement of Attacker/geoA3_attack.py:88-127 (lp_clip, the classification loss),
:288-310 (success check, vote, best-so-far), :326-352 (optimiser step, projections, clip), :374-384 (binary search)
and :59-85 (offset_proj, find_offset).  States and results are dicts of arrays.

What a function returns for a quantity says how it is to be compared:

* a bare integer / float32 array is EXACT (bit for bit): label, ok, the mode, best_step, best_bs, iter_best_score,
  last_label, the rows that copy; best_loss / iter_best_loss / prev_constrain (copies of a float32 constrain); the Margin
  cls_loss (`other - fake + confidence`, in that order, then max with 0) and its dlogits (0 or +-inv_global_batch); the
  binary update (max, min, (lo + up) * 0.5, c * 2); find_offset (x - ori[:, nn]); begin_search_step.
* a tuple `(value, tol)` is a float64 value evaluated from the float32 inputs and the bound a float32 evaluation of the
  same expression has to meet: CE loss and gradient, loss_n, Adam's m, v and offset, SGD, both partial steps,
  offset_proj, lp_clip.  x is not restated: it is fl32(ori + offset) of the offset the kernel itself stored, bit for bit.

The bound
---------
u = 2^-24 is the relative error of one float32 operation (round to nearest), composed to first order; a fused
multiply-add is ONE operation (hipcc contracts a*b + c by default, so the product is not rounded), but whether a given
a*b + c is contracted is the compiler's choice, so wherever a product feeds a sum both the product and the sum are given
one u each.  expf, logf, sqrtf and `/` are taken at 2 ulp = 4u.  A float32 result below the normal range may lose all
its bits: 2^-126 absolute where that can happen (expf of a very negative argument; g*g*0.001 of a tiny gradient -- the
floor on v is given exactly where (g*g)*0.001 < 2^-126).  Every tol has the shape `c u mag + 2u |ref|`: `mag` is the
float64 sum of the absolute terms behind the entry, each weighted by the roundings it passes through (that weight is c;
nothing is fitted to a kernel), and 2u |ref| is the slack term of DESIGN 8a.

CE, one row (x = logits, mx = max x, t = x - mx, e = exp t, se = sum e, R = ceil(C / 64) + 6 roundings of the strided
sum and the six butterfly steps):
    rel(se)  <= u (R + 4 + sum(|t| e) / se) + C 2^-126 / se      (t: 1 op, expf: 4u, the sum: R u)
    tol(lse) = rel(se) + 4u |log se| + u |lse|                   (logf, then + mx)
    tol(ce)  = tol(lse) + u |ce| + 2u |ce|
    a = x - lse, p = exp a, q = p - onehot, d = sgn invB q:
    tol(d)   = invB (p (4u + u |a| + tol(lse)) + 2^-126 + u |q|) + 2u |d| + 2u |d|
loss_n = cls + scale_const * constrain:  tol = tol(cls) + u |sc con| + u |ln| + 2u |ln|.

Gradient g = g_cls + cg g_geo, cg = scale_const[b] * inv_global_batch (1 op): tol(g) = 2u |cg g_geo| + u |g| (nothing
without g_geo).  Adam (b1 = fl32(0.9), 1-b1 = fl32(0.1), b2 = fl32(0.999), 1-b2 = fl32(0.001): torch forms 1 - beta in
double and rounds once):
    tol(m') = 0.1 tol(g) + u (|b1 m| + |0.1 g| + |m'|)
    tol(v') = 0.001 (2 |g| tol(g)) + u (2 * 0.001 g^2 + |b2 v| + |v'|) [+ 2^-126]
    s = sqrt v':  ds = min(tol(v') / (2 s), sqrt tol(v')) + 4u s
    den = s / sqrt_bc2 + 1e-8:  dden = ds / sqrt_bc2 + 4u s / sqrt_bc2 + u den
    r = m' / den:  dr = tol(m') / den + |r| dden / den + 4u |r|
    w' = w - step_size r:  tol(w') = step_size dr + u |step_size r| + u |w'|
SGD: tol(w') = step_size tol(g) + u |step_size g| + u |w'|; with momentum buf = pm mom + g:
tol(buf) = tol(g) + u |pm mom| + u |buf| (0 at `first`, where buf = g).  Every offset tol then gets + 2u |w'|.

offset_proj (n = the normal, den = |n| + 1e-6): |n|^2 three terms (3u, halved by the root), sqrtf 4u, + 1e-6 u: den within
7u; nh = n / den within 11u; dot = sum o nh within 14u sum|o nh|; result dot nh:
    tol = |nh| 14u sum|o nh| + 12u |dot nh| + 2u |dot nh|.

lp_clip (len = sqrt sum o^2, inputs o with tolerance tol(o)): a scaled entry o / len * cc is
    tol = cc / len (tol(o) + |o| |dlen| / len) + 11u |res| + 2u |res|,   |dlen| = sqrt(sum tol(o)^2)
(three squares and two sums 3u halved, sqrtf 4u: len within 6u; `/` 4u; `*` u), a kept entry keeps tol(o), a zeroed entry
is exactly 0.  lp_clip is discontinuous at len == cc_linf and len == 1e-6: len is computed in float64, and where it lies
within `8u len + |dlen|` of a threshold both branches are returned and either is accepted (8u len is the kernel's own
rounding of len; |dlen| is what the tolerance of its input moves len by, zero when the clipped vector is an input or a
vector the step left alone: w - step * 0 is w, so a point with g = m = v = 0 has tol 0).  A vector with ONE non-zero
coordinate a has the exact length |a| in float32 too (the square is rounded once, its root is |a| again): no band, so the
planted (cc_linf, 0, 0) decides `len < cc_linf` exactly.
Outside the planted exact cases at most 1e-3 of a case's points may be in that band (`band_fraction`, asserted on the
CPU from this module alone).  A NaN coordinate makes len NaN: both `where`s of the reference pick the zero.

Every optimiser tol also carries 2^-126 absolute: an intermediate below the normal range (step_size * cg * 1e-30) keeps only
absolute accuracy.  Entries the derivation shows to be exact (w - step * 0) keep tol 0.

Calibration (tests/test_attack_state_ref.py, CPU only, never against a kernel): the `emu_*` functions below evaluate the
same expressions in numpy float32, once plainly and once with every a*b + c rounded once (product and sum in float64).
The first-order composition is attained almost entirely by an honest evaluation: with every rounding at 1 u the plain
evaluation reaches 0.79 of the bound (Adam's m, the momentum buffer), 0.74 (SGD's offset) and 0.52 (CE's gradient).  Every
rounding above is therefore given K u with K = 2 -- room for the second-order terms and for another association of the
same sums -- which puts both evaluations at or below half of tol on every case of this module.  K is not fitted to a
kernel and the band of lp_clip keeps the plain u.

`mut` (a set of names) switches on ONE deliberate mistake each; the CPU test shows that every one of them changes an
exact result or exceeds tol on a named case of this module.
"""
import math

import numpy as np

F = np.float32
D = np.float64
U = 2.0 ** -24
K = 2                # every rounding of the derivation is given K u (see "Calibration" above)
KU = K * U
TINY = 2.0 ** -126
BIG = F(1e10)
EPS6 = F(1e-6)
ADAM_EPS = F(1e-8)
B1, B1C, B2, B2C = F(0.9), F(0.1), F(0.999), F(0.001)
NEG = F(-10000.0)
NONE, CE, MARGIN = 0, 1, 2
NO_MUT = frozenset()
MUTATIONS = ("best_le", "iter_le", "argmax_high", "other_high", "mode_large", "vote_ge", "hinge_zero_grad",
             "metric_current", "beta_in_float", "geo_no_inv_batch", "clip_le", "proj_no_eps", "last_from_0",
             "lower_no_max", "test_on_lower", "momentum_at_first")


def is_tol(r):
    return isinstance(r, tuple)


# ------------------------------------------------------------------------------------------------------------------
# state
# ------------------------------------------------------------------------------------------------------------------
def new_state(B, N, classes, targeted, cls_loss_type, confidence, inv_global_batch, gt, target, scale_const,
              lower_bound=None, upper_bound=None, hist_steps=0):
    """The state attack() sets up before the first binary step (geoA3_attack.py:216-229)."""
    return dict(
        B=B, N=N, classes=classes, targeted=int(targeted), cls_loss_type=int(cls_loss_type), confidence=F(confidence),
        inv_global_batch=F(inv_global_batch), gt=np.asarray(gt, np.int32).copy(),
        target=np.asarray(target, np.int32).copy(), scale_const=np.asarray(scale_const, F).copy(),
        lower_bound=np.zeros(B, F) if lower_bound is None else np.asarray(lower_bound, F).copy(),
        upper_bound=np.full(B, BIG, F) if upper_bound is None else np.asarray(upper_bound, F).copy(),
        best_loss=np.full(B, BIG, F), best_attack=np.ones((B, 3, N), F), best_step=np.full(B, -1, np.int32),
        best_bs=np.full(B, -1, np.int32), iter_best_loss=np.full(B, BIG, F), iter_best_score=np.full(B, -1, np.int32),
        prev_constrain=np.full(B, BIG, F), label=np.full(B, -7, np.int32), cls_loss=np.full(B, -7, F),
        loss_n=np.full(B, -7, F), loss_hist=np.full((hist_steps, B), -7, F) if hist_steps else None,
        last_label=np.full(1, -7, np.int32))


def copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else
                tuple(a.copy() for a in v) if isinstance(v, tuple) else v) for k, v in st.items()}


def _compare(label, target, gt, targeted):
    return (label == target) if targeted else (label != gt)


def _argmax(row, high=False):
    """torch.argmax: the FIRST maximal index (`high`: the mistake of taking the last)."""
    assert not np.isnan(row).any(), "the restatement says nothing about a row with a NaN logit"
    idx = np.flatnonzero(row == row.max())
    return int(idx[-1] if high else idx[0])


def _mode(labels, large=False):
    """torch.mode: the most frequent value, the SMALLEST of equally frequent ones."""
    vals, cnt = np.unique(np.asarray(labels), return_counts=True)
    best = vals[cnt == cnt.max()]
    return int(best.max() if large else best.min())


# ------------------------------------------------------------------------------------------------------------------
# head
# ------------------------------------------------------------------------------------------------------------------
def classify(st, logits, vote_logits=None, mut=NO_MUT):
    """geoa3_attack_head_classify: cls_loss, dlogits (already carrying inv_global_batch), label, ok, last_label."""
    lg = np.asarray(logits, F)
    B, C = lg.shape
    assert B == st["B"] and C == st["classes"]
    tg, typ, invb, conf = st["targeted"], st["cls_loss_type"], st["inv_global_batch"], st["confidence"]
    label, ok = np.zeros(B, np.int32), np.zeros(B, np.int32)
    cls32, d32 = np.zeros(B, F), np.zeros((B, C), F)
    cls64, clstol, d64, dtol = np.zeros(B), np.zeros(B), np.zeros((B, C)), np.zeros((B, C))
    R = math.ceil(C / 64) + 6
    for b in range(B):
        tgt = int(st["target"][b])
        am = _argmax(lg[b], "argmax_high" in mut)
        if typ == MARGIN:
            w = lg[b].copy()
            w[tgt] = NEG                       # (1 - onehot) * logits - onehot * 1e4
            oi = _argmax(w, "other_high" in mut)
            other, fake = w[oi], lg[b, tgt]
            raw = F(F(other - fake) + conf) if tg else F(F(fake - other) + conf)
            cls32[b] = max(raw, F(0))
            passes = raw > 0 if "hinge_zero_grad" in mut else raw >= 0   # clamp(min=0) passes the gradient at equality
            g_other = (invb if passes else F(0)) * F(1 if tg else -1)
            d32[b, oi] += g_other
            d32[b, tgt] -= g_other
        elif typ == CE:
            x = lg[b].astype(D)
            mx = x.max()
            t = x - mx
            e = np.exp(t)
            se = e.sum()
            rel_se = KU * (R + 4 + (np.abs(t) * e).sum() / se) + C * TINY / se
            lse = math.log(se) + mx
            tol_lse = rel_se + 4 * KU * abs(math.log(se)) + KU * abs(lse)
            ce = lse - x[tgt]
            sgn = 1.0 if tg else -1.0
            cls64[b], clstol[b] = sgn * ce, tol_lse + 3 * KU * abs(ce)
            a = x - lse
            p = np.exp(a)
            q = p.copy()
            q[tgt] -= 1.0
            d = sgn * float(invb) * q
            d64[b] = d
            dtol[b] = float(invb) * (p * (4 * KU + KU * np.abs(a) + tol_lse) + TINY + KU * np.abs(q)) + 4 * KU * np.abs(d)
        if vote_logits is None:
            label[b] = am
            ok[b] = _compare(am, tgt, int(st["gt"][b]), tg)
        else:
            vl = np.asarray(vote_logits, F)[b]
            labs = [_argmax(r) for r in vl]
            n_ok = sum(bool(_compare(l, tgt, int(st["gt"][b]), tg)) for l in labs)
            label[b] = _mode(labs, "mode_large" in mut)
            half = F(0.5) * F(len(labs))
            ok[b] = (F(n_ok) >= half) if "vote_ge" in mut else (F(n_ok) > half)   # MORE than half
    out = dict(label=label, ok=ok, last_label=label[B - 1:].copy())
    if typ == CE:
        out["cls_loss"], out["dlogits"] = (cls64, clstol), (d64, dtol)
    else:
        out["cls_loss"], out["dlogits"] = cls32, d32
    return out


def finish(st, cl, constrain, x, step, search_step, mut=NO_MUT):
    """geoa3_attack_head_finish on the result `cl` of classify(): loss_n, the loss history and the best-so-far rules of
    geoA3_attack.py:301-310.  Returns (new state, rows whose iterate was copied into best_attack)."""
    st = copy_state(st)
    B = st["B"]
    con = np.zeros(B, F) if constrain is None else np.asarray(constrain, F)
    st["label"], st["last_label"], st["cls_loss"] = cl["label"].copy(), cl["last_label"].copy(), cl["cls_loss"]
    c64, ctol = cl["cls_loss"] if is_tol(cl["cls_loss"]) else (cl["cls_loss"].astype(D), np.zeros(B))
    with np.errstate(invalid="ignore", over="ignore"):
        prod = st["scale_const"].astype(D) * con.astype(D)
        ln = c64 + prod
        st["loss_n"] = (ln, ctol + KU * np.abs(prod) + 3 * KU * np.abs(ln))
    copied = []
    lt_best = (lambda a, b: a <= b) if "best_le" in mut else (lambda a, b: a < b)
    lt_iter = (lambda a, b: a <= b) if "iter_le" in mut else (lambda a, b: a < b)
    for b in range(B):
        metric = con[b] if "metric_current" in mut else st["prev_constrain"][b]   # the PREVIOUS step's constrain loss
        if cl["ok"][b] and lt_best(metric, st["best_loss"][b]):
            st["best_loss"][b], st["best_step"][b], st["best_bs"][b] = metric, step, search_step
            st["best_attack"][b] = np.asarray(x, F)[b]
            copied.append(b)
        if cl["ok"][b] and lt_iter(metric, st["iter_best_loss"][b]):
            st["iter_best_loss"][b], st["iter_best_score"][b] = metric, cl["label"][b]
    st["prev_constrain"] = con.copy()
    return st, copied


def head(st, logits, constrain, x, step, search_step, vote_logits=None, mut=NO_MUT):
    """geoa3_attack_head / geoa3_attack_head_vote.  Returns (new state, dict(dlogits, ok, copied))."""
    cl = classify(st, logits, vote_logits, mut)
    new, copied = finish(st, cl, constrain, x, step, search_step, mut)
    return new, dict(dlogits=cl["dlogits"], ok=cl["ok"], copied=copied)


# ------------------------------------------------------------------------------------------------------------------
# optimiser steps, clip, projections
# ------------------------------------------------------------------------------------------------------------------
def _gradient(st, g_cls, g_geo, shape, mut):
    """g = g_cls + scale_const[b] * inv_global_batch * g_geo as (value, tol), [B, 3, *]."""
    g = np.zeros(shape) if g_cls is None else np.asarray(g_cls, F).astype(D)
    tol = np.zeros(shape)
    if g_geo is not None:
        cg = st["scale_const"].astype(D) * (1.0 if "geo_no_inv_batch" in mut else float(st["inv_global_batch"]))
        with np.errstate(invalid="ignore"):
            term = cg.reshape(-1, 1, 1) * np.asarray(g_geo, F).astype(D)
            g = g + term
            tol = 2 * KU * np.abs(term) + KU * np.abs(g) + np.where(term != 0, TINY, 0.0)
    return g, tol


def _adam(w, m, v, g, tol_g, step_size, sqrt_bc2, mut):
    b2c = float(F(1) - B2) if "beta_in_float" in mut else float(B2C)
    b1c = float(F(1) - B1) if "beta_in_float" in mut else float(B1C)
    step_size, sqrt_bc2 = float(F(step_size)), float(F(sqrt_bc2))
    with np.errstate(invalid="ignore", divide="ignore"):
        m1 = float(B1) * m + b1c * g
        tol_m = b1c * tol_g + KU * (np.abs(float(B1) * m) + np.abs(b1c * g) + np.abs(m1)) + TINY
        gg = b2c * g * g
        v1 = float(B2) * v + gg
        tol_v = b2c * 2 * np.abs(g) * tol_g + KU * (2 * gg + np.abs(float(B2) * v) + np.abs(v1))
        tol_v = tol_v + np.where(gg < TINY, TINY, 0.0)
        s = np.sqrt(v1)
        ds = np.minimum(np.where(s > 0, tol_v / (2 * np.where(s > 0, s, 1.0)), np.inf), np.sqrt(tol_v)) + 4 * KU * s
        den = s / sqrt_bc2 + float(ADAM_EPS)
        dden = ds / sqrt_bc2 + 4 * KU * s / sqrt_bc2 + KU * den
        r = m1 / den
        dr = (tol_m - TINY) / den + np.abs(r) * dden / den + 4 * KU * np.abs(r)
        w1 = w - step_size * r
        tol_w = step_size * dr + KU * np.abs(step_size * r) + 3 * KU * np.abs(w1) + TINY
        tol_w = np.where((step_size * r == 0) & (dr == 0), 0.0, tol_w)     # w - 0 is w itself
    return (m1, tol_m + 2 * KU * np.abs(m1)), (v1, tol_v + 2 * KU * np.abs(v1)), (w1, tol_w)


def _sgd(w, g, tol_g, step_size):
    step_size = float(F(step_size))
    with np.errstate(invalid="ignore"):
        w1 = w - step_size * g
        tol_w = step_size * tol_g + KU * np.abs(step_size * g) + 3 * KU * np.abs(w1) + TINY
        return w1, np.where((step_size * g == 0) & (tol_g == 0), 0.0, tol_w)     # w - 0 is w itself


def _momentum(pm, g, tol_g, momentum, first, mut=NO_MUT):
    """torch.optim.SGD's buffer: the gradient itself at the first step, momentum * buf + g afterwards."""
    if first and "momentum_at_first" not in mut:
        return g, tol_g
    carried = float(F(momentum)) * pm
    buf = carried + g
    return buf, tol_g + KU * np.abs(carried) + KU * np.abs(buf) + TINY


def lp_clip(o, tol, cc_linf, mut=NO_MUT):
    """lp_clip of geoA3_attack.py:88-98 on [B, 3, N] float64 values with tolerance `tol`.  Returns
    ((value, tol), alt, band): alt = (value, tol) of the other branch where `band` [B, 1, N] is set, else None."""
    cc = float(F(cc_linf))
    if cc == 0.0:
        return (o, tol), None, np.zeros((o.shape[0], 1, o.shape[2]), bool)
    eps = float(EPS6)
    with np.errstate(invalid="ignore", divide="ignore"):
        nan = np.isnan(o).any(1, keepdims=True)
        o0, t0 = np.where(nan, 0.0, o), np.where(nan, 0.0, tol)
        ln = np.sqrt((o0 * o0).sum(1, keepdims=True))
        dln_in = np.sqrt((t0 * t0).sum(1, keepdims=True))
        # a vector with one non-zero coordinate has an exact length (sqrtf(fl(a * a)) == |a|): no band of its own
        band_w = np.where((o0 != 0).sum(1, keepdims=True) > 1, 8 * U * ln, 0.0) + dln_in
        lt = (ln <= cc) if "clip_le" in mut else (ln < cc)
        gt = ln > eps
        band_cc = (np.abs(ln - cc) <= band_w) & (band_w > 0)
        band_eps = (np.abs(ln - eps) <= band_w) & (band_w > 0) & ~(lt & ~band_cc)
        assert not (band_cc & band_eps).any(), "cc_linf this close to 1e-6 is not restated"
        safe = np.where(ln > 0, ln, 1.0)
        res = o0 / safe * cc
        tol_res = cc / safe * (t0 + np.abs(o0) * dln_in / safe) + 13 * KU * np.abs(res)

        def pick(lt_, gt_):
            val = np.where(lt_, o0, np.where(gt_, res, 0.0))
            tl = np.where(lt_, t0, np.where(gt_, tol_res, 0.0))
            return np.where(nan, 0.0, val), np.where(nan, 0.0, tl)
        band = (band_cc | band_eps) & ~nan
        main = pick(lt, gt)
        alt = pick(lt ^ band_cc, gt ^ band_eps) if band.any() else None
    return main, alt, band


def band_fraction(band, planted=()):
    """Share of a case's points inside the either-branch band, the planted points (list of (b, n)) left out."""
    bd = band.copy()
    for b, n in planted:
        bd[b, 0, n] = False
    return bd.sum() / bd.size


def update(st, g_cls, g_geo, ori, offset, m, v, optim, step_size, sqrt_bc2, cc_linf, mut=NO_MUT):
    """geoa3_attack_update: dict(m, v, offset as (value, tol); offset_alt, band for the clip's either-branch points)."""
    w = np.asarray(offset, F).astype(D)
    g, tol_g = _gradient(st, g_cls, g_geo, w.shape, mut)
    out = dict(m=None, v=None)
    if optim == 0:
        out["m"], out["v"], (w1, tol_w) = _adam(w, np.asarray(m, F).astype(D), np.asarray(v, F).astype(D), g, tol_g,
                                                step_size, sqrt_bc2, mut)
    else:
        w1, tol_w = _sgd(w, g, tol_g, step_size)
    out["offset"], out["offset_alt"], out["band"] = lp_clip(w1, tol_w, cc_linf, mut)
    return out


def project(mode, ori, normal, nn, offset, x, cc_linf=0.0, mut=NO_MUT):
    """geoa3_attack_project.  mode 0 (find_offset): the exact float32 x - ori[:, nn].  mode 1 (offset_proj + lp_clip):
    dict(offset=(value, tol), offset_alt, band)."""
    nn = np.asarray(nn).astype(np.int64)
    B, N = nn.shape
    idx = np.broadcast_to(nn[:, None, :], (B, 3, N))
    if mode == 0:
        return dict(offset=np.asarray(x, F) - np.take_along_axis(np.asarray(ori, F), idx, 2))
    n = np.take_along_axis(np.asarray(normal, F), idx, 2).astype(D)
    o = np.asarray(offset, F).astype(D)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt((n * n).sum(1, keepdims=True)) + (0.0 if "proj_no_eps" in mut else float(EPS6))
        nh = n / den
        terms = o * nh
        dot = terms.sum(1, keepdims=True)
        res = dot * nh
        tol = np.abs(nh) * 14 * KU * np.abs(terms).sum(1, keepdims=True) + 14 * KU * np.abs(res)
    out = {}
    out["offset"], out["offset_alt"], out["band"] = lp_clip(res, tol, cc_linf, mut)
    return out


def partial_step(st, g_cls, g_geo, pidx, periodical, part, pm, pv, optim, step_size, sqrt_bc2, momentum, first,
                 mut=NO_MUT):
    """geoa3_attack_partial_step on the [B, 3, kr] variable.  optim -1: nothing but x moves (returns {}).  Otherwise
    dict(part, pm, pv as (value, tol)); x[:, :, pidx] is fl32(periodical + part) of the stored part in every case."""
    if optim < 0:
        return {}
    pidx = np.asarray(pidx).astype(np.int64)
    B, kr = pidx.shape
    idx = np.broadcast_to(pidx[:, None, :], (B, 3, kr))
    gc = None if g_cls is None else np.take_along_axis(np.asarray(g_cls, F), idx, 2)
    gg = None if g_geo is None else np.take_along_axis(np.asarray(g_geo, F), idx, 2)
    w = np.asarray(part, F).astype(D)
    g, tol_g = _gradient(st, gc, gg, w.shape, mut)
    if optim == 0:
        pm1, pv1, p1 = _adam(w, np.asarray(pm, F).astype(D), np.asarray(pv, F).astype(D), g, tol_g, step_size, sqrt_bc2,
                             mut)
        return dict(part=p1, pm=pm1, pv=pv1)
    buf, tol_buf = _momentum(np.asarray(pm, F).astype(D), g, tol_g, momentum, first, mut)
    w1, tol_w = _sgd(w, buf, tol_buf, step_size)
    return dict(part=(w1, tol_w), pm=(buf, tol_buf + 2 * KU * np.abs(buf)), pv=None)


# ------------------------------------------------------------------------------------------------------------------
# binary search, start of a binary step
# ------------------------------------------------------------------------------------------------------------------
def binary_update(st, mut=NO_MUT):
    """geoA3_attack.py:374-384 in float32, with its quirk: the LAST instance's label decides for every k."""
    st = copy_state(st)
    lab = int(st["label"][0] if "last_from_0" in mut else st["last_label"][0])
    big9 = F(1e9)
    for k in range(st["B"]):
        c, lo, up = st["scale_const"][k], st["lower_bound"][k], st["upper_bound"][k]
        if _compare(lab, int(st["target"][k]), int(st["gt"][k]), st["targeted"]) and st["iter_best_score"][k] != -1:
            lo = c if "lower_no_max" in mut else max(lo, c)
            if (lo if "test_on_lower" in mut else up) < big9:
                c = F(F(lo + up) * F(0.5))
            else:
                c = F(c * F(2))
        else:
            up = min(up, c)
            if up < big9:
                c = F(F(lo + up) * F(0.5))
        st["scale_const"][k], st["lower_bound"][k], st["upper_bound"][k] = c, lo, up
    return st


def begin_search_step(st, ori, init_offset, have_adam=True):
    """geoa3_attack_begin_search_step: (new state, dict(offset, m, v, x)), all exact."""
    st = copy_state(st)
    st["iter_best_loss"][:] = BIG
    st["iter_best_score"][:] = -1
    st["prev_constrain"][:] = BIG
    o = np.asarray(init_offset, F).copy()
    z = np.zeros_like(o) if have_adam else None
    return st, dict(offset=o, m=z, v=None if z is None else z.copy(), x=np.asarray(ori, F) + o)


# ------------------------------------------------------------------------------------------------------------------
# float32 evaluations for the calibration (numpy float32; fused: every a*b + c rounded once)
# ------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c, fused):
    a, b, c = np.asarray(a, F), np.asarray(b, F), np.asarray(c, F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if fused:
            return (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)
        return (a * b + c).astype(F)


def emu_ce(st, logits):
    """Plain float32 CE loss and gradient (no product feeds a sum here: one evaluation)."""
    lg = np.asarray(logits, F)
    B, C = lg.shape
    sgn, invb = F(1 if st["targeted"] else -1), st["inv_global_batch"]
    cls, d = np.zeros(B, F), np.zeros((B, C), F)
    with np.errstate(under="ignore"):
        for b in range(B):
            tgt = int(st["target"][b])
            mx = lg[b].max()
            se = F(0)
            for e in np.exp(lg[b] - mx):
                se = F(se + e)
            lse = F(np.log(se) + mx)
            cls[b] = sgn * F(lse - lg[b, tgt])
            q = np.exp(lg[b] - lse)
            q[tgt] = F(q[tgt] - F(1))
            d[b] = F(sgn * invb) * q
    return cls, d


def emu_loss_n(st, cls, constrain, fused):
    return _fma(st["scale_const"], np.asarray(constrain, F), np.asarray(cls, F), fused)


def _emu_gradient(st, g_cls, g_geo, shape, fused):
    g = np.zeros(shape, F) if g_cls is None else np.asarray(g_cls, F)
    if g_geo is not None:
        cg = (st["scale_const"] * st["inv_global_batch"]).astype(F).reshape(-1, 1, 1)
        g = _fma(np.broadcast_to(cg, shape), g_geo, g, fused)
    return g


def _emu_adam(w, m, v, g, step_size, sqrt_bc2, fused):
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        m1 = _fma(m, B1, (g * B1C).astype(F), fused)
        v1 = _fma(v, B2, ((g * g).astype(F) * B2C).astype(F), fused)
        den = (np.sqrt(v1) / F(sqrt_bc2)).astype(F) + ADAM_EPS
        r = (m1 / den).astype(F)
        return m1, v1, _fma(-F(step_size), r, w, fused)


def emu_lp_clip(o, cc_linf, fused):
    cc = F(cc_linf)
    if cc == 0:
        return o
    with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
        l2 = _fma(o[:, 2:3], o[:, 2:3], _fma(o[:, 1:2], o[:, 1:2], (o[:, 0:1] * o[:, 0:1]).astype(F), fused), fused)
        ln = np.sqrt(l2)
        scaled = np.where(ln > EPS6, ((o / ln).astype(F) * cc).astype(F), F(0))
        return np.where(ln < cc, o, scaled).astype(F)


def emu_update(st, g_cls, g_geo, offset, m, v, optim, step_size, sqrt_bc2, cc_linf, fused):
    w = np.asarray(offset, F)
    g = _emu_gradient(st, g_cls, g_geo, w.shape, fused)
    m1 = v1 = None
    if optim == 0:
        m1, v1, w1 = _emu_adam(w, np.asarray(m, F), np.asarray(v, F), g, step_size, sqrt_bc2, fused)
    else:
        w1 = _fma(-F(step_size), g, w, fused)
    return dict(m=m1, v=v1, offset=emu_lp_clip(w1, cc_linf, fused))


def emu_project(normal, nn, offset, cc_linf, fused):
    nn = np.asarray(nn).astype(np.int64)
    B, N = nn.shape
    n = np.take_along_axis(np.asarray(normal, F), np.broadcast_to(nn[:, None, :], (B, 3, N)), 2)
    o = np.asarray(offset, F)
    with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
        n2 = _fma(n[:, 2:3], n[:, 2:3], _fma(n[:, 1:2], n[:, 1:2], (n[:, 0:1] * n[:, 0:1]).astype(F), fused), fused)
        den = np.sqrt(n2) + EPS6
        nh = (n / den).astype(F)
        dot = _fma(o[:, 2:3], nh[:, 2:3], _fma(o[:, 1:2], nh[:, 1:2], (o[:, 0:1] * nh[:, 0:1]).astype(F), fused), fused)
        return emu_lp_clip((dot * nh).astype(F), cc_linf, fused)


def emu_partial(st, g_cls, g_geo, pidx, part, pm, pv, optim, step_size, sqrt_bc2, momentum, first, fused):
    pidx = np.asarray(pidx).astype(np.int64)
    B, kr = pidx.shape
    idx = np.broadcast_to(pidx[:, None, :], (B, 3, kr))
    gc = None if g_cls is None else np.take_along_axis(np.asarray(g_cls, F), idx, 2)
    gg = None if g_geo is None else np.take_along_axis(np.asarray(g_geo, F), idx, 2)
    w = np.asarray(part, F)
    g = _emu_gradient(st, gc, gg, w.shape, fused)
    if optim == 0:
        m1, v1, w1 = _emu_adam(w, np.asarray(pm, F), np.asarray(pv, F), g, step_size, sqrt_bc2, fused)
        return dict(part=w1, pm=m1, pv=v1)
    buf = g if first else _fma(pm, F(momentum), g, fused)
    return dict(part=_fma(-F(step_size), buf, w, fused), pm=buf, pv=None)


def ratio(got, ref):
    """Worst |got - value| / tol of a (value, tol) result; entries that are NaN on both sides and exact zeros with a zero
    tol count as 0."""
    val, tol = ref
    got = np.asarray(got, D)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - val)
        both_nan = np.isnan(got) & np.isnan(val)
        r = np.where(both_nan | ((err == 0) & ~np.isnan(err)), 0.0, err / tol)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def ratio_either(got, ref, alt, band):
    """ratio() where a point inside `band` may meet either branch."""
    val, tol = ref
    got = np.asarray(got, D)

    def per_point(v, t):
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(got - v)
            r = np.where((np.isnan(got) & np.isnan(v)) | (err == 0), 0.0, err / t)
        return np.where(np.isnan(r), np.inf, r).max(1, keepdims=True)
    r = per_point(val, tol)
    if alt is not None:
        r = np.where(band, np.minimum(r, per_point(*alt)), r)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------------
# cases (shared by the CPU and the GPU test; generated from seeds, nothing recorded)
# ------------------------------------------------------------------------------------------------------------------
HEAD_CLASSES = (2, 10, 40, 64, 65, 130)
HEAD_ROWS = ("random", "two_max", "three_max", "target_max", "other_tie", "hinge_zero", "hinge_below")
HEAD_B, HEAD_N = 7, 77


def head_case(cls_loss_type, targeted, C, confidence, seed=0):
    """B = 7 rows of logits, one per HEAD_ROWS entry (N = 77: 3 N is no multiple of the workgroup)."""
    rng = np.random.default_rng(1000 * seed + 100 * cls_loss_type + 10 * targeted + C)
    B, N = HEAD_B, HEAD_N
    lg = (3 * rng.standard_normal((B, C))).astype(F)
    lg = np.clip(lg, -8, 8)
    tgt = rng.integers(0, C, B).astype(np.int32)
    conf = F(confidence)
    if cls_loss_type == CE:                       # +-80: exp underflows, the gradient saturates
        lg[0, 0], lg[0, C - 1] = 80, -80
    # two equal maxima: classes 0 and 64 share lane 0 of the strided walk, 63 | 64 are the wave's last and first lane
    two = (0, 64) if C >= 65 else (0, C - 1)
    three = (1, 63, 64) if C >= 65 else tuple(sorted({0, C // 2, C - 1}))
    lg[1, list(two)] = 9.25
    lg[2, list(three)] = 9.25
    tgt[1], tgt[2] = two[-1], three[-1]           # the tie includes the target: the first index wins, not the target
    lg[3, tgt[3]] = 9.5                            # the target is the maximum
    if C >= 3:                                    # `other` tied between two non-target classes, above everything else
        a, b = [c for c in (C - 1, 0, 1) if c != tgt[4]][:2]
        lg[4, [a, b]] = 8.75
    # hinge exactly 0 / one float32 below 0 (row 5 / row 6): fake and other are the two largest logits
    # targeted: raw = other - fake + conf with fake = hi, other = 1;  untargeted: fake - other + conf with other = hi,
    # fake = 1.  hi = 1 + conf gives raw == 0 exactly (0, 0.5 and 1.5 are representable), one float32 above it raw < 0.
    for row, below in ((5, False), (6, True)):
        t = int(tgt[row])
        o = (t + 1) % C
        lg[row] = np.clip(lg[row], -8, 0.5)
        hi = F(F(1.0) + conf)
        if below:
            hi = np.nextafter(hi, F(4))
        lg[row, t], lg[row, o] = (hi, F(1)) if targeted else (F(1), hi)
    gt = tgt.copy() if not targeted else ((tgt + 1 + rng.integers(0, C - 1, B)) % C).astype(np.int32)
    sc = (10.0 ** rng.uniform(-2, 2, B)).astype(F)
    con = (10.0 ** rng.uniform(-3, 1, B)).astype(F)
    x = rng.standard_normal((B, 3, N)).astype(F)
    st = new_state(B, N, C, targeted, cls_loss_type, conf, F(1.0 / 13.0), gt, tgt, sc, hist_steps=3)
    st["prev_constrain"] = (con * F(0.5)).astype(F)      # a previous step that beats 1e10: ok rows record
    return dict(state=st, logits=lg, constrain=con, x=x, step=2, search_step=1)


VOTE_EVAL = (1, 2, 3, 8, 63, 64)
VOTE_ROWS = ("unanimous", "exact_half", "half_plus_one", "two_equal", "three_way", "differs_from_logits", "random")


def vote_case(eval_num, targeted, C=40, seed=0):
    """B = 7 rows of vote patterns (VOTE_ROWS).  The labels are planted as one-hot-ish vote logits; target = 5, and
    the votes that do not succeed go to 9 / 3 / 7 (untargeted: gt = 5, a vote succeeds when it is NOT 5)."""
    rng = np.random.default_rng(77 * seed + eval_num + 1000 * targeted)
    B, N, E = 7, HEAD_N, eval_num
    tgt = np.full(B, 5, np.int32)
    gt = np.full(B, 11 if targeted else 5, np.int32)
    win = 5 if targeted else 9        # a label that satisfies _compare
    lose = 9 if targeted else 5       # one that does not
    labs = np.zeros((B, E), np.int64)
    labs[0] = win
    labs[1] = np.where(np.arange(E) < E // 2, win, lose)              # E even: exactly half (fails); E odd: below half
    labs[2] = np.where(np.arange(E) < E // 2 + 1, win, lose)          # half + 1 (odd E: the smallest majority)
    labs[3] = np.where(np.arange(E) % 2 == 0, 9, 5) if E % 2 == 0 else np.where(np.arange(E) < E // 2 + 1, 9, 5)
    labs[4] = np.array([7, 3, 9])[np.arange(E) % 3]                   # three-way: counts equal when 3 | E
    labs[5] = win
    labs[6] = rng.integers(0, 4, E)
    labs[3] = labs[3][rng.permutation(E)]
    vl = rng.standard_normal((B, E, C)).astype(F)
    for b in range(B):
        for e in range(E):
            vl[b, e, labs[b, e]] = 6.0
    vl[0, 0, 39] = 6.0                                                # a tie inside a vote row: the first index (5 / 9) wins
    if C > 64 + win:
        vl[0, 0, 64 + win] = 6.0                                      # and one on the same lane of the strided walk
    lg = rng.standard_normal((B, C)).astype(F)
    lg[5, lose] = 7.0                                                 # arg-max of `logits` disagrees with the vote
    sc = np.ones(B, F)
    con = (10.0 ** rng.uniform(-3, 1, B)).astype(F)
    x = rng.standard_normal((B, 3, N)).astype(F)
    st = new_state(B, N, C, targeted, MARGIN, F(0), F(1.0 / B), gt, tgt, sc, hist_steps=3)
    st["prev_constrain"] = (con * F(0.5)).astype(F)
    return dict(state=st, logits=lg, vote_logits=vl, constrain=con, x=x, step=1, search_step=0, labels=labs)


UPDATE_SHAPES = ((1, 1), (3, 77), (7, 300), (1, 257))
UPDATE_CC = (0.0, 0.004, 5e-7)


def adam_scalars(t, lr=0.01):
    """step_size and sqrt_bc2 of step t (1-based), formed in double as AttackRunner._optim_scalars forms them."""
    return lr / (1.0 - 0.9 ** t), math.sqrt(1.0 - 0.999 ** t)


def update_case(B, N, cc_linf, grads, steps=6, seed=0):
    """Inputs of a chain of `steps` update calls.  grads: 'cls', 'geo', 'both' or 'none'.  Gradients span six decades and
    carry exact zeros and 1e-30; scale_const differs by 1e4 between instances.  planted: {name: (b, n)}."""
    rng = np.random.default_rng(seed + 17 * B + N + int(cc_linf * 1e7))
    shape = (B, 3, N)
    cc = F(cc_linf)

    def grad():
        g = (rng.standard_normal((steps,) + shape) * 10.0 ** rng.uniform(-6, 0, (steps,) + shape)).astype(F)
        r = rng.random((steps,) + shape)
        g[r < 0.05] = 0
        g[(r >= 0.05) & (r < 0.1)] = 1e-30
        return g
    g_cls = grad() if grads in ("cls", "both") else None
    g_geo = grad() if grads in ("geo", "both") else None
    ori = rng.standard_normal(shape).astype(F)
    scale = 3e-3 if cc == 0 else float(cc) * (0.6 if cc > 1e-6 else 1.5)
    offset = (scale * rng.standard_normal(shape)).astype(F)
    planted = {}
    if N >= 77:
        b = B - 1
        planted = dict(on_radius=(b, 5), zero=(b, 9))
        if 0 < cc < EPS6:
            planted["between"] = (b, 13)
        if grads != "none":
            planted["nan_grad"] = (b, 20)
        for arr in (g_cls, g_geo):
            if arr is not None:
                for bb, nn in planted.values():
                    arr[:, bb, :, nn] = 0                                     # these points never move: m = v = 0
                arr[0, b, 1, 20] = np.nan                                     # one NaN gradient at the first step
        offset[b, :, 5] = (cc if cc != 0 else F(0.004), 0, 0)                 # length exactly cc_linf
        offset[b, :, 9] = 0
        if "between" in planted:
            offset[b, :, 13] = (F(7e-7), 0, F(2e-7))                          # cc_linf <= length <= 1e-6: becomes 0
    sc = (10.0 ** (4 * np.arange(B) / max(B - 1, 1) - 2)).astype(F)           # 1e-2 .. 1e2
    st = new_state(B, N, 40, 0, CE, F(0), F(1.0 / 13.0), np.zeros(B, np.int32), np.zeros(B, np.int32), sc)
    # Adam's first step moves every coordinate by lr: a quarter of the radius keeps all three clip branches populated
    lr = 0.01 if cc == 0 else float(cc) / 4
    return dict(state=st, g_cls=g_cls, g_geo=g_geo, ori=ori, offset=offset, cc_linf=float(cc), planted=planted,
                steps=steps, lr=lr)


def project_case(B, N, cc_linf, nn_kind, seed=0):
    """offset_proj inputs: normals of scale 1 with rows of scale 1e-3 / 1e3 and one zero normal; nn a permutation or constant."""
    rng = np.random.default_rng(seed + 31 * B + N + (0 if nn_kind == "perm" else 5))
    shape = (B, 3, N)
    ori = rng.standard_normal(shape).astype(F)
    nrm = rng.standard_normal(shape)
    nrm /= np.sqrt((nrm ** 2).sum(1, keepdims=True))
    scale = np.ones((B, 1, N))
    scale[:, :, 1::5], scale[:, :, 2::5] = 1e-3, 1e3
    nrm = (nrm * scale).astype(F)
    nrm[B - 1, :, N // 2] = 0
    offset = (0.01 * rng.standard_normal(shape)).astype(F)
    x = (ori + offset).astype(F)
    if nn_kind == "perm":
        nn = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.int32)
    else:
        nn = np.full((B, N), N // 2 if N > 1 else 0, np.int32)
    return dict(ori=ori, normal=nrm, offset=offset, x=x, nn=nn, cc_linf=float(F(cc_linf)))


def partial_case(B, N, kr, seed=0):
    rng = np.random.default_rng(seed + 13 * B + N + kr)
    steps = 4
    g_cls = (rng.standard_normal((steps, B, 3, N)) * 10.0 ** rng.uniform(-5, 0, (steps, B, 3, N))).astype(F)
    g_geo = rng.standard_normal((steps, B, 3, N)).astype(F)
    pidx = np.stack([rng.permutation(N)[:kr] for _ in range(B)]).astype(np.int32)
    periodical = rng.standard_normal((B, 3, N)).astype(F)
    part = (1e-3 * rng.standard_normal((B, 3, kr))).astype(F)
    sc = (10.0 ** (4 * np.arange(B) / max(B - 1, 1) - 2)).astype(F)
    st = new_state(B, N, 40, 0, CE, F(0), F(1.0 / 13.0), np.zeros(B, np.int32), np.zeros(B, np.int32), sc)
    return dict(state=st, g_cls=g_cls, g_geo=g_geo, pidx=pidx, periodical=periodical, part=part, steps=steps)


def binary_case(targeted):
    """B = 300 (more than one workgroup of 256): gt/target satisfying or not x iter_best_score {-1, 0, 5} x upper_bound
    {1e10, 1e9, the float32 below 1e9, 40} x lower_bound below / above scale_const, repeated to fill 300 rows."""
    rows = [(sat, s, up, lo) for sat in (0, 1) for s in (-1, 0, 5) for up in (1e10, 1e9, 999999936.0, 40.0)
            for lo in (0.5, 20.0)]
    B = 300
    rows = [rows[i % len(rows)] for i in range(B)]
    last = 7
    sat = np.array([r[0] for r in rows])
    # targeted: cmp = (last == target[k]);  untargeted: cmp = (last != gt[k])
    target = np.where(sat == 1, last, 3).astype(np.int32) if targeted else np.where(sat == 1, 3, last).astype(np.int32)
    gt = np.full(B, 1, np.int32) if targeted else target.copy()
    sc = np.full(B, 10.0, F)
    sc[48:] = (10.0 * (1 + np.arange(B - 48) / 64.0)).astype(F)
    st = new_state(B, 1, 40, targeted, NONE, F(0), F(1.0 / B), gt, target, sc,
                   lower_bound=[r[3] for r in rows], upper_bound=[r[2] for r in rows])
    st["iter_best_score"] = np.array([r[1] for r in rows], np.int32)
    st["label"] = np.full(B, last, np.int32)
    st["label"][0] = 3                       # instance 0's label differs from the last instance's
    st["last_label"][:] = last
    return st


BOOK_STEPS = 12


def bookkeeping_script(seed=0):
    """Twelve head calls on B = 7, N = 77 (3 N = 231 is no multiple of the 256-thread workgroup), loss type None,
    untargeted (the label of a success changes from call to call): the success pattern and the constrain values are dictated.  Row 3 never succeeds, row 5 succeeds only at
    every third call, the others follow the base script (metric = the PREVIOUS call's constrain, 1e10 after a begin):

      call  search/step  ok  constrain  metric  what happens
       0     0 / 0       y   5          1e10    success at step 0: nothing recorded (1e10 is not < 1e10)
       1     0 / 1       y   5          5       first record
       2     0 / 2       y   3          5       equal metric: not recorded
       3     0 / 3       n   2          3       better metric while failing: not recorded
       4     0 / 4       y   NaN        2       better metric while succeeding: recorded, best_attack = this x
       5     0 / 5       y   1          NaN     NaN metric: never recorded
       -- begin_search_step --                  iter_best_* restart, best_* persist
       6     1 / 0       y   4          1e10    nothing
       7     1 / 1       y   1.5        4       iter_best records (4 < 1e10), best does not (4 > 2)
       8     1 / 2       y   1.5        1.5     both record
       9     1 / 3       y   0.5        1.5     equal: nothing
      10     1 / 4       n   0.25       0.5     failing: nothing
      11     1 / 5       y   0.125      0.25    both record
    Row r's constrain is the base value times (1 + r / 8), exact in float32."""
    rng = np.random.default_rng(seed + 5)
    B, N, C = 7, 77, 10
    ok = np.array([1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 1], bool)
    con = np.array([5, 5, 3, 2, np.nan, 1, 4, 1.5, 1.5, 0.5, 0.25, 0.125])
    gt = np.array([0, 3, 9, 4, 5, 6, 2], np.int32)
    calls = []
    for t in range(BOOK_STEPS):
        okr = np.repeat(ok[t], B)
        okr[3] = False
        okr[5] = (t % 3 == 1)
        lg = rng.standard_normal((B, C)).astype(F)
        for b in range(B):                    # untargeted: success is any label but gt, and the label changes with the call
            lg[b, (gt[b] + 1 + t % 3) % C if okr[b] else gt[b]] = 5.0
        calls.append(dict(logits=lg, ok=okr, constrain=(con[t] * (1 + np.arange(B) / 8.0)).astype(F),
                          x=rng.standard_normal((B, 3, N)).astype(F), search_step=t // 6, step=t % 6,
                          begin=(t % 6 == 0)))
    sc = np.linspace(0.5, 2.0, B).astype(F)
    st = new_state(B, N, C, 0, NONE, F(0), F(1.0 / B), gt, gt, sc, hist_steps=6)
    return st, calls
