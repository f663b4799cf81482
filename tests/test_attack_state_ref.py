"""CPU pin of tests/_attack_state_ref.py, the restatement tests/test_gpu_attack_state.py holds attack_state.hip to:

* against torch (autograd of the expressions of geoA3_attack.py:105-125, torch.argmax, torch.mode, torch.optim.Adam and
  torch.optim.SGD in float64) and against oracle/geoa3_oracle.py (lp_clip, offset_proj, find_offset);
* the binary update against the hand table of the issue;
* sensitivity: each deliberate mistake of R.MUTATIONS changes an exact result or exceeds tol on a named case;
* the lp_clip band holds at most 1e-3 of a case's points outside the planted ones;
* calibration: a plain float32 numpy evaluation, and one with every a*b + c rounded once, stay at or below half of every
  tol (the worst ratios are printed: run with -s; they are the CPU column of DESIGN 8c).
"""
import itertools

import numpy as np
import pytest
import torch

from oracle import geoa3_oracle as O
from tests import _attack_state_ref as R

F, D, U = np.float32, np.float64, R.U
T = torch.from_numpy
LOSSES = ((R.NONE, "None"), (R.CE, "CE"), (R.MARGIN, "Margin"))


# ----------------------------------------------------------------------------------------------------------------------
# the classification loss, label and vote against torch
# ----------------------------------------------------------------------------------------------------------------------
def torch_cls_loss(logits, target, typ, targeted, confidence, classes):
    """geoA3_attack.py:105-125 verbatim, on whatever dtype `logits` has."""
    if typ == "Margin":
        onehot = torch.zeros(target.size() + (classes,), dtype=logits.dtype)
        onehot.scatter_(1, target.unsqueeze(1), 1.)
        fake = (onehot * logits).sum(1)
        other = ((1. - onehot) * logits - onehot * 10000.).max(1)[0]
        if targeted:
            return torch.clamp(other - fake + confidence, min=0.)
        return torch.clamp(fake - other + confidence, min=0.)
    if typ == "CE":
        ce = torch.nn.CrossEntropyLoss(reduction="none")(logits, target)
        return ce if targeted else -ce
    return torch.zeros(logits.shape[0], dtype=logits.dtype)


@pytest.mark.parametrize("C", R.HEAD_CLASSES)
@pytest.mark.parametrize("targeted", (0, 1))
@pytest.mark.parametrize("typ,name", LOSSES)
def test_cls_loss_and_gradient_against_autograd(typ, name, targeted, C):
    for conf in (0.0, 0.5):
        case = R.head_case(typ, targeted, C, conf)
        st = case["state"]
        cl = R.classify(st, case["logits"])
        lg = T(case["logits"].astype(D)).requires_grad_()
        cls = torch_cls_loss(lg, T(st["target"].astype(np.int64)), name, targeted, conf, C)
        invb = float(st["inv_global_batch"])
        if cls.requires_grad:
            (cls * invb).sum().backward()      # loss_n.mean() with 1 / b (geoA3_attack.py:178)
            grad = lg.grad.numpy()
        else:
            grad = np.zeros_like(case["logits"], D)
        want = cls.detach().numpy()
        if typ == R.CE:
            (v, tol), (dv, dtol) = cl["cls_loss"], cl["dlogits"]
            np.testing.assert_allclose(v, want, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(dv, grad, rtol=1e-11, atol=1e-15)
            assert (tol > 0).all() and (dtol > 0).all()
        else:
            # three float32 operations on exact inputs: within 2u of the float64 value's terms; zero stays zero
            lgd = case["logits"].astype(D)
            scale = np.abs(lgd).max(1) * 2 + conf
            assert (np.abs(cl["cls_loss"].astype(D) - want) <= 2 * U * scale).all()
            assert ((cl["cls_loss"] == 0) == (want == 0)).all()
            assert np.array_equal(cl["dlogits"].astype(D), grad), (name, targeted, C, conf)


@pytest.mark.parametrize("C", R.HEAD_CLASSES)
def test_label_against_torch_argmax(C):
    for typ, targeted in itertools.product((R.CE, R.MARGIN), (0, 1)):
        case = R.head_case(typ, targeted, C, 0.0)
        cl = R.classify(case["state"], case["logits"])
        assert cl["label"].tolist() == torch.argmax(T(case["logits"]), 1).tolist()
        st = case["state"]
        want = (cl["label"] == st["target"]) if targeted else (cl["label"] != st["gt"])
        assert np.array_equal(cl["ok"].astype(bool), want)
        assert cl["last_label"][0] == cl["label"][-1]


@pytest.mark.parametrize("C", (40, 130))
@pytest.mark.parametrize("targeted", (0, 1))
@pytest.mark.parametrize("E", R.VOTE_EVAL)
def test_vote_against_torch_mode(E, targeted, C):
    case = R.vote_case(E, targeted, C)
    st = case["state"]
    cl = R.classify(st, case["logits"], case["vote_logits"])
    votes = torch.argmax(T(case["vote_logits"]), 2)
    assert np.array_equal(votes.numpy(), case["labels"]), "the planted votes are the arg-max of every vote row"
    assert cl["label"].tolist() == votes.mode(1).values.tolist()
    succ = O._compare(votes, T(st["target"].astype(np.int64)).view(-1, 1), T(st["gt"].astype(np.int64)).view(-1, 1),
                      bool(targeted)).sum(1) > 0.5 * E
    assert cl["ok"].astype(bool).tolist() == succ.tolist()
    rows = dict(zip(R.VOTE_ROWS, range(7)))
    assert cl["ok"][rows["unanimous"]] == 1 and cl["ok"][rows["exact_half"]] == 0
    assert cl["ok"][rows["half_plus_one"]] == 1
    if E % 2 == 0:
        assert cl["label"][rows["two_equal"]] == 5          # 5 and 9 equally often: the smaller
    if E % 3 == 0:
        assert cl["label"][rows["three_way"]] == 3
    r = rows["differs_from_logits"]
    assert cl["label"][r] != int(case["logits"][r].argmax()) and cl["ok"][r] == 1


# ----------------------------------------------------------------------------------------------------------------------
# optimisers against torch.optim in float64
# ----------------------------------------------------------------------------------------------------------------------
def test_adam_and_sgd_against_torch_optim():
    """Eight steps in float64 with the scalars AttackRunner._optim_scalars forms.  The restatement's constants are the
    kernel's float32 ones (0.9f, 0.1f, 0.999f, 0.001f, 1e-8f, the float32 step size), each within 2^-24 of torch's
    doubles: a step of size lr agrees to a few 2^-24 lr, eight of them to 8 * 8 * 2^-24 * lr."""
    rng = np.random.default_rng(3)
    shape, lr, steps = (3, 3, 50), 0.01, 8
    gs = rng.standard_normal((steps,) + shape) * 10.0 ** rng.uniform(-4, 0, (steps,) + shape)
    w0 = 1e-3 * rng.standard_normal(shape)
    z = np.zeros(shape)
    for kind in ("adam", "sgd", "sgd_momentum"):
        p = T(w0.copy()).requires_grad_()
        opt = (torch.optim.Adam([p], lr=lr) if kind == "adam" else
               torch.optim.SGD([p], lr=lr, momentum=0.9 if kind == "sgd_momentum" else 0.0))
        w, m, v = w0.copy(), z.copy(), z.copy()
        for t in range(steps):
            p.grad = T(gs[t].copy())
            opt.step()
            if kind == "adam":
                ss, bc2 = R.adam_scalars(t + 1, lr)
                (m, _), (v, _), (w, _) = R._adam(w, m, v, gs[t], z, ss, bc2, R.NO_MUT)
            elif kind == "sgd":
                w, _ = R._sgd(w, gs[t], z, lr)
            else:
                m, _ = R._momentum(m, gs[t], z, 0.9, t == 0)
                if t == 0:     # `first`: torch's buffer after the first step is the gradient itself
                    assert np.array_equal(opt.state[p]["momentum_buffer"].numpy(), gs[0]) and np.array_equal(m, gs[0])
                w, _ = R._sgd(w, m, z, lr)
            scale = lr * (1.0 if kind == "adam" else np.abs(gs[: t + 1]).sum(0) * 10)
            err = np.abs(w - p.detach().numpy())
            assert (err <= 64 * U * scale + 1e-18).all(), (kind, t, float((err / (64 * U * scale + 1e-18)).max()))


# ----------------------------------------------------------------------------------------------------------------------
# clip and projections against the oracle
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc", (0.004, 5e-7, 0.01))
def test_lp_clip_against_oracle(cc):
    rng = np.random.default_rng(11)
    o = (float(cc) * rng.standard_normal((3, 3, 200)) * 10.0 ** rng.uniform(-1.5, 1, (3, 1, 200))).astype(F)
    o[0, :, 0] = 0
    ccf = float(F(cc))
    (val, tol), alt, band = R.lp_clip(o.astype(D), np.zeros(o.shape), cc)
    assert not band.any()
    want = O.lp_clip(T(o.astype(D)), ccf).numpy()
    np.testing.assert_allclose(val, want, rtol=1e-13, atol=0)
    ln = np.sqrt((o.astype(D) ** 2).sum(1))
    assert (ln < ccf).any() and (ln > max(ccf, 1e-6)).any()
    if ccf < 1e-6:
        assert ((ln >= ccf) & (ln <= 1e-6)).any() and (val[:, :, (ln >= ccf).any(0) & (ln <= 1e-6).any(0)] == 0).any()
    # the reference's two `where`s turn a NaN coordinate into a zero vector
    o[1, 2, 7] = np.nan
    (val, tol), _, _ = R.lp_clip(o.astype(D), np.zeros(o.shape), cc)
    want = O.lp_clip(T(o.astype(D)), ccf).numpy()
    assert (want[1, :, 7] == 0).all() and (val[1, :, 7] == 0).all() and not np.isnan(val).any()


@pytest.mark.parametrize("B,N", R.UPDATE_SHAPES)
def test_projections_against_oracle(B, N):
    case = R.project_case(B, N, 0.0, "perm")
    ori, nrm, off, x = (case[k].astype(D) for k in ("ori", "normal", "offset", "x"))

    def brute_nn(q):
        d = ((q[:, :, :, None] - ori[:, :, None, :]) ** 2).sum(1)
        return d.argmin(2).astype(np.int32)
    nn = brute_nn(off)
    got = R.project(1, case["ori"], case["normal"], nn, case["offset"], case["x"], 0.0)["offset"][0]
    want = O.offset_proj(T(off), T(ori), T(nrm)).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-300)
    nn = brute_nn(x)
    got = R.project(0, case["ori"], None, nn, case["offset"], case["x"])["offset"]
    want = O.find_offset(T(ori), T(x)).numpy()
    assert got.dtype == F and np.array_equal(got, want.astype(F))   # one float32 subtraction: the rounded exact value


# ----------------------------------------------------------------------------------------------------------------------
# binary update: the hand table
# ----------------------------------------------------------------------------------------------------------------------
def table_row(cmp_and_score, lo, up, c):
    lo, up, c = F(lo), F(up), F(c)
    if cmp_and_score:
        lo2 = max(lo, c)
        return lo2, up, (F(F(lo2 + up) * F(0.5)) if up < F(1e9) else F(c * F(2)))
    up2 = min(up, c)
    return lo, up2, (F(F(lo + up2) * F(0.5)) if up2 < F(1e9) else c)


@pytest.mark.parametrize("targeted", (0, 1))
def test_binary_update_reproduces_the_table(targeted):
    st = R.binary_case(targeted)
    new = R.binary_update(st)
    last = int(st["last_label"][0])
    seen = set()
    for k in range(st["B"]):
        cmp = (last == st["target"][k]) if targeted else (last != st["gt"][k])
        yes = bool(cmp and st["iter_best_score"][k] != -1)
        lo2, up2, c2 = table_row(yes, st["lower_bound"][k], st["upper_bound"][k], st["scale_const"][k])
        got = (new["lower_bound"][k], new["upper_bound"][k], new["scale_const"][k])
        assert [a.tobytes() for a in got] == [F(a).tobytes() for a in (lo2, up2, c2)], k
        seen.add((yes, float(st["upper_bound"][k]), bool(st["lower_bound"][k] > st["scale_const"][k])))
    assert len(seen) == 2 * 4 * 2
    # up = 1e9 exactly takes the "else" side, the float32 below it the midpoint
    assert F(999999936.0) < F(1e9) and np.nextafter(F(999999936.0), F(2e9)) == F(1e9)
    assert table_row(True, 0.5, 1e9, 10)[2] == F(20) and table_row(True, 0.5, 999999936.0, 10)[2] == F(499999968.0)
    assert table_row(False, 0.5, 40, 10)[1:] == (F(10), F(5.25))
    yes_1e9 = [k for k in range(48) if st["upper_bound"][k] == F(1e9) and new["lower_bound"][k] >= st["scale_const"][k]
               and st["iter_best_score"][k] != -1 and new["upper_bound"][k] == F(1e9)]
    assert yes_1e9 and all(new["scale_const"][k] == F(st["scale_const"][k] * 2) for k in yes_1e9)


# ----------------------------------------------------------------------------------------------------------------------
# drivers shared by the sensitivity, band and calibration tests
# ----------------------------------------------------------------------------------------------------------------------
def run_script(mut=R.NO_MUT):
    """The state after every call of the scripted run (a later record overwrites an earlier wrong one)."""
    st, calls = R.bookkeeping_script()
    states = {}
    for i, c in enumerate(calls):
        if c["begin"]:
            st, _ = R.begin_search_step(st, c["x"], np.zeros_like(c["x"]))
        st, _ = R.head(st, c["logits"], c["constrain"], c["x"], c["step"], c["search_step"], mut=mut)
        states[i] = st
    return states


def differs(a, b):
    """Does result b (mutated) differ from a: an exact array in any bit, a (value, tol) beyond a's tol?"""
    if a is None or b is None:
        return (a is None) != (b is None)
    if R.is_tol(a):
        return R.ratio(b[0], a) > 1.0
    if isinstance(a, np.ndarray):
        return a.tobytes() != b.tobytes()
    if isinstance(a, dict):
        return any(differs(a[k], b[k]) for k in a if k in b and k not in ("band", "offset_alt"))
    return a != b


def update_first_step(case, optim, mut=R.NO_MUT, emu=None):
    lr = case["lr"]
    ss, bc2 = R.adam_scalars(1, lr) if optim == 0 else (lr, 1.0)
    g = lambda a: None if a is None else a[0]
    z = np.zeros_like(case["offset"])
    if emu is None:
        return R.update(case["state"], g(case["g_cls"]), g(case["g_geo"]), case["ori"], case["offset"], z, z, optim, ss,
                        bc2, case["cc_linf"], mut)
    return R.emu_update(case["state"], g(case["g_cls"]), g(case["g_geo"]), case["offset"], z, z, optim, ss, bc2,
                        case["cc_linf"], emu == "fused")


def partial_sgd(case, mut=R.NO_MUT):
    pm = np.full_like(case["part"], 3.0)      # whatever the buffer held before `first`
    return R.partial_step(case["state"], case["g_cls"][0], case["g_geo"][0], case["pidx"], case["periodical"],
                          case["part"], pm, None, 1, 0.01, 1.0, 0.9, 1, mut)


def head_of(case, mut=R.NO_MUT):
    st, out = R.head(case["state"], case["logits"], case["constrain"], case["x"], case["step"], case["search_step"],
                     case.get("vote_logits"), mut)
    return dict(st, dlogits=out["dlogits"], ok=out["ok"])


def project_of(case, mut=R.NO_MUT):
    return R.project(1, case["ori"], case["normal"], case["nn"], case["offset"], case["x"], case["cc_linf"], mut)


# mutation -> the named case that has to notice it
SENSITIVITY = {
    "best_le": lambda m: (run_script(), run_script(m)),                       # call 2: equal metric
    "iter_le": lambda m: (run_script(), run_script(m)),                       # call 9: equal metric, another label
    "metric_current": lambda m: (run_script(), run_script(m)),
    "argmax_high": lambda m: tuple(head_of(R.head_case(R.CE, 1, 65, 0.0), x) for x in (R.NO_MUT, m)),     # row two_max
    "other_high": lambda m: tuple(head_of(R.head_case(R.MARGIN, 1, 40, 0.5), x) for x in (R.NO_MUT, m)),  # row other_tie
    "hinge_zero_grad": lambda m: tuple(head_of(R.head_case(R.MARGIN, 0, 10, 0.5), x) for x in (R.NO_MUT, m)),
    "mode_large": lambda m: tuple(head_of(R.vote_case(2, 1), x) for x in (R.NO_MUT, m)),                  # row two_equal
    "vote_ge": lambda m: tuple(head_of(R.vote_case(64, 0), x) for x in (R.NO_MUT, m)),                    # row exact_half
    "beta_in_float": lambda m: tuple(update_first_step(R.update_case(3, 77, 0.0, "cls"), 0, x) for x in (R.NO_MUT, m)),
    "geo_no_inv_batch": lambda m: tuple(update_first_step(R.update_case(3, 77, 0.0, "geo"), 1, x)
                                        for x in (R.NO_MUT, m)),
    "clip_le": lambda m: tuple(update_first_step(R.update_case(3, 77, 5e-7, "cls"), 1, x) for x in (R.NO_MUT, m)),
    "proj_no_eps": lambda m: tuple(project_of(R.project_case(3, 77, 0.0, "perm"), x) for x in (R.NO_MUT, m)),
    "last_from_0": lambda m: (R.binary_update(R.binary_case(1)), R.binary_update(R.binary_case(1), m)),
    "lower_no_max": lambda m: (R.binary_update(R.binary_case(0)), R.binary_update(R.binary_case(0), m)),
    "test_on_lower": lambda m: (R.binary_update(R.binary_case(1)), R.binary_update(R.binary_case(1), m)),
    "momentum_at_first": lambda m: tuple(partial_sgd(R.partial_case(3, 77, 3), x) for x in (R.NO_MUT, m)),
}


@pytest.mark.parametrize("name", R.MUTATIONS)
def test_every_mistake_is_noticed(name):
    good, bad = SENSITIVITY[name](frozenset([name]))
    assert differs(good, bad), "no case notices the mistake `%s`: a case is missing" % name


def test_the_planted_clip_point_decides_exactly():
    """(cc_linf, 0, 0) with cc_linf = 5e-7: `len < cc_linf` is false, `len > 1e-6` is false: the point becomes 0 (with
    `<=` it would stay).  Under 0.004 it is rescaled to itself."""
    for cc in (5e-7, 0.004):
        case = R.update_case(3, 77, cc, "both")
        out = update_first_step(case, 0)
        b, n = case["planted"]["on_radius"]
        assert not out["band"][b, 0, n] and out["offset"][1][b, 0, n] <= 14 * R.KU * cc
        want = 0.0 if cc < 1e-6 else float(F(cc))
        assert out["offset"][0][b, 0, n] == want and (out["offset"][0][b, 1:, n] == 0).all()
        b, n = case["planted"]["nan_grad"]
        assert (out["offset"][0][b, :, n] == 0).all() and np.isnan(out["m"][0][b, 1, n])
        if cc < 1e-6:
            b, n = case["planted"]["between"]
            assert (out["offset"][0][b, :, n] == 0).all() and (out["offset"][1][b, :, n] == 0).all()
    case = R.update_case(3, 77, 0.0, "cls")
    b, n = case["planted"]["nan_grad"]
    got = update_first_step(case, 0)["offset"][0][b, :, n]
    assert np.isnan(got[1]) and not np.isnan(got[[0, 2]]).any()     # without a clip the NaN stays, at that coordinate


# ----------------------------------------------------------------------------------------------------------------------
# band cap and calibration
# ----------------------------------------------------------------------------------------------------------------------
UPDATE_GRID = [(B, N, cc, gr, optim) for (B, N) in R.UPDATE_SHAPES for cc in R.UPDATE_CC
               for gr, optim in (("cls", 0), ("geo", 1), ("both", 0), ("both", 1), ("none", 0))]


def test_band_holds_at_most_a_thousandth_of_the_points():
    for B, N, cc, gr, optim in UPDATE_GRID:
        case = R.update_case(B, N, cc, gr)
        out = update_first_step(case, optim)
        assert R.band_fraction(out["band"], case["planted"].values()) <= 1e-3, (B, N, cc, gr, optim)
    for (B, N), cc, kind in itertools.product(R.UPDATE_SHAPES, (0.0, 0.01), ("perm", "const")):
        out = project_of(R.project_case(B, N, cc, kind))
        assert R.band_fraction(out["band"]) <= 1e-3, (B, N, cc, kind)


def chain_ratios(case, optim, fused):
    """Six chained update steps in float32 (the evaluation's own m, v, offset carry on); every step against the
    restatement evaluated from that step's float32 inputs."""
    off, m, v = case["offset"].copy(), np.zeros_like(case["offset"]), np.zeros_like(case["offset"])
    worst = {}
    for t in range(case["steps"]):
        ss, bc2 = R.adam_scalars(t + 1, case["lr"]) if optim == 0 else (case["lr"], 1.0)
        gc = None if case["g_cls"] is None else case["g_cls"][t]
        gg = None if case["g_geo"] is None else case["g_geo"][t]
        ref = R.update(case["state"], gc, gg, case["ori"], off, m, v, optim, ss, bc2, case["cc_linf"])
        got = R.emu_update(case["state"], gc, gg, off, m, v, optim, ss, bc2, case["cc_linf"], fused)
        if optim == 0:
            worst["m"] = max(worst.get("m", 0), R.ratio(got["m"], ref["m"]))
            worst["v"] = max(worst.get("v", 0), R.ratio(got["v"], ref["v"]))
            m, v = got["m"], got["v"]
        worst["offset"] = max(worst.get("offset", 0),
                              R.ratio_either(got["offset"], ref["offset"], ref["offset_alt"], ref["band"]))
        off = got["offset"]
    return worst


def test_float32_evaluations_stay_below_half_of_tol():
    worst = {}

    def note(key, fused, r):
        k = (key, "fused" if fused else "plain")
        worst[k] = max(worst.get(k, 0.0), r)
    for typ in (R.CE, R.MARGIN, R.NONE):
        for targeted, C, conf in itertools.product((0, 1), R.HEAD_CLASSES, (0.0, 0.5)):
            case = R.head_case(typ, targeted, C, conf)
            st, out = R.head(case["state"], case["logits"], case["constrain"], case["x"], 2, 1)
            if typ == R.CE:
                cls, d = R.emu_ce(case["state"], case["logits"])
                note("ce cls_loss", False, R.ratio(cls, st["cls_loss"]))
                note("ce dlogits", False, R.ratio(d, out["dlogits"]))
            else:
                cls = st["cls_loss"]
            for fused in (False, True):
                note("loss_n", fused, R.ratio(R.emu_loss_n(case["state"], cls, case["constrain"], fused), st["loss_n"]))
    for B, N, cc, gr, optim in UPDATE_GRID:
        for fused in (False, True):
            for k, r in chain_ratios(R.update_case(B, N, cc, gr), optim, fused).items():
                note(("adam " if optim == 0 else "sgd ") + k, fused, r)
    for (B, N), cc, kind in itertools.product(R.UPDATE_SHAPES, (0.0, 0.01), ("perm", "const")):
        case = R.project_case(B, N, cc, kind)
        ref = project_of(case)
        for fused in (False, True):
            got = R.emu_project(case["normal"], case["nn"], case["offset"], cc, fused)
            note("project", fused, R.ratio_either(got, ref["offset"], ref["offset_alt"], ref["band"]))
    for (B, N), kr, optim in itertools.product(((1, 77), (3, 77), (7, 300)), (1, 3, 5), (0, 1)):
        case = R.partial_case(B, N, kr)
        for fused in (False, True):
            part, pm, pv = case["part"].copy(), np.full_like(case["part"], 3.0), np.zeros_like(case["part"])
            if optim == 0:
                pm[:] = 0
            for t in range(case["steps"]):
                args = (0,) + R.adam_scalars(t + 1) + (0.0, 0) if optim == 0 else (1, 0.01, 1.0, 0.9, int(t == 0))
                ref = R.partial_step(case["state"], case["g_cls"][t], case["g_geo"][t], case["pidx"],
                                     case["periodical"], part, pm, pv, *args)
                got = R.emu_partial(case["state"], case["g_cls"][t], case["g_geo"][t], case["pidx"], part, pm, pv, *args,
                                    fused)
                for k in ("part", "pm", "pv"):
                    if ref[k] is not None:
                        note("partial %s %s" % ("adam" if optim == 0 else "sgd", k), fused, R.ratio(got[k], ref[k]))
                part, pm = got["part"], got["pm"]
                pv = got["pv"] if optim == 0 else pv
    for k in sorted(worst):
        print("%-28s %-6s worst |err| / tol = %.3f" % (k[0], k[1], worst[k]))
    bad = {k: v for k, v in worst.items() if not v <= 0.5}
    assert not bad, bad
