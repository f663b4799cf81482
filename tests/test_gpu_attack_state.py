"""Every kernel of geoa3_amd/csrc/attack_state.hip alone, through the C ABI (ctypes, torch tensors as buffers), against
the restatement tests/_attack_state_ref.py (pinned on the CPU by tests/test_attack_state_ref.py; the bound and its
derivation are in the restatement's docstring).

Integers, branch results, float32 copies and the short fixed float32 expressions are compared bit for bit; everything
else within the restatement's `tol`.  Chained steps carry the GPU's own state: every step is held to the restatement
evaluated from the float32 inputs that step had.  Each test prints its worst |err| / tol (run with -s).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _attack_state_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
EINVAL = -1
POISON = 12345.0
INT_KEYS = ("best_step", "best_bs", "iter_best_score", "label", "last_label")
COPY_KEYS = ("scale_const", "lower_bound", "upper_bound", "best_loss", "iter_best_loss", "prev_constrain", "best_attack")
STATE_KEYS = INT_KEYS + COPY_KEYS + ("cls_loss", "loss_n", "loss_hist")


@pytest.fixture(scope="module")
def lib():
    from geoa3_amd import _lib
    return _lib.load()


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def same_bits(a, b):
    """The same bits, a NaN matching any NaN (the payload of a NaN that arithmetic produced is not restated)."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and a[~na].tobytes() == b[~nb].tobytes()


class DevState:
    """The restatement's state dict on the device: one tensor per buffer (best_attack over-allocated by a guard row of
    1.0 after row B - 1) and the geoa3_attack_state that points at them."""

    def __init__(self, st, loss_hist=True):
        from geoa3_amd import _lib
        self.t = {k: cu(st[k]) for k in ("gt", "target") + INT_KEYS + COPY_KEYS if k != "best_attack"}
        for k in ("cls_loss", "loss_n"):
            self.t[k] = torch.full((st["B"],), POISON, device="cuda")
        ba = np.ones((st["B"] + 1, 3, st["N"]), F)
        ba[: st["B"]] = st["best_attack"]
        self.t["best_attack"] = cu(ba)
        self.t["loss_hist"] = cu(st["loss_hist"]) if (loss_hist and st["loss_hist"] is not None) else None
        self.B = st["B"]
        self.c = _lib.AttackState(B=st["B"], N=st["N"], classes=st["classes"], targeted=st["targeted"],
                                  cls_loss_type=st["cls_loss_type"], confidence=float(st["confidence"]),
                                  inv_global_batch=float(st["inv_global_batch"]),
                                  **{k: ptr(v) for k, v in self.t.items()})
        self.ref = C.byref(self.c)

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: (None if v is None else v.cpu().numpy().copy()) for k, v in self.t.items()}


def assert_result(got, want, what):
    """A bare array: the same bits.  (value, tol): within tol.  Returns the worst ratio."""
    if R.is_tol(want):
        r = R.ratio(got, want)
        assert r <= 1.0, (what, r)
        return r
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, got, want)
    return 0.0


def assert_state(snap, ref, what):
    worst = 0.0
    for k in INT_KEYS + COPY_KEYS:
        got = snap[k]
        if k == "best_attack":
            assert (got[-1] == 1.0).all(), (what, "the guard row after row B - 1 was written")
            got = got[:-1]
        assert_result(got, ref[k], (what, k))
    for k in ("cls_loss", "loss_n"):
        worst = max(worst, assert_result(snap[k], ref[k], (what, k)))
    return worst


def call_head(lib, dv, case, split=False, constrain=True, plain_entry=False):
    """One head step on DevState dv.  Returns (dlogits, ok or None) as numpy."""
    B, Cn = case["logits"].shape
    lg, x = cu(case["logits"]), cu(case["x"])
    vl = cu(case.get("vote_logits"))
    E = 0 if vl is None else vl.shape[1]
    con = cu(case["constrain"]) if constrain else None
    dl = torch.full((B, Cn), POISON, device="cuda")
    ok = None
    if split:
        ok = torch.full((B,), -9, dtype=torch.int32, device="cuda")
        assert lib.geoa3_attack_head_classify(dv.ref, ptr(lg), ptr(vl), E, ptr(dl), ptr(ok), stream()) == 0
        assert lib.geoa3_attack_head_finish(dv.ref, ptr(ok), ptr(con), ptr(x), case["step"], case["search_step"],
                                            stream()) == 0
    elif plain_entry:
        assert vl is None
        assert lib.geoa3_attack_head(dv.ref, ptr(lg), ptr(con), ptr(x), case["step"], case["search_step"], ptr(dl),
                                     stream()) == 0
    else:
        assert lib.geoa3_attack_head_vote(dv.ref, ptr(lg), ptr(vl), E, ptr(con), ptr(x), case["step"],
                                          case["search_step"], ptr(dl), stream()) == 0
    torch.cuda.synchronize()
    return dl.cpu().numpy(), (None if ok is None else ok.cpu().numpy())


def check_head_case(lib, case, what, plain_entry=False):
    """One-launch head against the restatement; then _classify + _finish on a second copy: every buffer the same bits."""
    st = case["state"]
    want, out = R.head(st, case["logits"], case["constrain"], case["x"], case["step"], case["search_step"],
                       case.get("vote_logits"))
    one = DevState(st)
    dl, _ = call_head(lib, one, case, plain_entry=plain_entry)
    snap = one.snapshot()
    worst = assert_state(snap, want, what)
    worst = max(worst, assert_result(dl, out["dlogits"], (what, "dlogits")))
    if st["cls_loss_type"] == R.NONE:
        assert dl.tobytes() == np.zeros_like(dl).tobytes()
    hist = snap["loss_hist"]
    assert hist[case["step"]].tobytes() == snap["loss_n"].tobytes(), (what, "loss_hist row")
    others = [i for i in range(hist.shape[0]) if i != case["step"]]
    assert (hist[others] == st["loss_hist"][others]).all()
    two = DevState(st)
    dl2, ok2 = call_head(lib, two, case, split=True)
    snap2 = two.snapshot()
    assert ok2.tolist() == out["ok"].tolist(), (what, "ok")
    assert dl2.tobytes() == dl.tobytes(), (what, "split dlogits")
    for k in STATE_KEYS:
        assert snap2[k].tobytes() == snap[k].tobytes(), (what, "split head differs in", k)
    return worst


# ----------------------------------------------------------------------------------------------------------------------
# head
# ----------------------------------------------------------------------------------------------------------------------
# shape of every case: B = 7 rows (R.HEAD_ROWS, one planted edge each), N = 77 (3 N = 231 is no multiple of 256)
@pytest.mark.parametrize("conf", (0.0, 0.5))
@pytest.mark.parametrize("Cn", R.HEAD_CLASSES)          # 64: one full wavefront; 65 / 130: a second and third strided pass
@pytest.mark.parametrize("targeted", (0, 1))
@pytest.mark.parametrize("typ", (R.NONE, R.CE, R.MARGIN))
def test_head_against_restatement(lib, typ, targeted, Cn, conf):
    case = R.head_case(typ, targeted, Cn, conf)
    worst = check_head_case(lib, case, (typ, targeted, Cn, conf), plain_entry=True)
    if typ == R.MARGIN:      # the planted rows are what they claim to be
        cl = R.classify(case["state"], case["logits"])
        rows = dict(zip(R.HEAD_ROWS, range(7)))
        assert cl["cls_loss"][rows["hinge_zero"]] == 0 and cl["cls_loss"][rows["hinge_below"]] == 0
        assert (cl["dlogits"][rows["hinge_zero"]] != 0).sum() == 2      # the gradient passes at equality
        assert (cl["dlogits"][rows["hinge_below"]] != 0).sum() == 0
    print("head", typ, targeted, Cn, conf, "worst err / tol %.3f" % worst)


def test_head_without_constrain_and_without_history(lib):
    for typ in (R.CE, R.MARGIN):
        case = R.head_case(typ, 1, 40, 0.5)
        st = case["state"]
        want, out = R.head(st, case["logits"], None, case["x"], case["step"], case["search_step"])
        assert (want["prev_constrain"] == 0).all()
        dv = DevState(st, loss_hist=False)
        assert dv.c.loss_hist is None
        dl, _ = call_head(lib, dv, case, constrain=False)
        assert_state(dv.snapshot(), want, "constrain = NULL")
        assert_result(dl, out["dlogits"], "dlogits")


@pytest.mark.parametrize("typ", (R.CE, R.MARGIN))
def test_head_nan_row_leaves_the_other_rows_alone(lib, typ):
    case = R.head_case(typ, 0, 65, 0.0)
    clean = DevState(case["state"])
    dl0, _ = call_head(lib, clean, case)
    bad = dict(case, logits=case["logits"].copy())
    bad["logits"][2, 64] = np.nan                   # not the last row: last_label stays that row's
    dirty = DevState(case["state"])
    dl1, _ = call_head(lib, dirty, bad)
    a, b = clean.snapshot(), dirty.snapshot()
    keep = [r for r in range(7) if r != 2]
    assert dl0[keep].tobytes() == dl1[keep].tobytes()
    for k in STATE_KEYS:
        if k == "last_label":
            assert a[k].tobytes() == b[k].tobytes()
        elif k == "loss_hist":
            assert a[k][:, keep].tobytes() == b[k][:, keep].tobytes()
        elif k == "best_attack":
            assert a[k][keep + [7]].tobytes() == b[k][keep + [7]].tobytes()
        else:
            assert a[k][keep].tobytes() == b[k][keep].tobytes(), k


# ----------------------------------------------------------------------------------------------------------------------
# vote
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", (40, 130))
@pytest.mark.parametrize("targeted", (0, 1))
@pytest.mark.parametrize("E", R.VOTE_EVAL)            # 64 fills s_vote and every lane of the mode's count
def test_vote_against_restatement(lib, E, targeted, Cn):
    case = R.vote_case(E, targeted, Cn)
    check_head_case(lib, case, ("vote", E, targeted, Cn))
    want, out = R.head(case["state"], case["logits"], case["constrain"], case["x"], case["step"], case["search_step"],
                       case["vote_logits"])
    rows = dict(zip(R.VOTE_ROWS, range(7)))
    # through ok, the bookkeeping: the exact half records nothing, half + 1 does
    assert want["best_step"][rows["exact_half"]] == -1 and want["best_step"][rows["half_plus_one"]] == case["step"]
    assert want["label"][rows["differs_from_logits"]] != case["logits"][rows["differs_from_logits"]].argmax()


# ----------------------------------------------------------------------------------------------------------------------
# bookkeeping over steps
# ----------------------------------------------------------------------------------------------------------------------
def test_bookkeeping_over_twelve_scripted_calls(lib):
    """B = 7, N = 77: R.bookkeeping_script's table.  After every call the complete state equals the restatement's."""
    st, calls = R.bookkeeping_script()
    dv = DevState(st)
    B, N = st["B"], st["N"]
    ori = np.zeros((B, 3, N), F)
    off, x = (torch.full((B, 3, N), POISON, device="cuda") for _ in range(2))
    recorded = {}
    for i, c in enumerate(calls):
        if c["begin"]:
            st, _ = R.begin_search_step(st, ori, ori)
            assert lib.geoa3_attack_begin_search_step(dv.ref, ptr(cu(ori)), ptr(cu(ori)), ptr(off), None, None, ptr(x),
                                                      stream()) == 0
            assert_state(dv.snapshot(), dict(st, cls_loss=dv.snapshot()["cls_loss"], loss_n=dv.snapshot()["loss_n"]),
                         ("begin", i))
        before = st
        st, out = R.head(st, c["logits"], c["constrain"], c["x"], c["step"], c["search_step"])
        assert out["ok"].astype(bool).tolist() == c["ok"].tolist()
        call_head(lib, dv, c)
        snap = dv.snapshot()
        assert_state(snap, st, ("call", i))
        assert snap["loss_hist"][c["step"]].tobytes() == snap["loss_n"].tobytes()
        for b in out["copied"]:
            assert snap["best_attack"][b].tobytes() == c["x"][b].tobytes()
        recorded[i] = out["copied"]
        if i in (0, 6):
            assert not out["copied"] and (st["iter_best_score"] == -1).all()       # 1e10 is not < 1e10
    # the script's table, row 0: records at calls 1, 4, 8, 11 only; row 3 never; the NaN metric of call 5 never
    assert [i for i in recorded if 0 in recorded[i]] == [1, 4, 8, 11]
    assert not any(3 in r for r in recorded.values()) and not recorded[5]
    assert (snap["best_attack"][3] == 1.0).all()
    assert st["best_bs"].tolist() == [1, 1, 1, -1, 1, 1, 1]


# ----------------------------------------------------------------------------------------------------------------------
# update
# ----------------------------------------------------------------------------------------------------------------------
def run_update_chain(lib, case, optim, rows=None, check=True):
    """The chain of case['steps'] geoa3_attack_update calls (rows: a batch-1 run of that row).  Returns the bits of
    (offset, m, v, x) after every step and the worst ratios."""
    st = case["state"]
    sel = slice(None) if rows is None else slice(rows, rows + 1)
    if rows is not None:
        st = dict(st, B=1, scale_const=st["scale_const"][sel], gt=st["gt"][sel], target=st["target"][sel])
        for k in ("lower_bound", "upper_bound", "best_loss", "best_step", "best_bs", "iter_best_loss", "iter_best_score",
                  "prev_constrain", "label", "best_attack"):
            st[k] = st[k][sel]
    dv = DevState(st)
    ori = cu(case["ori"][sel])
    off = cu(case["offset"][sel])
    m, v = torch.zeros_like(off), torch.zeros_like(off)
    x = torch.full_like(off, POISON)
    trace, worst = [], {"m": 0.0, "v": 0.0, "offset": 0.0}
    for t in range(case["steps"]):
        ss, bc2 = R.adam_scalars(t + 1, case["lr"]) if optim == 0 else (case["lr"], 1.0)
        gc = None if case["g_cls"] is None else case["g_cls"][t][sel]
        gg = None if case["g_geo"] is None else case["g_geo"][t][sel]
        pre = [a.cpu().numpy() for a in (off, m, v)]
        gct, ggt = cu(gc), cu(gg)
        assert lib.geoa3_attack_update(dv.ref, ptr(gct), ptr(ggt), ptr(ori), ptr(off), ptr(m) if optim == 0 else None,
                                       ptr(v) if optim == 0 else None, ptr(x), optim, ss, bc2, case["cc_linf"],
                                       stream()) == 0
        torch.cuda.synchronize()
        got = [a.cpu().numpy() for a in (off, m, v, x)]
        trace.append(b"".join(a.tobytes() for a in got))
        if check:
            ref = R.update(st, gc, gg, case["ori"][sel], pre[0], pre[1], pre[2], optim, ss, bc2, case["cc_linf"])
            if optim == 0:
                worst["m"] = max(worst["m"], assert_result(got[1], ref["m"], ("m", t)))
                worst["v"] = max(worst["v"], assert_result(got[2], ref["v"], ("v", t)))
            else:
                assert not got[1].any() and not got[2].any()          # SGD leaves the Adam buffers alone
            r = R.ratio_either(got[0], ref["offset"], ref["offset_alt"], ref["band"])
            assert r <= 1.0, ("offset", t, r)
            worst["offset"] = max(worst["offset"], r)
            assert same_bits(got[3], (case["ori"][sel] + got[0]).astype(F)), ("x = fl32(ori + offset)", t)
            if t == 0:
                assert R.band_fraction(ref["band"], case["planted"].values() if rows is None else ()) <= 1e-3
    return trace, worst, [a.cpu().numpy() for a in (off, m, v, x)]


# (1, 1): one thread; (3, 77): B N = 231 < 256; (7, 300): nine workgroups, the last partly filled; (1, 257): one thread
# in the second workgroup
@pytest.mark.parametrize("cc", R.UPDATE_CC)
@pytest.mark.parametrize("B,N", R.UPDATE_SHAPES)
@pytest.mark.parametrize("grads,optim", (("cls", 0), ("geo", 0), ("both", 0), ("none", 0), ("cls", 1), ("geo", 1),
                                         ("both", 1), ("none", 1)))
def test_update_against_restatement(lib, grads, optim, B, N, cc):
    case = R.update_case(B, N, cc, grads)
    sc = case["state"]["scale_const"]
    assert B == 1 or sc.max() / sc.min() >= 0.99e4
    trace, worst, final = run_update_chain(lib, case, optim)
    again, _, _ = run_update_chain(lib, case, optim, check=False)
    assert trace == again, "a second run gives other bits"
    b = B - 1
    one, _, row = run_update_chain(lib, case, optim, rows=b, check=False)
    for full, single in zip(final, row):
        assert full[b:b + 1].tobytes() == single.tobytes(), "a batch-1 run of the row gives other bits"
    pl = case["planted"]
    if pl:
        off = final[0]
        bb, n = pl["on_radius"]
        if cc != 0:       # it never moves (g = m = v = 0); under 5e-7 it is not < cc_linf and not > 1e-6: zero
            want = (0.0 if cc < 1e-6 else F(cc), 0.0, 0.0)
            assert off[bb, :, n].tolist() == [float(a) for a in want]
        bb, n = pl["zero"]
        assert not off[bb, :, n].any()
        if "between" in pl:
            bb, n = pl["between"]
            assert not off[bb, :, n].any()
        if "nan_grad" in pl:
            bb, n = pl["nan_grad"]
            if cc != 0:
                assert not off[bb, :, n].any()
            elif optim == 0:     # Adam keeps the NaN in m and v: the coordinate stays NaN, its neighbours do not
                assert np.isnan(off[bb, 1, n]) and not np.isnan(np.delete(off, n, 2)).any()
        # the planted points leave every other point alone: the same chain with ordinary values there
        plain = R.update_case(B, N, cc, grads)
        rng = np.random.default_rng(1)
        for bb, n in pl.values():
            plain["offset"][bb, :, n] = 1e-3 * rng.standard_normal(3)
            for key in ("g_cls", "g_geo"):
                if plain[key] is not None:
                    plain[key][:, bb, :, n] = rng.standard_normal((plain["steps"], 3))
        _, _, other = run_update_chain(lib, plain, optim, check=False)
        keep = np.ones(N, bool)
        keep[[n for _, n in pl.values()]] = False
        for a, c in zip(final, other):
            assert a[:, :, keep].tobytes() == c[:, :, keep].tobytes(), "a planted point moved another point"
    print("update", grads, optim, B, N, cc, " ".join("%s %.3f" % kv for kv in worst.items()))


# ----------------------------------------------------------------------------------------------------------------------
# project
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("perm", "const"))
@pytest.mark.parametrize("cc", (0.0, 0.01))
@pytest.mark.parametrize("B,N", R.UPDATE_SHAPES)
def test_project_against_restatement(lib, B, N, cc, kind):
    case = R.project_case(B, N, cc, kind)
    ori, nrm, nn = cu(case["ori"]), cu(case["normal"]), cu(case["nn"])
    # mode 0, find_offset: exact; x is not written
    off, x = torch.full((B, 3, N), POISON, device="cuda"), cu(case["x"])
    assert lib.geoa3_attack_project(0, ptr(ori), None, ptr(nn), ptr(off), ptr(x), B, N, 0.0, stream()) == 0
    torch.cuda.synchronize()
    assert_result(off.cpu().numpy(), R.project(0, case["ori"], None, case["nn"], None, case["x"])["offset"], "find_offset")
    assert bits(x) == case["x"].tobytes()
    # mode 1, offset_proj then lp_clip
    off, x = cu(case["offset"]), torch.full((B, 3, N), POISON, device="cuda")
    assert lib.geoa3_attack_project(1, ptr(ori), ptr(nrm), ptr(nn), ptr(off), ptr(x), B, N, cc, stream()) == 0
    torch.cuda.synchronize()
    got = off.cpu().numpy()
    ref = R.project(1, case["ori"], case["normal"], case["nn"], case["offset"], case["x"], cc)
    r = R.ratio_either(got, ref["offset"], ref["offset_alt"], ref["band"])
    assert r <= 1.0, r
    assert R.band_fraction(ref["band"]) <= 1e-3
    assert bits(x) == (case["ori"] + got).astype(F).tobytes()
    zero = case["nn"] == (N // 2 if N > 1 else 0)
    if B > 1 or N > 1:
        assert not got[B - 1][:, zero[B - 1]].any(), "a zero normal projects to 0"
    print("project", B, N, cc, kind, "worst err / tol %.3f" % r)


# ----------------------------------------------------------------------------------------------------------------------
# partial step
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kr", (1, 3, 5))
@pytest.mark.parametrize("B,N", ((1, 77), (3, 77), (7, 300)))
def test_partial_step_against_restatement(lib, B, N, kr):
    case = R.partial_case(B, N, kr)
    st = case["state"]
    dv = DevState(st)
    pidx, per = cu(case["pidx"]), cu(case["periodical"])
    assert all(len(set(r)) == kr for r in case["pidx"].tolist())
    idx = np.broadcast_to(case["pidx"].astype(np.int64)[:, None, :], (B, 3, kr))
    worst = {}
    for optim in (-1, 0, 1):
        part = cu(case["part"])
        pm = torch.full_like(part, 0.0 if optim == 0 else 3.0)       # SGD: whatever the buffer held before `first`
        pv = torch.zeros_like(part)
        x = torch.full((B, 3, N), POISON, device="cuda")
        for t in range(1 if optim < 0 else case["steps"]):
            args = ((-1, 0.0, 1.0, 0.0, 0) if optim < 0 else (0,) + R.adam_scalars(t + 1) + (0.0, 0) if optim == 0 else
                    (1, 0.01, 1.0, 0.9, int(t == 0)))
            pre = [a.cpu().numpy() for a in (part, pm, pv)]
            x.fill_(POISON)
            gc, gg = cu(case["g_cls"][t]), cu(case["g_geo"][t])
            assert lib.geoa3_attack_partial_step(dv.ref, ptr(gc), ptr(gg), ptr(pidx), kr, ptr(per), ptr(part), ptr(pm),
                                                 ptr(pv), ptr(x), *args, stream()) == 0
            torch.cuda.synchronize()
            got = dict(part=part.cpu().numpy(), pm=pm.cpu().numpy(), pv=pv.cpu().numpy())
            ref = R.partial_step(st, case["g_cls"][t], case["g_geo"][t], case["pidx"], case["periodical"], *pre, *args)
            for k, p in zip(("part", "pm", "pv"), pre):
                if ref.get(k) is None:      # optim -1 moves nothing but x; SGD leaves pv alone
                    assert got[k].tobytes() == p.tobytes(), (optim, k)
                else:
                    key = ("adam " if optim == 0 else "sgd ") + k
                    worst[key] = max(worst.get(key, 0.0), assert_result(got[k], ref[k], (optim, t, k)))
            want_x = np.full((B, 3, N), POISON, F)        # x[:, :, pidx] = fl32(periodical + part), nothing else
            np.put_along_axis(want_x, idx, (np.take_along_axis(case["periodical"], idx, 2) + got["part"]).astype(F), 2)
            assert bits(x) == want_x.tobytes(), (optim, t)
    print("partial", B, N, kr, " ".join("%s %.3f" % kv for kv in worst.items()))


# ----------------------------------------------------------------------------------------------------------------------
# binary update, begin
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("targeted", (0, 1))
def test_binary_update_bit_for_bit(lib, targeted):
    """B = 300: a second workgroup of 44 threads.  One update of the cross product, then three chained ones."""
    st = R.binary_case(targeted)
    dv = DevState(st)
    for i in range(4):
        st = R.binary_update(st)
        assert lib.geoa3_attack_binary_update(dv.ref, stream()) == 0
        snap = dv.snapshot()
        for k in INT_KEYS + COPY_KEYS:
            got = snap[k][:-1] if k == "best_attack" else snap[k]
            assert_result(got, st[k], (i, k))


@pytest.mark.parametrize("B,N", ((1, 1), (3, 77), (7, 300)))       # (1, 1): 3 B N = 3 < 256 threads reset B rows too
@pytest.mark.parametrize("adam", (False, True))
def test_begin_search_step_bit_for_bit(lib, B, N, adam):
    rng = np.random.default_rng(B + N)
    st = R.new_state(B, N, 40, 0, R.CE, 0.0, 1.0 / B, np.zeros(B), np.zeros(B), np.ones(B))
    st["iter_best_loss"][:] = 3.0
    st["iter_best_score"][:] = 4
    st["prev_constrain"][:] = 0.5
    st["best_loss"][:] = 2.0
    st["best_step"][:] = 6
    ori, init = rng.standard_normal((B, 3, N)).astype(F), (1e-3 * rng.standard_normal((B, 3, N))).astype(F)
    dv = DevState(st)
    off, m, v, x = (torch.full((B, 3, N), POISON, device="cuda") for _ in range(4))
    assert lib.geoa3_attack_begin_search_step(dv.ref, ptr(cu(ori)), ptr(cu(init)), ptr(off), ptr(m) if adam else None,
                                              ptr(v) if adam else None, ptr(x), stream()) == 0
    want, out = R.begin_search_step(st, ori, init, adam)
    snap = dv.snapshot()
    for k in INT_KEYS + COPY_KEYS:
        assert_result(snap[k][:-1] if k == "best_attack" else snap[k], want[k], k)
    assert (want["best_loss"] == 2.0).all() and (want["iter_best_loss"] == R.BIG).all()
    assert bits(off) == init.tobytes() and bits(x) == out["x"].tobytes()
    poison = np.full((B, 3, N), POISON, F).tobytes()
    assert bits(m) == (out["m"].tobytes() if adam else poison) and bits(v) == (out["v"].tobytes() if adam else poison)


# ----------------------------------------------------------------------------------------------------------------------
# arguments
# ----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_return_einval_and_write_nothing(lib):
    """Every documented GEOA3_EINVAL condition of the nine entries, on poisoned buffers; the unmodified argument list of
    each entry is accepted afterwards, so the refusals are the substituted argument's."""
    B, N, Cn, E, kr = 3, 77, 10, 4, 3
    st = R.new_state(B, N, Cn, 1, R.CE, 0.0, 1.0 / B, np.zeros(B), np.ones(B), np.ones(B), hist_steps=2)
    dv = DevState(st)
    f = lambda *shape: torch.full(shape, POISON, device="cuda")
    buf = dict(logits=f(B, Cn), vote=f(B, E, Cn), con=f(B), x=f(B, 3, N), dl=f(B, Cn), ori=f(B, 3, N), off=f(B, 3, N),
               m=f(B, 3, N), v=f(B, 3, N), g=f(B, 3, N), nrm=f(B, 3, N), per=f(B, 3, N), part=f(B, 3, kr), pm=f(B, 3, kr),
               pv=f(B, 3, kr), ok=torch.ones(B, dtype=torch.int32, device="cuda"),
               nn=torch.zeros(B, N, dtype=torch.int32, device="cuda"),
               pidx=torch.arange(kr, dtype=torch.int32, device="cuda").repeat(B, 1).contiguous())
    p = {k: v.data_ptr() for k, v in buf.items()}
    s = stream()
    # entry -> (valid arguments, [(position, bad value), ...])
    table = {
        "geoa3_attack_head": ([dv.ref, p["logits"], p["con"], p["x"], 0, 0, p["dl"], s],
                              [(0, None), (1, None), (3, None), (6, None)]),
        "geoa3_attack_head_vote": ([dv.ref, p["logits"], p["vote"], E, p["con"], p["x"], 0, 0, p["dl"], s],
                                   [(0, None), (1, None), (5, None), (8, None), (3, 0), (3, 65), (3, -1)]),
        "geoa3_attack_head_classify": ([dv.ref, p["logits"], p["vote"], E, p["dl"], p["ok"], s],
                                       [(0, None), (1, None), (4, None), (5, None), (3, 0), (3, 65)]),
        "geoa3_attack_head_finish": ([dv.ref, p["ok"], p["con"], p["x"], 0, 0, s], [(0, None), (1, None), (3, None)]),
        "geoa3_attack_update": ([dv.ref, p["g"], p["g"], p["ori"], p["off"], p["m"], p["v"], p["x"], 0, 0.01, 1.0, 0.0, s],
                                [(0, None), (3, None), (4, None), (7, None), (5, None), (6, None)]),
        "geoa3_attack_partial_step": ([dv.ref, p["g"], p["g"], p["pidx"], kr, p["per"], p["part"], p["pm"], p["pv"],
                                       p["x"], 0, 0.01, 1.0, 0.9, 0, s],
                                      [(0, None), (3, None), (5, None), (6, None), (9, None), (4, 0), (10, 2), (10, -2),
                                       (7, None), (8, None)]),
        "geoa3_attack_project": ([1, p["ori"], p["nrm"], p["nn"], p["off"], p["x"], B, N, 0.01, s],
                                 [(1, None), (3, None), (4, None), (5, None), (6, 0), (7, 0), (0, 2), (0, -1), (2, None)]),
        "geoa3_attack_binary_update": ([dv.ref, s], [(0, None)]),
        "geoa3_attack_begin_search_step": ([dv.ref, p["ori"], p["ori"], p["off"], p["m"], p["v"], p["x"], s],
                                           [(0, None), (1, None), (2, None), (3, None), (6, None)]),
    }
    before_state = {k: None if v is None else v.tobytes() for k, v in dv.snapshot().items()}
    before = {k: bits(v) for k, v in buf.items()}
    for name, (args, bad) in table.items():
        fn = getattr(lib, name)
        for pos, val in bad:
            a = list(args)
            a[pos] = val
            assert fn(*a) == EINVAL, (name, pos, val)
    # SGD with momentum needs its buffer as well (optim 1 without pm)
    a = list(table["geoa3_attack_partial_step"][0])
    a[10], a[7] = 1, None
    assert lib.geoa3_attack_partial_step(*a) == EINVAL
    after_state = {k: None if v is None else v.tobytes() for k, v in dv.snapshot().items()}
    assert after_state == before_state and {k: bits(v) for k, v in buf.items()} == before, "a refused call wrote"
    # finite inputs for the accepted calls
    for k in ("logits", "vote", "con", "x", "ori", "off", "m", "v", "g", "nrm", "per", "part", "pm", "pv"):
        buf[k].fill_(0.5)
    for name, (args, _) in table.items():
        assert getattr(lib, name)(*args) == 0, name
    torch.cuda.synchronize()
