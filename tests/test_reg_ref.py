"""CPU: the float64 restatement of the neighbour-based regularisers (tests/_reg_ref.py) against the reference's own
values and gradients stored in tests/golden/geoa3_golden_reg.npz (tests/golden/make_golden_reg.py)."""
import os

import numpy as np
import pytest
import torch

from tests import _reg_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ["kNN_smoothing_loss", "repulsion_loss", "displacement_loss", "corresponding_normal_loss"]


@pytest.fixture(scope="module")
def gr():
    return np.load(os.path.join(REPO, "tests", "golden", "geoa3_golden_reg.npz"), allow_pickle=False)


def load_case(gr, fname, tag, dtype=torch.float64):
    """-> (x, rest (the other tensor arguments), kwargs, prefix)"""
    x, ori, nrm = (torch.from_numpy(gr["cloud/%s/%s" % (tag, n)]).to(dtype) for n in ("x", "ori", "nrm"))
    pre = "%s/%s/" % (fname, tag)
    kw = {str(n): (int(v) if str(n) == "k" else float(v)) for n, v in zip(gr[pre + "kw_names"], gr[pre + "kw_values"])}
    rest = {"displacement_loss": (ori,), "corresponding_normal_loss": (nrm,)}.get(fname, ())
    return x, rest, kw, pre


def all_cases(gr):
    return [(f, str(t)) for f in NAMES for t in gr["%s/cases" % f]]


def test_fixture_lists_the_four_functions(gr):
    assert [str(n) for n in gr["api/names"]] == NAMES
    tags = {f: [str(t) for t in gr["%s/cases" % f]] for f in NAMES}
    for f in NAMES:   # N = 64, 256, 1024, one non-multiple of 64
        assert {"n64", "n200", "n256", "n1024"} <= set(tags[f])
    assert "dup256" in tags["kNN_smoothing_loss"] and "dup256" in tags["repulsion_loss"]


def test_float64_restatement_matches_the_reference(gr):
    for fname, tag in all_cases(gr):
        x, rest, kw, pre = load_case(gr, fname, tag)
        val, grad = R.value_and_grad(getattr(R, fname), x, torch.from_numpy(gr[pre + "g"]), *rest, **kw)
        v64, g64 = torch.from_numpy(gr[pre + "value64"]), torch.from_numpy(gr[pre + "grad64"])
        assert val.shape == v64.shape and grad.shape == g64.shape
        assert (val - v64).abs().max() <= 1e-12 * v64.abs().max(), (fname, tag)
        assert (grad - g64).abs().max() <= 1e-12 * g64.abs().max(), (fname, tag)


def test_float32_restatement_within_the_reference_error(gr):
    """The same restatement in float32 lands within a few e_ref of the float64 result: e_ref is the scale of float32
    rounding for these functions, which is what the GPU tests take their bound from."""
    for fname, tag in all_cases(gr):
        x, rest, kw, pre = load_case(gr, fname, tag, torch.float32)
        val, grad = R.value_and_grad(getattr(R, fname), x, torch.from_numpy(gr[pre + "g"]), *rest, **kw)
        for got, key in ((val, "value"), (grad, "grad")):
            ref = torch.from_numpy(gr[pre + key + "64"])
            floor = float(np.finfo(np.float32).eps) * float(ref.abs().max())
            assert (got.double() - ref).abs().max() <= 4 * max(float(gr[pre + "e_ref_" + key]), floor), (fname, tag, key)


def test_mask_and_indices_of_the_restatement(gr):
    for fname, tag in all_cases(gr):
        x, rest, kw, pre = load_case(gr, fname, tag, torch.float32)
        k = kw.get("k", {"repulsion_loss": 4, "displacement_loss": 16, "corresponding_normal_loss": 2}.get(fname))
        cloud = rest[0] if fname == "displacement_loss" else x
        idx = R.knn_self(cloud, k + 1)[1][:, :, 1:]
        assert np.array_equal(idx.numpy(), gr[pre + "knn_idx"].astype(np.int64)), (fname, tag)
        if fname == "kNN_smoothing_loss":
            for dt in (torch.float32, torch.float64):
                c = R.smoothing_parts(x.to(dt), k, kw.get("threshold_coef", 1.05))[2]
                assert np.array_equal(c.numpy().astype(np.uint8), gr[pre + "cond"]), (tag, dt)
