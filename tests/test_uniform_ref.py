"""CPU: the float64 restatement of uniform_loss (tests/_uniform_ref.py) against the reference's own values, gradients and
indices stored in tests/golden/geoa3_golden_uniform.npz (tests/golden/make_golden_uniform.py)."""
import os

import numpy as np
import pytest
import torch

from tests import _uniform_ref as R

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = ["n188", "n256", "n1024", "n2048", "dupzero", "custom", "bn3"]


@pytest.fixture(scope="module")
def gu():
    return np.load(os.path.join(REPO, "tests", "golden", "geoa3_golden_uniform.npz"), allow_pickle=False)


def case(gu, tag):
    pre = "uni/%s/" % tag
    x = torch.from_numpy(gu[pre + "x"])
    bn3 = tag == "bn3"
    planar = x.permute(0, 2, 1).contiguous() if bn3 else x
    pcts = [float(p) for p in gu[pre + "percentages"]]
    return pre, planar, bn3, pcts, float(gu[pre + "radius"]), int(gu[pre + "k"])


def test_fixture_cases_listed(gu):
    assert list(gu["uni/cases"]) == CASES
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "geoa3_golden_uniform.npz")) < 1 << 20


@pytest.mark.parametrize("tag", CASES)
def test_restatement_matches_reference(gu, tag):
    pre, x, bn3, pcts, radius, k = case(gu, tag)
    fps, rows = R.indices(x, pcts, radius)
    assert np.array_equal(fps.numpy(), gu[pre + "fps"])
    for i, r in enumerate(rows):
        assert np.array_equal(r.numpy(), gu[pre + "bq%d" % i]), i
    loss, g = R.uniform_ref(x, pcts, radius, k, idx=(fps, rows))
    np.testing.assert_allclose(float(loss), float(gu[pre + "loss"]), rtol=1e-5)
    ref_g = gu[pre + "grad"]
    g = g.permute(0, 2, 1).numpy() if bn3 else g.numpy()
    assert np.abs(g - ref_g).max() <= 1e-5 * np.abs(ref_g).max()


@pytest.mark.parametrize("tag", CASES)
def test_parts_match_restatement_and_reference(gu, tag):
    """uniform_ref_parts (pair by pair, with the counts a per-element bound needs) == uniform_ref to 1e-12, and the fixture."""
    pre, x, bn3, pcts, radius, k = case(gu, tag)
    idx = (torch.from_numpy(gu[pre + "fps"]).long(), [torch.from_numpy(gu[pre + "bq%d" % i]).long() for i in range(len(pcts))])
    loss, g = R.uniform_ref(x, pcts, radius, k, idx=idx)
    p = R.uniform_ref_parts(x, pcts, radius, k, idx=idx, cells=1 << 14)       # (several chunks)
    assert abs(float(p["loss"]) - float(loss)) <= 1e-12 * abs(float(loss))
    assert float((p["grad"] - g).abs().max()) <= 1e-12 * float(g.abs().max())
    np.testing.assert_allclose(float(p["loss"]), float(gu[pre + "loss"]), rtol=1e-5)
    ref_g = gu[pre + "grad"]
    pg = p["grad"].permute(0, 2, 1).numpy() if bn3 else p["grad"].numpy()
    assert np.abs(pg - ref_g).max() <= 1e-5 * np.abs(ref_g).max()
    # A bounds the gradient (|u - e| <= u + e, |sum| <= sum | |); a point that receives nothing has a zero gradient
    assert (p["grad"].abs() <= p["A"] * (1 + 1e-12)).all()
    assert (p["grad"].permute(0, 2, 1)[p["n"] == 0] == 0).all() and (p["A"].permute(0, 2, 1)[p["n"] == 0] == 0).all()
    B, _, N = x.shape
    rows = B * int(N * 0.05) * sum(int(N * (q * 4)) for q in pcts)
    assert 0 < int(p["n"].sum()) <= 2 * k * rows and p["near"].shape[1] == 3


def test_parts_report_a_near_tie_and_ignore_copies():
    """Group of 4 slots, K = 2: the row's 2nd and 3rd nearest at squared distances 1 and (1 + 2^-23)^2 (relative gap 2^-22 < 8 * 2^-24) is
    a near-tie; the same gap between two slots of the same coordinates (a padded copy) is none."""
    N = 20
    x = torch.zeros(1, 3, N)
    x[0, 0, :] = torch.arange(N) * 10.0
    x[0, 0, 1], x[0, 0, 2], x[0, 1, 2] = 1.0, 0.0, 1.0 + 2.0 ** -23          # |p1 - p0| = 1, |p2 - p0| = 1 + 2^-23
    fps = torch.zeros(1, 1, dtype=torch.long)
    tie = R.uniform_ref_parts(x, (0.05,), 1.0, 1, idx=(fps, [torch.tensor([[[0, 1, 2, 5]]])]))
    assert [0, 0, 0] in tie["near"].tolist()
    none = R.uniform_ref_parts(x, (0.05,), 1.0, 1, idx=(fps, [torch.tensor([[[0, 1, 1, 5]]])]))
    assert [0, 0, 0] not in none["near"].tolist()
    # ... but a copy of the K-th slot between it and a close point of other coordinates is stepped over
    over = R.uniform_ref_parts(x, (0.05,), 1.0, 1, idx=(fps, [torch.tensor([[[0, 1, 1, 2]]])]))
    assert [0, 0, 0] in over["near"].tolist()
