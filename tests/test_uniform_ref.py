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
