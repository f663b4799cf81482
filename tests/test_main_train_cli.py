"""CPU: main_train.py's flag set and defaults against the reference's (tests/golden/main_train_flags.json: the parsed flag
list, data only), its refusals, and geoa3_amd.data.augment_batch on CPU tensors."""
import ast
import json
import math
import os

import pytest
import torch

import main_train
from geoa3_amd.data import augment_batch

HERE = os.path.dirname(os.path.abspath(__file__))


def test_flag_set_and_defaults_match_reference():
    ref = json.load(open(os.path.join(HERE, "golden", "main_train_flags.json")))
    assert len(ref) == 17
    actions = {o: a for a in main_train.build_parser()._actions for o in a.option_strings}
    for names, default, store_true in ref:
        for n in names:
            assert n in actions, n
        act = actions[names[-1]]
        if store_true:
            assert act.default is False and act.nargs == 0
        else:
            want = ast.literal_eval(default)
            assert act.default == want and type(act.default) is type(want), (names, act.default, want)


@pytest.mark.parametrize("argv,word", [(["--arch", "PointNetPP"], "PointNetPP"), (["--arch", "DGCNN"], "DGCNN"),
                                       (["-g", "2"], "mGPU")])
def test_refusals_name_what_they_refuse(argv, word, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg = main_train.build_parser().parse_args(argv + ["--synthetic", "-c", "5"])
    with pytest.raises(NotImplementedError, match=word):
        main_train.main(cfg)
    assert not os.listdir(tmp_path)          # refused before anything is written


def test_tensorboard_is_imported_only_on_request():
    src = open(main_train.__file__).read()
    assert src.count("tensorboard") >= 1 and "\nfrom torch.utils.tensorboard" not in src and "\nimport tensorboard" not in src


def _run(seed, B=6, N=40):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, N, 3, generator=g)
    return x, augment_batch(x, torch.Generator().manual_seed(seed))


def test_augment_batch_same_seed_same_result_and_input_untouched():
    x, a = _run(3)
    x0 = x.clone()
    _, b = _run(3)
    _, c = _run(4)
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.equal(x, x0)
    assert a.shape == x.shape and a.dtype == x.dtype


def test_augment_batch_is_rotation_scale_shift_jitter_within_the_ranges():
    """Every output cloud is s R x_perm + t + jitter: fit the affine map per cloud by least squares (N >> 12 unknowns) and
    check R orthonormal with the up axis fixed up to the clipped perturbation, s in [0.8, 1.25], |t| <= 0.1, the residual
    (the jitter) within its clip, and the point order a permutation shared by the batch."""
    B, N = 5, 400
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, N, 3, generator=g).double()
    y = augment_batch(x, torch.Generator().manual_seed(5))
    # the shuffle: jitter <= 0.05 and the random points are far apart, so matching by the fitted map is unambiguous; recover
    # the permutation from cloud 0 and require it for all clouds
    perm = None
    for b in range(B):
        # solve y = [x 1] A for the best permutation: start from the nearest neighbour under a fit on sorted norms is
        # fragile; use the invariance of pairwise distances instead -- scale-normalised distance profiles
        dx = torch.cdist(x[b], x[b]).sort(1).values
        dy = torch.cdist(y[b], y[b]).sort(1).values
        s_est = (dy[:, 1:].mean() / dx[:, 1:].mean())
        match = torch.cdist(dy / s_est, dx).argmin(1)          # y point i  <-  x point match[i]
        assert match.unique().numel() == N
        perm = match if perm is None else perm
        assert torch.equal(match, perm)
        X1 = torch.cat([x[b][match], torch.ones(N, 1, dtype=x.dtype)], 1)
        A = torch.linalg.lstsq(X1, y[b]).solution                # [4,3]: rows 0..2 = s R (row vectors), row 3 = t
        sR, t = A[:3], A[3]
        s = sR.det().abs() ** (1.0 / 3.0)
        R = sR / s
        assert 0.8 - 0.01 <= float(s) <= 1.25 + 0.01
        assert float(t.abs().max()) <= 0.1 + 0.01
        assert torch.allclose(R @ R.t(), torch.eye(3, dtype=x.dtype), atol=0.02)
        assert float(R.det()) > 0
        # up axis (y): the big rotation keeps it; the perturbation moves it by at most its three clipped angles
        up = torch.tensor([0.0, 1.0, 0.0], dtype=x.dtype) @ R
        assert math.acos(min(1.0, float(up[1]))) <= 3 * 0.18 + 0.02
        resid = y[b] - X1 @ A
        assert float(resid.abs().max()) <= 0.05 + 0.01 and float(resid.std()) < 0.02
