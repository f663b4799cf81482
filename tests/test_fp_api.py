"""CPU-only: the public surface of the feature-propagation operators -- the C ABI declares them, the ctypes mirror holds them,
`geoa3_amd.pointnet2.ext` has all nine names of the reference's `_ext` (bindings.cpp:6-19), PointnetFPModule keeps the
reference's parameter names, and CPU tensors are refused as the reference refuses them."""
import os
import re

import numpy as np
import pytest
import torch

from geoa3_amd import _lib

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_ENTRIES = ["geoa3_pn2_three_nn", "geoa3_pn2_three_nn_ex", "geoa3_pn2_three_interpolate", "geoa3_pn2_three_interpolate_ex",
               "geoa3_pn2_three_interpolate_grad", "geoa3_pn2_three_interpolate_scratch_bytes"]
# Model/pointnet2_ops_lib/pointnet2_ops/_ext-src/src/bindings.cpp:6-19
EXT_NAMES = ["gather_points", "gather_points_grad", "furthest_point_sampling", "three_nn", "three_interpolate",
             "three_interpolate_grad", "ball_query", "group_points", "group_points_grad"]


def test_header_and_signatures_hold_the_new_entries():
    hdr = open(os.path.join(REPO, "include", "geoa3_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
    assert "out of scope" not in hdr


def test_ext_has_all_nine_names():
    from geoa3_amd import pointnet2 as P
    for name in EXT_NAMES:
        assert callable(getattr(P.ext, name)), name
    for name in ("three_nn", "three_interpolate", "PointnetFPModule"):
        assert hasattr(P, name), name


def test_fp_module_keeps_the_reference_names():
    from geoa3_amd import pointnet2 as P
    gf = np.load(os.path.join(REPO, "tests", "golden", "geoa3_golden_fp.npz"), allow_pickle=False)
    c_in = gf["fp/gauss/known_feats"].shape[1] + gf["fp/gauss/unknow_feats"].shape[1]
    mod = P.PointnetFPModule([c_in, 64, 32])
    assert list(mod.state_dict().keys()) == list(gf["fp/gauss/sd_names"])
    mod.load_state_dict({k: torch.from_numpy(gf["fp/gauss/sd/" + k]) for k in gf["fp/gauss/sd_names"]})
    assert list(P.PointnetFPModule([4, 8], bn=False).state_dict().keys()) == ["mlp.0.weight", "mlp.0.bias"]


def test_cpu_tensors_are_refused():
    from geoa3_amd import pointnet2 as P
    x, k = torch.zeros(1, 4, 3), torch.zeros(1, 5, 3)
    idx, w = torch.zeros(1, 4, 3, dtype=torch.int32), torch.zeros(1, 4, 3)
    with pytest.raises(_lib.Geoa3Error, match="CPU not supported"):
        P.ext.three_nn(x, k)
    with pytest.raises(_lib.Geoa3Error, match="CPU not supported"):
        P.ext.three_interpolate(torch.zeros(1, 2, 5), idx, w)
    with pytest.raises(_lib.Geoa3Error, match="CPU not supported"):
        P.ext.three_interpolate_grad(torch.zeros(1, 2, 4), idx, w, 5)
    with pytest.raises(_lib.Geoa3Error, match="CPU not supported"):
        P.three_nn(x, k)
    with pytest.raises(_lib.Geoa3Error, match="CPU not supported"):
        P.PointnetFPModule([2, 4])(x, k, None, torch.zeros(1, 2, 5))
