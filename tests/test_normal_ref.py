"""CPU: the float64 restatements of tests/_normal_ref.py on inputs whose answer is known, and the input side's
plumbing that needs no GPU (the dataset's refusal of a file without normals, parser defaults, directory suffixes)."""
import os

import numpy as np
import pytest
import torch
from scipy.io import savemat

from tests import _normal_ref as R

BASE = ["--attack", "GeoA3", "--attack_label", "Untarget"]


def test_plane_with_in_plane_jitter_gives_the_plane_normal():
    g = np.random.default_rng(0)
    xs, ys = np.meshgrid(np.arange(12.0), np.arange(12.0))
    xy = np.stack([xs.ravel(), ys.ravel()]) * 0.125 + g.uniform(-0.03, 0.03, (2, 144))
    pc = np.concatenate([xy, np.full((1, 144), 0.375)])              # the plane z = 3/8, exactly
    n, w = R.estimate_normal(pc, R.knn_table(pc, 9))
    assert np.abs(w[:, 0]).max() < 1e-30                             # no spread along z at all
    np.testing.assert_allclose(n, np.tile([[0.0], [0.0], [1.0]], (1, 144)), atol=1e-12)
    # tilted: rotate the plane, the normal follows (canonical sign: largest component positive)
    c, s = np.cos(0.7), np.sin(0.7)
    rot = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    nt, _ = R.estimate_normal(rot @ pc, R.knn_table(rot @ pc, 9))
    np.testing.assert_allclose(nt, np.tile((rot @ [0.0, 0.0, 1.0])[:, None], (1, 144)), atol=1e-12)


def test_sphere_gives_the_radial_direction_outward():
    m = 1500                                                          # Fibonacci lattice: near-uniform on the unit sphere
    i = np.arange(m) + 0.5
    z = 1 - 2 * i / m
    phi = i * np.pi * (3 - np.sqrt(5))
    r = np.sqrt(1 - z * z)
    pc = np.stack([r * np.cos(phi), r * np.sin(phi), z]) + np.array([[0.01], [-0.02], [0.015]])
    idx = R.knn_table(pc, 13)
    n, _ = R.estimate_normal(pc, idx, "outward")
    radial = pc - pc.mean(axis=1, keepdims=True)
    radial /= np.linalg.norm(radial, axis=0)
    cos = (n * radial).sum(axis=0)
    assert cos.min() > 0.999, cos.min()                               # outward at every point, and radial
    n0, _ = R.estimate_normal(pc, idx)
    assert np.array_equal(np.abs(n0), np.abs(n))                      # the orientation changes the sign only
    lead = np.take_along_axis(n0, np.abs(n0).argmax(axis=0)[None], axis=0)
    assert (lead > 0).all() and (np.sign((n0 * n).sum(0)) == np.sign((n0 * radial).sum(0))).all()
    np.testing.assert_allclose(np.linalg.norm(n, axis=0), 1.0, atol=1e-12)


def test_normalisation_of_a_hand_computed_cloud():
    pts = np.array([[0.0, 4.0, 0.0, 0.0], [0.0, 0.0, 4.0, 0.0], [0.0, 0.0, 0.0, 4.0]])   # mean (1,1,1)
    out, mean, scale = R.normalize_cloud(pts)
    assert np.array_equal(mean, [1.0, 1.0, 1.0]) and scale == np.sqrt(11.0)             # |(3,-1,-1)| = sqrt(11)
    want = np.array([[-1.0, 3.0, -1.0, -1.0], [-1.0, -1.0, 3.0, -1.0], [-1.0, -1.0, -1.0, 3.0]]) / np.sqrt(11.0)
    np.testing.assert_allclose(out, want, atol=1e-15)
    assert abs(np.linalg.norm(out, axis=0).max() - 1.0) < 1e-15 and np.abs(out.mean(axis=1)).max() < 1e-16


def _mat_without_normal(path, M=4, N=32):
    from geoa3_amd.data import synthetic_clouds
    data, normal = synthetic_clouds(M, N, seed=3)
    savemat(str(path), {"data": data.numpy(), "label": np.full((M, 1), 17, dtype=np.int64)})
    return data, normal


def test_file_without_normals_is_refused_with_the_flag_named(tmp_path):
    from geoa3_amd._lib import Geoa3Error
    from geoa3_amd.data import ModelNet40
    path = tmp_path / "bare.mat"
    _mat_without_normal(path)
    with pytest.raises(Geoa3Error, match="estimate_normal_knn"):
        ModelNet40(data_mat_file=str(path), attack_label="Untarget")
    with pytest.raises(Geoa3Error, match="estimate_normal_knn"):
        ModelNet40(data_mat_file=str(path), attack_label="Untarget", resample_num=16, estimate_normal_knn=0)


def test_resampling_without_a_gpu_says_so(tmp_path, monkeypatch):
    from geoa3_amd._lib import Geoa3Error
    from geoa3_amd.data import ModelNet40, write_synthetic_mat
    path = write_synthetic_mat(str(tmp_path / "full.mat"), [17, 9], 32, seed=1)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(Geoa3Error, match="GPU"):
        ModelNet40(data_mat_file=path, attack_label="Untarget", resample_num=16)
    ds = ModelNet40(data_mat_file=path, attack_label="Untarget", estimate_normal_knn=8)   # the file's normals: no GPU needed
    assert ds.normal.shape == (2, 3, 32)


def test_utility_rejects_cpu_tensors():
    from geoa3_amd import utility as U
    from geoa3_amd._lib import Geoa3Error
    pc = torch.zeros(1, 3, 8)
    for call in (lambda: U.estimate_normal(pc, 3), lambda: U.farthest_points_normal_sample(pc, pc, 4),
                 lambda: U.farthest_points_normalized(pc, pc, 4), lambda: U.normalize_cloud(pc)):
        with pytest.raises(Geoa3Error):
            call()
    with pytest.raises(ValueError):
        U.estimate_normal(pc, 3, orient="inward")


def test_parser_defaults_leave_the_input_untouched():
    import main_attack
    cfg = main_attack.build_parser().parse_args(BASE)
    assert cfg.resample_num == -1 and cfg.estimate_normal_knn == 0 and cfg.estimate_normal_orient == "none"
    with pytest.raises(SystemExit):
        main_attack.build_parser().parse_args(BASE + ["--estimate_normal_orient", "inward"])


def test_directory_suffixes_of_the_input_flags():
    import main_attack
    p = main_attack.build_parser()
    base = main_attack.saved_dir_name(p.parse_args(BASE))
    assert "Resample" not in base and "EstNormal" not in base and base.endswith("_CurLoss1.0_k16")
    assert main_attack.saved_dir_name(p.parse_args(BASE + ["--resample_num", "512"])) == base + "_Resample512"
    assert main_attack.saved_dir_name(p.parse_args(BASE + ["--estimate_normal_knn", "8"])) == base + "_EstNormal_k8"
    assert main_attack.saved_dir_name(p.parse_args(BASE + ["--estimate_normal_knn", "8", "--estimate_normal_orient",
                                                           "outward"])) == base + "_EstNormal_k8_outward"
    # the orientation alone estimates nothing and names nothing; all three come after every other optional suffix
    assert main_attack.saved_dir_name(p.parse_args(BASE + ["--estimate_normal_orient", "outward"])) == base
    full = main_attack.saved_dir_name(p.parse_args(BASE + ["--is_pro_grad", "--corr_normal_loss_weight", "0.5",
                                                           "--resample_num", "64", "--estimate_normal_knn", "12",
                                                           "--estimate_normal_orient", "outward"]))
    assert full.endswith("_ProGrad_CorrNor0.5_k2_Resample64_EstNormal_k12_outward")


def test_binding_and_header_declare_the_two_entries():
    import ctypes as C
    import re
    from geoa3_amd import _lib
    vp = C.c_void_p
    assert _lib.SIGNATURES["geoa3_estimate_normal"] == (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp])
    assert _lib.SIGNATURES["geoa3_normalize_cloud"] == (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp])
    hdr = re.sub(r"\s+", " ", open(os.path.join(os.path.dirname(__file__), "..", "include", "geoa3_hip.h")).read())
    assert ("int geoa3_estimate_normal(const float* pc, const int32_t* knn_idx, int B, int N, int K1, int orient, "
            "float* normal_out, void* stream);") in hdr
    assert ("int geoa3_normalize_cloud(const float* pts, float* out, int B, int M, float* centroid_out, "
            "float* scale_out, void* stream);") in hdr
