"""CPU-only: the command line, the output directory and the binding of the displacement / repulsion / corresponding-normal
terms of the attack loop (--displacement_loss_weight, --repulsion_loss_weight, --corr_normal_loss_weight)."""
import ctypes as C
import os
import re

import main_attack
from geoa3_amd import _lib
from geoa3_amd.attack import RUNNER_CFG_FIELDS

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BASE = ["--attack", "GeoA3", "--attack_label", "Untarget"]
FIELDS = {"displacement_loss_weight": 0.0, "displacement_loss_knn": 16, "repulsion_loss_weight": 0.0,
          "repulsion_loss_knn": 4, "repulsion_loss_h": 0.03, "corr_normal_loss_weight": 0.0, "corr_normal_loss_knn": 2}


def test_flags_parse_with_the_reference_functions_defaults():
    cfg = main_attack.build_parser().parse_args(BASE)
    for name, default in FIELDS.items():
        assert getattr(cfg, name) == default and type(getattr(cfg, name)) is type(default), name
    cfg = main_attack.build_parser().parse_args(BASE + ["--displacement_loss_weight", "2", "--displacement_loss_knn", "8",
                                                        "--repulsion_loss_weight", "0.5", "--repulsion_loss_knn", "6",
                                                        "--repulsion_loss_h", "0.05", "--corr_normal_loss_weight", "1.5",
                                                        "--corr_normal_loss_knn", "3"])
    assert [getattr(cfg, n) for n in FIELDS] == [2.0, 8, 0.5, 6, 0.05, 1.5, 3]


def test_directory_name_is_unchanged_at_zero_weights():
    cfg = main_attack.build_parser().parse_args(BASE + ["--displacement_loss_knn", "8", "--repulsion_loss_h", "0.05"])
    name = main_attack.saved_dir_name(cfg)
    for field in FIELDS:                       # a namespace from before the flags existed names the same directory
        delattr(cfg, field)
    assert main_attack.saved_dir_name(cfg) == name
    assert not re.search(r"_Disp|_Rep|_CorrNor", name)


def test_directory_name_carries_the_suffixes_in_order():
    p = main_attack.build_parser()
    off = main_attack.saved_dir_name(p.parse_args(BASE + ["--is_use_knn_smoothing_loss"]))
    on = main_attack.saved_dir_name(p.parse_args(BASE + ["--is_use_knn_smoothing_loss", "--displacement_loss_weight", "2",
                                                         "--repulsion_loss_weight", "0.5", "--corr_normal_loss_weight",
                                                         "1.5", "--corr_normal_loss_knn", "3"]))
    assert off.endswith("_kNNSmooth5.0_k5_coef1.1")
    assert on == off + "_Disp2.0_k16_Rep0.5_k4_h0.03_CorrNor1.5_k3"
    one = main_attack.saved_dir_name(p.parse_args(BASE + ["--repulsion_loss_weight", "0.25", "--repulsion_loss_h", "0.1"]))
    assert one.endswith("_k16_Rep0.25_k4_h0.1")          # after the curvature term's own _k16


def test_binding_and_header_declare_the_fold():
    ret, args = _lib.SIGNATURES["geoa3_reg_fold_points"]
    vp = C.c_void_p
    assert ret is C.c_int and args == [vp, vp, C.c_float, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp]
    assert _lib.SIGNATURES["geoa3_corr_normal_loss_grad"] == _lib.SIGNATURES["geoa3_repulsion_loss_grad"][:1] + (
        [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp],)
    hdr = open(os.path.join(REPO, "include", "geoa3_hip.h")).read()
    assert ("int geoa3_reg_fold_points(const float* out, const float* grad, float w, int B, int N, float* term, "
            "float* constrain, int constrain_add, float* g, int g_add, void* stream);") in re.sub(r"\s+", " ", hdr)
    assert int(re.search(r"#define GEOA3_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 608


def test_runner_cache_key_holds_the_new_fields():
    assert set(FIELDS) | {"reg_share_table"} <= set(RUNNER_CFG_FIELDS)
