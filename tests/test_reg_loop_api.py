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
    assert int(re.search(r"#define GEOA3_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION == 609


def _plan(use_curv=True, k=8, disp=None, rep=None, cn=None, ks=None, **share):
    """knn_table_plan with a term on where its k is given"""
    from geoa3_amd.attack import knn_table_plan
    w = lambda x: 0.0 if x is None else 1.0
    return knn_table_plan(use_curv, k, w(disp), disp or 16, w(rep), rep or 4, w(cn), cn or 2, w(ks), ks or 5, **share)


def test_table_plan_of_the_loop_tests():
    """The sharing flags, column counts and searches per iteration that tests/test_gpu_reg_loop.py asserts on a runner
    (sections 5 and 2), from the plan alone."""
    curv = ("curv", 9)
    # 5: shared tables, the same with reg_share_table = False, and terms wider than the curvature table
    assert _plan(disp=8, rep=4, cn=2) == ({"disp": curv, "rep": curv, "cn": curv}, 1)
    assert _plan(disp=8, rep=4, cn=2, reg_share_table=False) == ({"disp": curv, "rep": ("reg", 5), "cn": ("reg", 5)}, 2)
    assert _plan(disp=12, rep=12, cn=3, ks=5) == ({"knn": curv, "disp": ("clean", 13), "rep": ("reg", 13),
                                                   "cn": ("reg", 13)}, 2)
    # 2: every weight zero, whatever the k's and switches say
    from geoa3_amd.attack import knn_table_plan
    assert knn_table_plan(True, 4, 0.0, 8, 0.0, 6, 0.0, 3, 0.0, 5, True, False) == ({}, 1)


def test_table_plan_without_the_curvature_table():
    # no curvature term, every term on: the smoothing term's own search plus ONE for repulsion and normal
    assert _plan(use_curv=False, k=16, disp=16, rep=4, cn=2, ks=5) == (
        {"knn": ("own", 6), "disp": ("clean", 17), "rep": ("reg", 5), "cn": ("reg", 5)}, 2)
    assert _plan(use_curv=False, rep=4) == ({"rep": ("reg", 5)}, 1) and _plan(use_curv=False, cn=3) == ({"cn": ("reg", 4)}, 1)
    # the smoothing term refused the curvature table, or wider than it
    assert _plan(ks=5, rep=4, knn_share_table=False) == ({"knn": ("own", 6), "rep": ("curv", 9)}, 2)
    assert _plan(ks=9) == ({"knn": ("own", 10)}, 2) and _plan(ks=8) == ({"knn": ("curv", 9)}, 1)


def test_runner_cache_key_holds_the_new_fields():
    assert set(FIELDS) | {"reg_share_table"} <= set(RUNNER_CFG_FIELDS)
