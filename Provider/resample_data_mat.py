#!/usr/bin/env python3
"""Re-sample a `.mat` data file to fewer points per instance on the GPU: the job of the reference's
Provider/gen_data_mat_sample_from10000.py (10000 -> 5000 points, a numpy loop per instance with edited constants) as
one batched call with a command line.

    python Provider/resample_data_mat.py --data_mat_file Data/modelnet10_250instances10000_PointNet.mat \\
        --out_file Data/modelnet10_250instances5000_PointNet.mat --resample_num 5000

Every instance is farthest-point sampled (first index: np.random.randint per instance, in file order), centred on the
mean of the selected points and scaled to unit largest norm; the normals are gathered at the same indices.  A file
without `normal` gets PCA normals with --estimate_normal_knn K, estimated on the full cloud first.  Writes the same
three arrays: data [M,3,n] f32, normal [M,3,n] f32, label as read.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
from scipy.io import loadmat, savemat

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="FPS re-sampling of a point-cloud .mat file")
    p.add_argument("--data_mat_file", required=True, type=str)
    p.add_argument("--out_file", required=True, type=str)
    p.add_argument("--resample_num", required=True, type=int)
    p.add_argument("--estimate_normal_knn", type=int, default=0,
                   help="> 0: estimate the normals of a file that holds none from this many neighbours")
    p.add_argument("--estimate_normal_orient", default="none", choices=["none", "outward"])
    p.add_argument("--seed", type=int, default=None, help="np.random.seed for the first indices (default: unseeded)")
    return p


def main(cfg) -> str:
    from geoa3_amd.data import prepare_clouds
    if not os.path.isfile(cfg.data_mat_file):
        raise AssertionError("No exists .mat file!")
    if cfg.resample_num <= 0:
        raise ValueError("--resample_num must be positive")
    if cfg.seed is not None:
        np.random.seed(cfg.seed)
    orient = None if cfg.estimate_normal_orient == "none" else cfg.estimate_normal_orient
    data, normal, label = prepare_clouds(loadmat(cfg.data_mat_file), cfg.resample_num, cfg.estimate_normal_knn, orient,
                                         what=cfg.data_mat_file)
    os.makedirs(os.path.dirname(os.path.abspath(cfg.out_file)), exist_ok=True)
    savemat(cfg.out_file, {"data": data.numpy(), "normal": normal.numpy(), "label": label})
    return cfg.out_file


if __name__ == "__main__":
    print(main(build_parser().parse_args()))
