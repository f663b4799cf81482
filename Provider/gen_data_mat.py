#!/usr/bin/env python3
"""Write the instance `.mat` file main_attack.py reads -- the job of the reference's Provider/gen_data_mat.py, with its
flags and its output, from two sources:

    # the user's own shapes: ROOT/<class>/<split>/*.off|*.obj, sampled on their surfaces on the GPU (extension)
    python Provider/gen_data_mat.py --mesh_dir ModelNet40 --shape_names_file modelnet40_shape_names.txt \\
        --out_datadir Data --arch PointNet -outc 10 -outn 25 --npoint 1024 --dense_npoints 10000

    # the reference's own source: modelnet40_normal_resampled, rows x,y,z,nx,ny,nz (gen_data_mat.py:228-265)
    python Provider/gen_data_mat.py --datadir /data/modelnet40_normal_resampled --out_datadir Data --swap_yz

Both keep the instances the victim classifies correctly (:207-226), take torch.randperm(num)[:max_out_num] of every class
(:289) and write `modelnet<outc>_<M>instances<npoint>_<arch>.mat` with data [M,3,n] f32, normal [M,3,n] f32 and label
[M,1] (:304); the mesh source also writes the dense file (`..instances<dense_npoints>..`, :306) when --dense_npoints > 0.

The mesh path: every class's meshes in one ragged batch -> geoa3_amd.mesh.mesh_clouds (area-weighted surface samples
with the faces' own normals, then farthest-point sampling to --npoint and to --dense_npoints points, each normalised by
its own statistics, :195-197) -> the victim's forward on all clouds of the class at once.

Extensions: --mesh_dir / --split / --shape_names_file / --surface_samples; --swap_yz (the [0,2,1] permutation of :216 on
points and normals; the reference applies it always, :247-248); --seed; --synthetic (the seeded victim of main_attack.py
when no checkpoint exists); --keep_misclassified (a random-init victim keeps next to nothing otherwise).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
from scipy.io import savemat

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Point Cloud Attacking: the instance .mat file")
    p.add_argument("--datadir", default="/data/modelnet40_normal_resampled/", type=str, metavar="DIR",
                   help="modelnet40_normal_resampled (used when --mesh_dir is not given)")
    p.add_argument("--out_datadir", default="Data", type=str, metavar="DIR")
    p.add_argument("--arch", default="PointNet", type=str, metavar="ARCH")
    p.add_argument("-c", "--classes", default=40, type=int, metavar="N", help="num of classes (default: 40)")
    p.add_argument("-outc", "--out_classes", default=10, type=int, metavar="N",
                   help="10: the ten ModelNet10 classes by name; otherwise every class of the names file")
    p.add_argument("-outn", "--max_out_num", default=25, type=int, metavar="N", help="instances kept per class")
    p.add_argument("--pre_trn_npoint", default=1024, type=int, metavar="N")
    p.add_argument("--npoint", default=1024, type=int, metavar="N")
    p.add_argument("--dense_npoints", default=10000, type=int, metavar="N")
    # ------------ extensions
    p.add_argument("--mesh_dir", default=None, type=str, metavar="ROOT",
                   help="read triangle meshes ROOT/<class>/<split>/*.off|*.obj instead of --datadir")
    p.add_argument("--split", default="test", type=str)
    p.add_argument("--shape_names_file", default=None, type=str,
                   help="one class name per line, the line number is the label (required with --mesh_dir; default for "
                        "--datadir: <datadir>/modelnet40_shape_names.txt)")
    p.add_argument("--surface_samples", default=16384, type=int,
                   help="surface points drawn per mesh before the farthest-point sampling (at most 16384)")
    p.add_argument("--swap_yz", action="store_true", default=False, help="permute the axes [0,2,1] (gen_data_mat.py:216)")
    p.add_argument("--seed", default=None, type=int, help="seed of every draw (default: unseeded)")
    p.add_argument("--synthetic", action="store_true", default=False,
                   help="seeded random-init victim when Pretrained/<arch>/<pre_trn_npoint>/model_best.pth.tar is missing")
    p.add_argument("--keep_misclassified", action="store_true", default=False,
                   help="keep the instances the victim gets wrong too")
    return p


def load_victim(cfg, device):
    """The victim of --arch with its checkpoint (gen_data_mat.py:163-177), or main_attack.py's seeded stand-in under
    --synthetic."""
    import main_attack
    from geoa3_amd.data import synthetic_state_dict
    if cfg.arch not in main_attack.ARCHS:
        raise AssertionError("Not support such arch.")
    vcfg = argparse.Namespace(arch=cfg.arch, classes=cfg.classes, npoint=cfg.pre_trn_npoint)
    model_path = os.path.join("Pretrained", cfg.arch, str(cfg.pre_trn_npoint), "model_best.pth.tar")
    net = main_attack.make_victim(vcfg)
    if os.path.isfile(model_path):
        main_attack.load_checkpoint(net, vcfg, model_path)
        print("Successfully load pretrained-model from {}".format(model_path))
    elif not cfg.synthetic:
        raise FileNotFoundError(model_path)
    elif cfg.arch == "PointNet":
        net.load_state_dict(synthetic_state_dict(cfg.classes, seed=0, device=device))
    elif cfg.arch == "PointNetPP":
        with torch.no_grad():
            for mod in net.modules():
                if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                    mod.running_mean.normal_(0, 0.1)
                    mod.running_var.uniform_(0.5, 1.5)
    return net.to(device).eval()


def read_shape_names(path):
    with open(path) as fp:
        names = [ln.strip() for ln in fp if ln.strip()]
    if len(set(names)) != len(names):
        raise ValueError("%s names a class twice" % path)
    return names


def selected_classes(cfg, names):
    """[(class name, label)] in output order: the ten ModelNet10 names for -outc 10 (gen_data_mat.py:44-45,62-64), every
    class of the names file otherwise (:65-67)."""
    from geoa3_amd.data import TEN_LABEL_NAMES
    if cfg.out_classes == 10:
        return [(n, names.index(n)) for n in TEN_LABEL_NAMES if n in names]
    if cfg.out_classes != len(names):
        raise ValueError("-outc must be 10 or the number of classes the names file lists (%d)" % len(names))
    return [(n, i) for i, n in enumerate(names)]


def _swap(t):
    return t[:, [0, 2, 1], :].contiguous()


def mesh_files(mesh_dir, name, split):
    """(folder ROOT/<name>/<split>, its *.off / *.obj files, sorted); no files when the folder is missing"""
    from geoa3_amd import mesh
    folder = os.path.join(mesh_dir, name, split)
    files = sorted(f for f in os.listdir(folder) if os.path.splitext(f)[1].lower() in mesh.READERS) \
        if os.path.isdir(folder) else []
    return folder, files


def mesh_class_clouds(cfg, name, device):
    """Every mesh of ROOT/<name>/<split> -> (points [n,3,npoint], normals, dense points or None, dense normals or None).
    A mesh without any area is left out."""
    from geoa3_amd import mesh
    folder, files = mesh_files(cfg.mesh_dir, name, cfg.split)
    if not files:
        return None
    meshes = [mesh.READERS[os.path.splitext(f)[1].lower()](os.path.join(folder, f)) for f in files]
    (pts, nrm), dense, bad = mesh.mesh_clouds(mesh.pack_meshes(meshes, device), cfg.npoint, cfg.dense_npoints,
                                              cfg.surface_samples, return_bad_faces=True)
    for f, nb in zip(files, bad.tolist()):
        if nb:
            print("{}: {} bad faces (an index outside the vertices or a non-finite area) left out".format(
                os.path.join(folder, f), nb))
    keep = torch.isfinite(pts).all(2).all(1)
    for f, k in zip(files, keep.tolist()):
        if not k:
            print("{}: no face with an area, left out".format(os.path.join(folder, f)))
    dpts, dnrm = (dense[0][keep], dense[1][keep]) if dense is not None else (None, None)
    return pts[keep], nrm[keep], dpts, dnrm


def datadir_class_clouds(cfg, name, device):
    """The reference's source (gen_data_mat.py:228-248 with Provider/modelnet_trn_test.py:79-83): the first npoint rows
    x,y,z,nx,ny,nz of every <datadir>/<name>/<id>.txt the split file lists, points normalised on the GPU."""
    from geoa3_amd import utility as U
    with open(os.path.join(cfg.datadir, "modelnet40_%s.txt" % cfg.split)) as fp:
        ids = [ln.strip() for ln in fp if ln.strip()]
    ids = [i for i in ids if "_".join(i.split("_")[:-1]) == name]
    if not ids:
        return None
    rows = np.stack([np.loadtxt(os.path.join(cfg.datadir, name, i + ".txt"), delimiter=",", dtype=np.float32)[:cfg.npoint]
                     for i in ids])
    both = torch.from_numpy(rows).to(device).permute(0, 2, 1).contiguous()
    return U.normalize_cloud(both[:, :3].contiguous()), both[:, 3:6].contiguous(), None, None


def main(cfg):
    if not torch.cuda.is_available():
        raise RuntimeError("gen_data_mat.py samples, re-samples and classifies on the GPU, and none is present")
    device = torch.device("cuda")
    if cfg.seed is not None:
        np.random.seed(cfg.seed)
        torch.manual_seed(cfg.seed)
        torch.cuda.manual_seed_all(cfg.seed)
    from_meshes = cfg.mesh_dir is not None
    if from_meshes and not cfg.shape_names_file:
        raise ValueError("--mesh_dir needs --shape_names_file (one class name per line, the line number is the label)")
    names = read_shape_names(cfg.shape_names_file or os.path.join(cfg.datadir, "modelnet40_shape_names.txt"))
    if len(names) > cfg.classes:
        raise ValueError("the names file lists %d classes, the victim has %d (-c)" % (len(names), cfg.classes))
    net = load_victim(cfg, device)
    class_clouds = mesh_class_clouds if from_meshes else datadir_class_clouds

    data, normal, dense_data, dense_normal, label = [], [], [], [], []
    for name, lab in selected_classes(cfg, names):
        got = class_clouds(cfg, name, device)
        if got is None or got[0].shape[0] == 0:
            print("{0}: 0".format(name))
            continue
        pts, nrm, dpts, dnrm = got
        if cfg.swap_yz:
            pts, nrm = _swap(pts), _swap(nrm)
            if dpts is not None:
                dpts, dnrm = _swap(dpts), _swap(dnrm)
        with torch.no_grad():
            pred = net(pts).argmax(1)
        right = pred == lab
        print("{0}: {1} instances, {2} classified correctly".format(name, pts.shape[0], int(right.sum())))
        sel = torch.arange(pts.shape[0], device=device) if cfg.keep_misclassified else right.nonzero().view(-1)
        sel = sel[torch.randperm(sel.numel())[:cfg.max_out_num].to(device)]           # gen_data_mat.py:289
        data.append(pts[sel].cpu())
        normal.append(nrm[sel].cpu())
        if dpts is not None:
            dense_data.append(dpts[sel].cpu())
            dense_normal.append(dnrm[sel].cpu())
        label.append(torch.full((sel.numel(), 1), lab, dtype=torch.int64))
    if not data or sum(d.shape[0] for d in data) == 0:
        raise RuntimeError("no instance was kept: nothing to write")

    os.makedirs(cfg.out_datadir, exist_ok=True)
    label = torch.cat(label).numpy()
    written = []

    def write(points, normals, n):
        points, normals = torch.cat(points).numpy(), torch.cat(normals).numpy()
        path = os.path.join(cfg.out_datadir, "modelnet{0}_{1}instances{2}_{3}.mat".format(cfg.out_classes, points.shape[0],
                                                                                         n, cfg.arch))
        savemat(path, {"data": points, "normal": normals, "label": label})
        written.append(path)

    write(data, normal, cfg.npoint)
    if dense_data:
        write(dense_data, dense_normal, cfg.dense_npoints)
    return written


if __name__ == "__main__":
    for out in main(build_parser().parse_args()):
        print(out)
