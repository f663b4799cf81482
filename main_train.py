#!/usr/bin/env python3
"""Train the PointNet victim, or the DGCNN one -- the job of the reference's main_train.py, with its flags, defaults, loop and files:

    python main_train.py --datadir /data/modelnet40_normal_resampled --is_aug_data
    python main_train.py --mesh_dir ModelNet40 --shape_names_file modelnet40_shape_names.txt --is_aug_data
    python main_train.py --synthetic -c 5 --npoint 256 -b 16 --epochs 3
    python main_train.py --arch DGCNN --edge_train fused --datadir /data/modelnet40_normal_resampled --is_aug_data

Loop (main_train.py:188-347): label-smoothing loss at 0.2 + 0.001 ||T T^T - I||^2 / 2 on the feature transform, Adam with
per-parameter weight decay, lr 0.7^(epoch // 20) floored at 1e-5, the BatchNorm momentum schedule, the [0,2,1] axis swap of
:211, per-class and instance accuracy.  Files: Pretrained/<arch>/<npoint>/checkpoint.pth.tar and model_best.pth.tar (keys
epoch, state_dict, best_prec, class_prec, optimizer) and result.txt; --resume continues from a checkpoint.  main_attack.py,
defense.py and Provider/gen_data_mat.py load model_best.pth.tar unchanged.

The whole set lives on the GPU; batches are index selections, the augmentation (geoa3_amd.data.augment_batch) is batched
torch from a seeded generator.  --wide_train fused runs the three 1024-wide layers of a training step in the fused HIP
layer of geoa3_amd/pointnet_train.py (default: torch, the plain composition, the faster step at B 32: DESIGN.md 8d).

Extensions: --mesh_dir / --shape_names_file / --surface_samples (ROOT/<class>/train|test/*.off|*.obj through the reader and
surface sampler of Provider/gen_data_mat.py), --synthetic / --synthetic_instances (seeded CAD-like clouds, the label is
the kind: 5 classes), --wide_train, --quiet.

--arch DGCNN trains only together with --edge_train fused | torch (how a training step runs the four EdgeConv layers: the
fused HIP layer of geoa3_amd/dgcnn_train.py -- at B 32, N 1024 a step peaks at 0.95 GB against 5.3 GB and takes 11.2 against
32.4 ms: DESIGN.md 8e -- or the plain torch composition);
without it the arch is refused as before.  The loop is the one above with two differences: the loss is the smoothed-label
loss alone (DGCNN has no feature transform), and the BatchNorm momentum stays the module's own (--bn_momentum does not
apply).  --dgcnn_k, --emb_dims, --dropout are the public model's k, emb_dims and dropout.  Files: Pretrained/DGCNN/<npoint>/.
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import time

import numpy as np
import torch
import torch.nn as nn

BASE_DIR = os.path.dirname(os.path.abspath(__file__))
if BASE_DIR not in sys.path:
    sys.path.insert(0, BASE_DIR)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Point Cloud Training")
    # ------------ the reference's flags (main_train.py:33-56)
    p.add_argument("--id", default=0, type=int, help="0: --random_seed seeds every draw; otherwise the clock does")
    p.add_argument("--random_seed", default=0, type=int)
    p.add_argument("--datadir", default="/data/modelnet40_normal_resampled/", type=str, metavar="DIR", help="path to dataset")
    p.add_argument("-c", "--classes", default=40, type=int, metavar="N", help="num of classes (default: 40)")
    p.add_argument("--npoint", default=1024, type=int)
    p.add_argument("--is_aug_data", dest="is_aug_data", action="store_true", default=False)
    p.add_argument("--arch", default="PointNet", type=str, metavar="ARCH")
    p.add_argument("-g", "--mGPU", default=1, type=int, metavar="N", help="num of GPUs (default: 1)")
    p.add_argument("-j", "--num_workers", default=8, type=int, metavar="N", help="unused: the set lives on the GPU")
    p.add_argument("-b", "--batch_size", default=32, type=int, metavar="N", help="mini-batch size (default: 32)")
    p.add_argument("--epochs", default=250, type=int, metavar="N", help="number of total epochs to run")
    p.add_argument("--lr", default=0.001, type=float, metavar="LR", help="initial learning rate")
    p.add_argument("--decay-epochs", default=20, type=int, metavar="N", help="number of epochs to decay")
    p.add_argument("--bn_momentum", default=0.5, type=float, metavar="BN", help="initial bn momentum (PointNet; does not apply to DGCNN, whose BatchNorm momentum stays the module's own)")
    p.add_argument("--wd", default=0.0001, type=float, metavar="W", help="weight decay (default: 1e-4)")
    p.add_argument("--resume", default="", type=str, metavar="PATH", help="path to latest checkpoint (default: none)")
    p.add_argument("--is_use_tb", dest="is_use_tb", action="store_true", default=False, help="Using Tensorboard")
    # ------------ extensions
    p.add_argument("--mesh_dir", default=None, type=str, metavar="ROOT",
                   help="read triangle meshes ROOT/<class>/train|test/*.off|*.obj instead of --datadir")
    p.add_argument("--shape_names_file", default=None, type=str,
                   help="one class name per line, the line number is the label (required with --mesh_dir)")
    p.add_argument("--surface_samples", default=16384, type=int,
                   help="surface points drawn per mesh before the farthest-point sampling (at most 16384)")
    p.add_argument("--synthetic", action="store_true", default=False,
                   help="seeded CAD-like clouds instead of a data set; the label is the kind (5 classes)")
    p.add_argument("--synthetic_instances", default=160, type=int, help="training clouds under --synthetic (a quarter as many test clouds)")
    p.add_argument("--wide_train", default="torch", choices=["fused", "torch"],
                   help="the 1024-wide layers of a training step: the fused HIP layer (a third of the peak memory), or the "
                        "plain torch composition (the faster step at B 32, N 1024: DESIGN.md 8d)")
    p.add_argument("--edge_train", default=None, choices=["fused", "torch"],
                   help="--arch DGCNN: the EdgeConv layers of a training step: the fused HIP layer (no [B,C,N,k] tensor is "
                        "written), or the plain torch composition.  Required to train DGCNN; both values are explicit")
    p.add_argument("--dgcnn_k", default=20, type=int, help="--arch DGCNN: neighbours per point")
    p.add_argument("--emb_dims", default=1024, type=int, help="--arch DGCNN: width of the embedding (conv5)")
    p.add_argument("--dropout", default=0.5, type=float, help="--arch DGCNN: dropout of the head")
    p.add_argument("--quiet", action="store_true", default=False)
    return p


REFUSED_ARCHS = {
    "PointNetPP": "--arch PointNetPP cannot be trained here: the training-mode forward of geoa3_amd.pointnet2 raises "
                  "(its set-abstraction kernels are eval-mode only); only --arch PointNet is trained",
    "DGCNN": "--arch DGCNN is not trained without --edge_train fused | torch: by default the training-mode forward of "
             "geoa3_amd.dgcnn raises (its eval-mode EdgeConv kernels fold BatchNorm's running statistics); the flag selects "
             "the train-mode EdgeConv layer of geoa3_amd/dgcnn_train.py",
}


def check_supported(cfg) -> None:
    """The refusals, by name, before anything is read or written."""
    if cfg.arch in REFUSED_ARCHS and not (cfg.arch == "DGCNN" and getattr(cfg, "edge_train", None) is not None):
        raise NotImplementedError(REFUSED_ARCHS[cfg.arch])
    if cfg.arch not in ("PointNet", "DGCNN"):
        raise AssertionError("Not support such arch.")
    if cfg.mGPU > 1:
        raise NotImplementedError("-g / --mGPU %d cannot be honoured: training runs on one GPU (the fused wide layer takes "
                                  "its batch statistics over one device's batch; there is no DataParallel path)" % cfg.mGPU)


class SmoothedLabelLoss(nn.Module):
    """softmax_with_smoothing_label_loss of main_train.py:86-105: mean_b sum_k q_k (-log softmax)_k with
    q = one_hot (1 - s) + s / classes."""

    def __init__(self, num_classes: int = 40, label_smoothing: float = 0.2):
        super().__init__()
        self.num_classes, self.label_smoothing = num_classes, label_smoothing

    def forward(self, output, target):
        nll = -torch.log_softmax(output, 1)
        q = torch.nn.functional.one_hot(target, self.num_classes).to(output.dtype)
        q = q * (1 - self.label_smoothing) + self.label_smoothing / self.num_classes
        return (q * nll).sum(1).mean()


def transform_penalty(transform):
    """||T T^T - I||^2 / 2 summed over the batch (main_train.py:219-222)"""
    K = transform.size(1)
    d = torch.bmm(transform, transform.permute(0, 2, 1)) - torch.eye(K, device=transform.device, dtype=transform.dtype)
    return (d ** 2).sum() / 2


def adjust_learning_rate(optimizer, epoch, lr):
    lr = max(0.00001, lr * (0.7 ** (epoch // 20)))
    for group in optimizer.param_groups:
        group["lr"] = lr
    return lr


def save_checkpoint(state, is_best, dir, filename="checkpoint.pth.tar"):
    torch.save(state, os.path.join(dir, filename))
    if is_best:
        shutil.copyfile(os.path.join(dir, filename), os.path.join(dir, "model_best.pth.tar"))


# ---------------------------------------------------------------------------------------------------------------------
# data: (points [M,N,3] float32, labels [M] int64) per split, on the device
# ---------------------------------------------------------------------------------------------------------------------
def pc_normalize(points):
    """Provider/modelnet_trn_test.py:13-19, batched: centre on the mean, scale to unit largest norm"""
    points = points - points.mean(1, keepdim=True)
    return points / points.norm(dim=2).max(1)[0].view(-1, 1, 1)


def load_datadir(cfg, split, device):
    """The reference layout (Provider/modelnet_trn_test.py:22-45, 79-88): modelnet40_shape_names.txt, modelnet40_<split>.txt,
    <class>/<id>.txt comma separated; the first npoint rows, xyz, pc_normalize.  Read once."""
    names = [ln.rstrip() for ln in open(os.path.join(cfg.datadir, "modelnet40_shape_names.txt"))]
    classes = dict(zip(names, range(len(names))))
    ids = [ln.rstrip() for ln in open(os.path.join(cfg.datadir, "modelnet40_%s.txt" % split))]
    ids = [i for i in ids if i]
    shape = ["_".join(i.split("_")[:-1]) for i in ids]
    rows = np.stack([np.loadtxt(os.path.join(cfg.datadir, s, i + ".txt"), delimiter=",").astype(np.float32)[:cfg.npoint, :3]
                     for s, i in zip(shape, ids)])
    labels = torch.tensor([classes[s] for s in shape], dtype=torch.int64)
    return pc_normalize(torch.from_numpy(rows).to(device)), labels.to(device)


def load_meshes(cfg, split, device):
    """ROOT/<class>/<split>/*.off|*.obj -> --npoint surface points per mesh (area-weighted samples, farthest-point
    sampling, normalised: geoa3_amd.mesh.mesh_clouds, what Provider/gen_data_mat.py runs)."""
    from geoa3_amd import mesh
    from Provider.gen_data_mat import mesh_files, read_shape_names
    if not cfg.shape_names_file:
        raise ValueError("--mesh_dir needs --shape_names_file (one class name per line, the line number is the label)")
    pts, labels = [], []
    for lab, name in enumerate(read_shape_names(cfg.shape_names_file)):
        folder, files = mesh_files(cfg.mesh_dir, name, split)
        if not files:
            continue
        meshes = [mesh.READERS[os.path.splitext(f)[1].lower()](os.path.join(folder, f)) for f in files]
        (p, _), _ = mesh.mesh_clouds(mesh.pack_meshes(meshes, device), cfg.npoint, 0, cfg.surface_samples)
        keep = torch.isfinite(p).all(2).all(1)
        pts.append(p[keep].permute(0, 2, 1))
        labels.append(torch.full((int(keep.sum()),), lab, dtype=torch.int64, device=device))
    if not pts:
        raise RuntimeError("no mesh found under %s/<class>/%s" % (cfg.mesh_dir, split))
    return torch.cat(pts).contiguous(), torch.cat(labels)


def load_synthetic(cfg, split, device):
    from geoa3_amd.data import CAD_KINDS, synthetic_cad_clouds
    if cfg.classes != len(CAD_KINDS):
        raise ValueError("--synthetic has %d classes (the kinds of synthetic_cad_clouds): give -c %d" % (len(CAD_KINDS), len(CAD_KINDS)))
    M = cfg.synthetic_instances if split == "train" else max(cfg.synthetic_instances // 4, len(CAD_KINDS))
    data, _ = synthetic_cad_clouds(M, cfg.npoint, seed=cfg.random_seed + (1 if split == "train" else 2))
    labels = torch.arange(M) % len(CAD_KINDS)
    return data.permute(0, 2, 1).contiguous().to(device), labels.to(device)


def load_split(cfg, split, device):
    if cfg.synthetic:
        return load_synthetic(cfg, split, device)
    if cfg.mesh_dir is not None:
        return load_meshes(cfg, split, device)
    return load_datadir(cfg, split, device)


def to_network_frame(points):
    """[b,N,3] -> [b,3,N] with the axes permuted [0,2,1] (main_train.py:207,211)"""
    return points.transpose(2, 1)[:, [0, 2, 1], :].contiguous()


# ---------------------------------------------------------------------------------------------------------------------
def main(cfg):
    """-> a record of the run: {'epochs': [{'epoch', 'train_loss', 'train_acc', 'class_acc', 'instance_acc', 'is_best'}],
    'modeldir'}"""
    check_supported(cfg)
    if not torch.cuda.is_available():
        raise RuntimeError("main_train.py trains on the GPU, and none is present")
    from geoa3_amd.data import augment_batch
    from geoa3_amd.pointnet import PointNet
    device = torch.device("cuda")
    say = (lambda *a, **k: None) if cfg.quiet else print
    say(cfg)
    modeldir = os.path.join("Pretrained", cfg.arch, str(cfg.npoint))
    os.makedirs(modeldir, exist_ok=True)
    tb_writer = None
    if cfg.is_use_tb:
        from torch.utils.tensorboard import SummaryWriter
        os.makedirs(os.path.join(modeldir, "TB_event"), exist_ok=True)
        tb_writer = SummaryWriter(log_dir=os.path.join(modeldir, "TB_event"))

    seed = cfg.random_seed if cfg.id == 0 else int(time.time())          # main_train.py:136-142
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    gen = torch.Generator(device=device).manual_seed(seed)               # batch order and augmentation

    trn_x, trn_y = load_split(cfg, "train", device)
    tst_x, tst_y = load_split(cfg, "test", device)
    if int(max(trn_y.max(), tst_y.max())) >= cfg.classes:
        raise ValueError("the data holds label %d, the network has %d classes (-c)" % (int(max(trn_y.max(), tst_y.max())), cfg.classes))

    dgcnn = cfg.arch == "DGCNN"
    if dgcnn:
        from geoa3_amd.dgcnn import DGCNN
        net = DGCNN(k=cfg.dgcnn_k, emb_dims=cfg.emb_dims, dropout=cfg.dropout, output_channels=cfg.classes).to(device)
        net.edge_train = cfg.edge_train
    else:
        net = PointNet(cfg.classes).to(device)
        net.wide_train = cfg.wide_train
    criterion = SmoothedLabelLoss(cfg.classes)
    params = [{"params": [v], "lr": cfg.lr, "weight_decay": cfg.wd} for v in net.parameters() if v.requires_grad]
    optimizer = torch.optim.Adam(params)

    start_epoch, best_prec, class_prec = 1, 0, 0
    if cfg.resume:
        if not os.path.isfile(cfg.resume):
            raise AssertionError("WRONG RESUME PATH!")
        say("=> loading checkpoint '{}'".format(cfg.resume))
        checkpoint = torch.load(cfg.resume, map_location=device)
        start_epoch, best_prec, class_prec = checkpoint["epoch"] + 1, checkpoint["best_prec"], checkpoint["class_prec"]
        net.load_state_dict(checkpoint["state_dict"])
        optimizer.load_state_dict(checkpoint["optimizer"])
        say("\n=> loaded checkpoint '{}' (epoch {})".format(cfg.resume, checkpoint["epoch"]))

    record = {"epochs": [], "modeldir": modeldir}
    B = cfg.batch_size
    for epoch in range(start_epoch, cfg.epochs + 1):
        # ---- train
        net.train()
        order = torch.randperm(trn_x.shape[0], device=device, generator=gen)
        loss_sum = torch.zeros((), device=device, dtype=torch.float64)
        hit_sum = torch.zeros((), device=device, dtype=torch.float64)
        steps = (trn_x.shape[0] + B - 1) // B
        for i in range(steps):
            idx = order[i * B:(i + 1) * B]
            if idx.numel() < 2:          # BatchNorm has no statistics of one cloud's FC features
                continue
            points, target = trn_x[idx], trn_y[idx]
            if cfg.is_aug_data:
                points = augment_batch(points, gen)
            optimizer.zero_grad()
            if dgcnn:
                output = net(to_network_frame(points))
                loss = criterion(output, target)
            else:
                output, transform = net(to_network_frame(points))
                loss = criterion(output, target) + transform_penalty(transform) * 0.001
            loss.backward()
            optimizer.step()
            loss_sum += loss.detach().double() * idx.numel()
            hit_sum += (output.detach().argmax(1) == target).sum()
            if tb_writer is not None:
                tb_writer.add_scalar("Train Loss", float(loss), epoch * steps + i)
        seen = trn_x.shape[0] - (1 if trn_x.shape[0] % B == 1 else 0)
        trn_loss, trn_acc = float(loss_sum) / seen, 100.0 * float(hit_sum) / seen
        adjust_learning_rate(optimizer, epoch, cfg.lr)
        if not dgcnn:
            net.adjust_bn_momentum(epoch, cfg.bn_momentum)
        with open(os.path.join(modeldir, "result.txt"), "at") as f:
            f.write("epoch[{:3d}] train-acc: {:.3f}".format(epoch, trn_acc))

        # ---- val
        net.eval()
        seen_class = torch.zeros(cfg.classes, device=device, dtype=torch.float64)
        correct_class = torch.zeros(cfg.classes, device=device, dtype=torch.float64)
        with torch.no_grad():
            for i in range(0, tst_x.shape[0], B):
                points, target = tst_x[i:i + B], tst_y[i:i + B]
                right = (net(to_network_frame(points)).argmax(1) == target).double()
                seen_class.index_add_(0, target, torch.ones_like(right))
                correct_class.index_add_(0, target, right)
        present = seen_class > 0
        avg_class_acc = float((correct_class[present] / seen_class[present]).mean()) * 100
        test_acc = float(correct_class.sum() / seen_class.sum()) * 100
        with open(os.path.join(modeldir, "result.txt"), "at") as f:
            f.write("\t\ttest: C-acc {:.3f}  I-acc {:.3f}".format(avg_class_acc, test_acc))

        # ---- store checkpoint (main_train.py:312-344)
        is_best = test_acc > best_prec or (test_acc == best_prec and class_prec < avg_class_acc)
        if is_best:
            best_prec, class_prec = test_acc, avg_class_acc
        save_checkpoint({"epoch": epoch, "state_dict": net.state_dict(), "best_prec": best_prec, "class_prec": class_prec,
                         "optimizer": optimizer.state_dict()}, is_best, modeldir)
        with open(os.path.join(modeldir, "result.txt"), "at") as f:
            f.write("\t\tbest: C-acc {:.3f}  I-acc {:.3f}\n".format(class_prec, best_prec) if is_best else "\n")
        say("===> epoch [{:3d}]:  train loss {:.4f}  train acc {:.3f}    avg_class_acc  {:.4f}    avg_instance_acc {:.4f}    |    "
            "best: avg_class_acc  {:.4f}    avg_instance_acc {:.4f}\n".format(epoch, trn_loss, trn_acc, avg_class_acc, test_acc,
                                                                             class_prec, best_prec))
        record["epochs"].append(dict(epoch=epoch, train_loss=trn_loss, train_acc=trn_acc, class_acc=avg_class_acc,
                                     instance_acc=test_acc, is_best=is_best))
    return record


if __name__ == "__main__":
    main(build_parser().parse_args())
