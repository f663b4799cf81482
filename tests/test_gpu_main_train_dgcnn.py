"""GPU: main_train.py --arch DGCNN --edge_train fused end to end on synthetic clouds (5 classes, 128 points, batch 8,
3 epochs of 40 clouds): the files and their keys, result.txt's line format, a falling training loss, --resume, and
main_attack.py --arch DGCNN on the checkpoint it wrote; without --edge_train the arch is refused as before."""
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

ARGS = ["--arch", "DGCNN", "--edge_train", "fused", "--synthetic", "-c", "5", "--npoint", "128", "-b", "8", "--epochs", "3",
        "--synthetic_instances", "40", "--quiet"]


def test_without_edge_train_the_arch_is_refused(tmp_path, monkeypatch):
    import main_train
    monkeypatch.chdir(tmp_path)
    argv = [a for a in ARGS if a not in ("--edge_train", "fused")]
    with pytest.raises(NotImplementedError, match="DGCNN"):
        main_train.main(main_train.build_parser().parse_args(argv))
    assert not os.listdir(tmp_path)          # refused before anything is written


def test_train_resume_and_attack_the_result(tmp_path, monkeypatch):
    import main_attack
    import main_train
    from geoa3_amd.dgcnn import DGCNN
    monkeypatch.chdir(tmp_path)
    rec = main_train.main(main_train.build_parser().parse_args(ARGS))
    d = os.path.join("Pretrained", "DGCNN", "128")
    assert rec["modeldir"] == d
    for name in ("checkpoint.pth.tar", "model_best.pth.tar"):
        ck = torch.load(os.path.join(d, name), map_location="cpu")
        assert set(ck) == {"epoch", "state_dict", "best_prec", "class_prec", "optimizer"}
        assert list(ck["state_dict"]) == list(DGCNN(output_channels=5).state_dict())
    assert torch.load(os.path.join(d, "checkpoint.pth.tar"), map_location="cpu")["epoch"] == 3
    lines = open(os.path.join(d, "result.txt")).read().splitlines()
    assert len(lines) == 3
    pat = re.compile(r"^epoch\[ *(\d+)\] train-acc: \d+\.\d{3}\t\ttest: C-acc \d+\.\d{3}  I-acc \d+\.\d{3}"
                     r"(\t\tbest: C-acc \d+\.\d{3}  I-acc \d+\.\d{3})?$")
    assert [int(pat.match(ln).group(1)) for ln in lines] == [1, 2, 3]
    ep = rec["epochs"]
    print("train loss per epoch", [round(e["train_loss"], 4) for e in ep], "train acc", [round(e["train_acc"], 1) for e in ep],
          "test I-acc", [round(e["instance_acc"], 1) for e in ep], "C-acc", [round(e["class_acc"], 1) for e in ep])
    assert ep[-1]["train_loss"] < ep[0]["train_loss"]
    # --resume continues at epoch 4
    i = ARGS.index("--epochs")
    rec2 = main_train.main(main_train.build_parser().parse_args(
        ARGS[:i + 1] + ["4"] + ARGS[i + 2:] + ["--resume", os.path.join(d, "checkpoint.pth.tar")]))
    assert [e["epoch"] for e in rec2["epochs"]] == [4]
    assert len(open(os.path.join(d, "result.txt")).read().splitlines()) == 4
    # main_attack.py --arch DGCNN loads the checkpoint (the file exists: no stand-in weights) and runs one binary step of
    # three iterations on clouds of the five kinds, labelled by kind
    from geoa3_amd.data import write_synthetic_mat
    write_synthetic_mat(str(tmp_path / "Data" / "syn128.mat"), [i % 5 for i in range(10)], 128, seed=5, kind="cad")
    cfg = main_attack.build_parser().parse_args(
        ["--attack", "GeoA3", "--attack_label", "Untarget", "--arch", "DGCNN", "-b", "10", "-c", "5", "--npoint", "128",
         "--data_dir_file", str(tmp_path / "Data" / "syn128.mat"), "--binary_max_steps", "1", "--iter_max_steps", "3",
         "--curv_loss_knn", "8", "--quiet"])
    saved = main_attack.main(cfg)
    assert saved.startswith(os.path.join("Exps", "DGCNN_npoint128"))
    assert open(os.path.join(saved, "attack_result.txt")).read().startswith("attack success: ")
