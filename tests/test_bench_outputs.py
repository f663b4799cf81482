"""bench.py's plain run and `--dump-outputs`: a plain run times exactly --steps steps, prints the short headline line and
writes what its last timed step computed -- the same arrays as the attack loop driven directly on the same seeded inputs.
The dump's size limit and sampling are checked on the CPU."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = {"x", "logits", "g_cls", "g_geo", "loss_n", "cls_loss", "dis_loss", "hd_loss", "curv_loss", "constrain",
         "best_attack", "best_loss", "best_step"}


def _bench():
    sys.path.insert(0, REPO)
    return importlib.import_module("bench")


def test_dump_outputs_samples_the_same_rows_of_every_array_above_the_limit(tmp_path, monkeypatch):
    bench = _bench()
    rng = np.random.default_rng(3)
    arrays = {"x": rng.standard_normal((50, 3, 8)).astype(np.float32), "best_step": np.arange(50, dtype=np.float64)}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    for name, a in arrays.items():
        got = np.load(tmp_path / "all" / (name + ".npy"))
        assert got.dtype == a.dtype and np.array_equal(got, a)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2000)      # 50 rows of 104 bytes -> 19 rows
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    x, step = np.load(tmp_path / "s1" / "x.npy"), np.load(tmp_path / "s1" / "best_step.npy")
    assert x.nbytes + step.nbytes <= 2000 and len(step) == 19
    rows = step.astype(np.int64)
    assert np.all(np.diff(rows) > 0) and np.array_equal(x, arrays["x"][rows])
    assert np.array_equal(np.load(tmp_path / "s2" / "x.npy"), x)   # the sample is fixed


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_run_dumps_what_the_timed_loop_computed(tmp_path):
    import torch

    bench = _bench()
    steps, warmup, presteps = 5, 2, 3
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
           str(warmup), "--presteps", str(presteps), "--dump-outputs", str(tmp_path)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, env=env, timeout=800)
    assert r.returncode == 0, r.stderr[-3000:]
    line = r.stdout.strip().splitlines()[-1]
    out = json.loads(line)
    assert out["metric"] == "attack-iterations/sec (B=250, N=1024)" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["unit"] == "iterations/s of a 250-instance batch"
    assert out["steps"] == steps and out["warmup"] == warmup and out["config"]["presteps"] == presteps
    assert out["value"] == pytest.approx(1e3 / out["ms_per_step"], rel=1e-2)
    for key in ("roofline", "kernels_ms", "cd_kernel", "other_wide_mode", "other_configs", "cpu_baseline",
                "host_enqueue_ms_per_step", "multi_gpu"):
        assert key not in out, key                 # --full only
    assert len(line) < 2000
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(got) == NAMES
    assert all(a.dtype in (np.float32, np.float64) and a.shape[0] == 250 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6
    assert got["x"].shape == (250, 3, 1024) and np.isfinite(got["x"]).all()

    # the same loop driven directly: presteps + warmup + steps iterations from the same seeded inputs
    from geoa3_amd.attack import AttackRunner
    from geoa3_amd.data import synthetic_clouds, synthetic_state_dict
    from geoa3_amd.pointnet import PointNet, default_wide_mode
    dev = torch.device("cuda", 0)
    net = PointNet(40)
    net.load_state_dict(synthetic_state_dict(40, seed=0, device=dev))
    net = net.to(dev).eval()
    net.wide_mode = default_wide_mode()
    ori, nrm = synthetic_clouds(250, 1024, seed=100)
    ori, nrm = ori.to(dev), nrm.to(dev)
    with torch.no_grad():
        gt = net(ori).argmax(1)
    total = presteps + warmup + steps
    runner = AttackRunner(net, 250, 1024, bench.cfg_full_geoa3(total + 24), dev, global_batch=250)
    runner.setup(ori, nrm, gt, gt)
    runner.begin_search_step((torch.randn(250, 3, 1024, generator=torch.Generator().manual_seed(7)) * 1e-3).to(dev))
    for s in range(total):
        runner.step(s, 0)
    torch.cuda.synchronize()
    want = bench.step_outputs(runner)
    runner.end_search_step()
    for name in NAMES:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
