"""bench.py --dump-outputs DIR: after the timed steps, the loss terms of the last step and the model it updated land in DIR as float32
.npy files (at most 64 MB in all), so that two builds run with the same arguments can be compared output for output. Such a run uses
the engine's deterministic reductions: two runs with the same arguments write identical arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_losses_parameters_and_buffers(tmp_path):
    torch.manual_seed(0)
    model = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4))
    losses = {"loss": torch.tensor(1.5), "box_loss": torch.tensor([0.25])}
    bench.dump_outputs(str(tmp_path / "out"), model, losses)
    got = {f[:-4]: np.load(str(tmp_path / "out" / f)) for f in os.listdir(str(tmp_path / "out"))}
    assert set(got) == {"loss", "box_loss", "parameters", "buffers"}
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["loss"].tolist() == [1.5] and got["box_loss"].tolist() == [0.25]
    want = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    np.testing.assert_array_equal(got["parameters"], want)
    # running mean (4) + running var (4); the int64 step counter is not an output
    np.testing.assert_array_equal(got["buffers"], np.array([0.0] * 4 + [1.0] * 4, np.float32))


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    model = nn.Sequential(nn.Linear(1 << 12, 1 << 12, bias=False), nn.BatchNorm1d(1))   # 64 MiB of float32 weights, and more
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "out"), model, {"loss": torch.tensor(0.0)})
    assert not os.path.exists(str(tmp_path / "out"))


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step_the_same_every_run(tmp_path):
    runs = []
    for i, timing in enumerate((False, True)):
        # the first run is a plain one (headline only); the second, under --full, also times every kernel in an eager re-run of the
        # K steps after the timed region: the dump must be taken before it (the re-run trains the same model further), so both runs
        # write the same arrays
        out = tmp_path / ("dump%d" % i)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8", "--size", "256",
               "--dump-outputs", str(out)] + (["--full", "--no-cpu-baseline", "--no-deeplab", "--no-h2d", "--no-extra"] if timing else [])
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["config"]["deterministic"] is True
        assert ("kernels" in line) == timing and ("peaks_measured" in line) == timing
        if not timing:   # a plain run carries the headline alone
            assert not set(line) & {"roofline", "with_h2d", "infer", "config3_deeplabv3plus_r50", "config4_yolox_s", "cpu_baseline"}, sorted(line)
        files = {f[:-4]: str(out / f) for f in os.listdir(str(out))}
        assert set(files) == {"loss", "box_loss", "obj_loss", "cls_loss", "parameters", "buffers"}
        assert sum(os.path.getsize(f) for f in files.values()) <= 64 << 20
        got = {k: np.load(f) for k, f in files.items()}
        assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
        assert abs(float(got["loss"][0]) - line["config"]["final_loss"]) <= 1e-4 + 1e-3 * abs(line["config"]["final_loss"])
        runs.append(got)
    # the dumped model is the trained one: bench.py seeds its weights with 1029, and 1 warm-up, 2 capture warm-ups, 2 replays and
    # the 3 timed steps moved them
    from cvpytorch_amd import yolov5
    torch.manual_seed(1029)
    init = torch.cat([p.detach().float().reshape(-1) for p in yolov5.YOLOv5(80, "s").parameters()]).numpy()
    assert runs[0]["parameters"].size == init.size
    moved = runs[0]["parameters"] != init
    assert moved.mean() > 0.5, moved.mean()
    # same arguments, same inputs: the same outputs, bit for bit
    for k, v in runs[0].items():
        np.testing.assert_array_equal(v, runs[1][k], err_msg=k)
