"""bench.py's N-rank launch: `bench.py --gpus N` without a
launcher starts torch.distributed.run with N ranks as a child process, and a
WORLD_SIZE that disagrees with --gpus is an error, not a silent one-rank run."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _args(*argv):
    old = sys.argv
    sys.argv = ["bench.py", *argv]
    try:
        return bench.parse()
    finally:
        sys.argv = old


def test_one_gpu_runs_in_process():
    assert bench.check_launch(_args(), env={}) is None
    assert bench.check_launch(_args("--gpus", "1"), env={}) is None


def test_n_gpus_without_launcher_builds_torchrun_child():
    old = sys.argv
    sys.argv = ["bench.py", "--gpus", "4", "--steps", "7", "--exchange", "factored"]
    try:
        cmd = bench.check_launch(bench.parse(), env={})
    finally:
        sys.argv = old
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd and "--master-addr=127.0.0.1" in cmd
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "7", "--exchange", "factored"]


def test_under_launcher_world_size_must_match():
    assert bench.check_launch(_args("--gpus", "8"), env={"WORLD_SIZE": "8"}) is None
    with pytest.raises(SystemExit, match="WORLD_SIZE=8 but --gpus 1"):
        bench.check_launch(_args(), env={"WORLD_SIZE": "8"})
    with pytest.raises(SystemExit, match="WORLD_SIZE=2 but --gpus 4"):
        bench.check_launch(_args("--gpus", "4"), env={"WORLD_SIZE": "2"})
    with pytest.raises(SystemExit, match="must be >= 1"):
        bench.check_launch(_args("--gpus", "0"), env={})


def test_mismatch_exits_nonzero_before_any_work():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "WORLD_SIZE=3 but --gpus 2" in r.stderr
    assert not r.stdout.strip()


def test_rccl_launch_refuses_more_ranks_than_devices():
    # no GPU here: RCCL ranks cannot share one device, so N > visible devices is refused up front
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "RCCL needs 2 devices" in r.stderr


def test_full_and_dump_outputs_are_off_by_default():
    a = _args("--gpus", "1", "--steps", "3", "--warmup", "2")
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (3, 2)
    a = _args("--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_writes_float32_within_the_budget(tmp_path, monkeypatch):
    """Small arrays whole and in shape, a large one as the same seeded sample on every call, integer
    outputs as float32, absent gradients left out, and the files together inside the byte budget."""
    import numpy as np
    import torch

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)  # 1000 elements over 2 non-empty arrays
    big = torch.arange(10_000, dtype=torch.float64).reshape(100, 100)
    arrays = {"big": big, "radii": torch.arange(6, dtype=torch.int32).reshape(2, 3), "empty": torch.zeros(0, 3),
              "none": None}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), {"radii": arrays["radii"], "big": big + 0.0, "empty": arrays["empty"]})
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["big.npy", "radii.npy"]  # no file for an absent or empty array
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["radii.npy"].tolist() == [[0, 1, 2], [3, 4, 5]]
    s = got["big.npy"]
    assert s.shape == (500,) and np.all(np.diff(s) >= 0) and s.min() >= 0 and s.max() < 10_000
    assert len(np.unique(s)) > 400  # a spread sample, not one block
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))
    assert sum(v.nbytes for v in got.values()) <= 4000


@pytest.mark.gpu
def test_plain_run_prints_the_contract_line_and_dumps_outputs(tmp_path):
    """A plain run (small scene): --steps sets the timed steps, the line holds the contract fields and
    none of what --full measures, and --dump-outputs leaves the outputs and gradients of the last step."""
    import numpy as np

    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--P", "3000", "--width", "130", "--height", "70", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    (line,) = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "iters/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 1.0) < 1e-2
    assert not {"roofline", "cpu_baseline", "dist"} & set(line)
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert {"color", "radii", "mdepth", "alpha", "normal", "grad_means3D", "grad_means2D", "grad_shs",
            "grad_opacities", "grad_scales", "grad_rotations"} <= set(got)
    assert got["color"].shape == (3, 70, 130) and got["grad_shs"].shape == (3000, 16, 3)
    assert all(v.dtype == np.float32 and v.size and np.isfinite(v).all() for v in got.values())
    assert not {"grad_sg_axis", "grad_sg_sharpness", "grad_sg_color"} & set(got)  # SG degree 0: empty, no file
    assert np.abs(got["color"]).max() > 0 and np.abs(got["grad_means3D"]).max() > 0 and got["radii"].max() > 0
    assert sum(v.nbytes for v in got.values()) <= 64e6


def test_launcher_starts_n_ranks(tmp_path):
    """The real child launch (gloo, CPU): two ranks start, see WORLD_SIZE = 2
    and rank 0 prints the line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
                        "--launch-probe"], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert lines == [{"n_gpus": 2, "rank_sum": 3}]
