"""bench.py --gpus N starts its own N ranks: the
launcher's decision and command, and the N-rank plumbing end to end on the CPU
(--dry-run: gloo ranks, the all-gather and max over ranks the real bench uses,
one JSON line relayed from rank 0)."""

import json
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_check_world_decides_launch_run_or_refuse():
    import bench
    assert bench.check_world(SimpleNamespace(gpus=1), {}) == "run"
    assert bench.check_world(SimpleNamespace(gpus=8), {}) == "launch"
    assert bench.check_world(SimpleNamespace(gpus=8), {"WORLD_SIZE": "8"}) == "run"
    assert bench.check_world(SimpleNamespace(gpus=1), {"WORLD_SIZE": "1"}) == "run"
    with pytest.raises(SystemExit, match="WORLD_SIZE=2 but --gpus 1"):
        bench.check_world(SimpleNamespace(gpus=1), {"WORLD_SIZE": "2"})


def test_launch_command_is_torchrun_on_this_script(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7"])
    cmd = bench.launch_command(SimpleNamespace(gpus=4), 29555)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--master-addr=127.0.0.1" in cmd and "--master-port=29555" in cmd
    assert cmd[-5:] == [os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "7"]


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_exact_floats_fixed_sample_and_size(tmp_path):
    """--dump-outputs: float32 / float64 files that hold the integers exactly, small
    arrays whole, large ones as the same sample on every call, under 64 MB together."""
    import numpy as np
    import torch
    import bench
    n = 12_000_000
    code = (torch.arange(n, dtype=torch.int64) * 2654435761 % (1 << 32)).to(torch.int32)  # every bit in use
    arrs = {"code": code, "status": (torch.arange(n) % 251).to(torch.uint8),
            "counters": torch.tensor([0, 1, 2 ** 40 + 1], dtype=torch.int64),
            "digest_long": torch.arange(96, dtype=torch.uint8).view(3, 32), "empty": torch.zeros(0, dtype=torch.int32)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrs)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert sorted(got) == sorted(arrs)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    assert got["code"].dtype == np.float64 and got["status"].dtype == np.float32
    assert got["counters"].tolist() == [0, 1, 2 ** 40 + 1] and got["empty"].shape == (0,)
    assert np.array_equal(got["digest_long"], np.arange(96).reshape(3, 32))
    # the sample: the same sorted rows of both arrays, values exact
    share = bench.DUMP_BYTES // len(arrs)
    idx = np.sort(np.random.default_rng(1234).integers(0, n, share // 8))
    assert np.array_equal(got["code"], code.numpy()[idx].astype(np.float64))
    idx4 = np.sort(np.random.default_rng(1234).integers(0, n, share // 4))
    assert np.array_equal(got["status"], (idx4 % 251).astype(np.float32))
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_bench_gpus_2_dry_run_spawns_two_ranks():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env["AVDB_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"],
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["records_total"] == 200
    assert abs(out["ms_per_step"] - 2.0) < 1e-9  # the max over the two ranks' times
