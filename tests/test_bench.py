"""bench.py's output dump (--dump-outputs) and its plain / --full split: the dump's sizes on CPU tensors, and on the GPU a
plain run and a --full run of the same arguments that must time and return the very same episode."""
import glob
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stub_env(n, dtype, env_offset=0):
    """the tensors of a BatchedT1DSimEnv that dump_outputs reads, on the CPU"""
    import torch
    g = torch.Generator().manual_seed(3)
    e = types.SimpleNamespace(n=n, device=torch.device("cpu"), env_offset=env_offset)
    e.x = torch.randn(45, n, generator=g, dtype=dtype)[0:13]
    e.cgm, e.reward, e.bg = (torch.randn(n, generator=g, dtype=dtype) for _ in range(3))
    e.done = (torch.rand(n, generator=g) < 0.1).to(torch.uint8)
    e.t = torch.full((n,), 1800, dtype=torch.int32)
    return e


@pytest.mark.parametrize("n,dtype_name,rank,world", [(1 << 20, "float64", 0, 1), (1 << 20, "float32", 0, 1),
                                                     (4 << 20, "float64", 0, 1), (1000, "float64", 0, 1),
                                                     (1 << 20, "float64", 3, 8)])
def test_dump_outputs_stay_under_64_mb_and_repeat(tmp_path, n, dtype_name, rank, world):
    import torch
    import bench
    env = _stub_env(n, getattr(torch, dtype_name), env_offset=rank * n)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(env, str(a), rank, world)
    bench.dump_outputs(env, str(b), rank, world)
    suffix = "" if world == 1 else ".rank%d" % rank
    files = sorted(glob.glob(str(a / "*.npy")))
    names = {os.path.basename(f)[:-len(suffix + ".npy")] for f in files}
    assert {"cgm", "reward", "done", "bg", "t", "patient_state", "patient_state_envs"} <= names
    assert sum(os.path.getsize(f) for f in files) * world <= 64 * 10 ** 6
    for f in files:
        x, y = np.load(f), np.load(str(b / os.path.basename(f)))
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
    ids = np.load(str(a / ("patient_state_envs%s.npy" % suffix))).astype(np.int64) - env.env_offset
    assert np.array_equal(np.load(str(a / ("patient_state%s.npy" % suffix))), env.x[:, ids].numpy())
    if "env_index" in names:
        ids = np.load(str(a / ("env_index%s.npy" % suffix))).astype(np.int64) - env.env_offset
    else:
        ids = np.arange(n)
        assert n <= 1 << 20 or world > 1
    assert np.array_equal(np.load(str(a / ("cgm%s.npy" % suffix))), env.cgm[ids].numpy())
    assert np.array_equal(np.load(str(a / ("done%s.npy" % suffix))), env.done[ids].float().numpy())


def _bench(args, timeout=600):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return json.loads(p.stdout.decode().strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_and_full_bench_runs_return_the_same_outputs(tmp_path):
    """--full replays the batch on the oracle (three full resets) ahead of the timed episode; the plain run skips that
    and must still time the same episode -- same Philox stream, same outputs bit for bit -- and report what it timed."""
    common = ["--gpus", "1", "--envs", "8192", "--steps", "37", "--warmup", "10", "--prewarm", "0",
              "--accuracy-envs", "64", "--accuracy-minutes", "120", "--rk4-steps", "10"]
    plain = _bench(common + ["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(common + ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    for j in (plain, full):
        assert j["steps"] == 37 and j["ms_per_step"] > 0 and j["sane"] and j["unit"] == "env-steps/s"
    assert plain["accuracy"] is None and plain["north_star_rk4"] is None and "cpu_baseline" not in plain
    assert full["accuracy"]["max_abs_err_mg_dl"] < 1.0 and full["north_star_rk4"]["launches_timed"] == 10
    files = sorted(os.listdir(str(tmp_path / "plain")))
    assert files == sorted(os.listdir(str(tmp_path / "full"))) and "cgm.npy" in files
    for f in files:
        x, y = np.load(str(tmp_path / "plain" / f)), np.load(str(tmp_path / "full" / f))
        assert np.array_equal(x, y), f
    t = np.load(str(tmp_path / "plain" / "t.npy"))
    assert t.shape == (8192,) and (t == 47).all()
    assert plain["bg_mean"] == full["bg_mean"]
