#!/usr/bin/env python3
"""Cost and accuracy of the exact mode (t1d_step_dopri5: scipy's dopri5 as the reference drives it) on the bench's
workload: Navigator (one-minute steps), random meal tables (episodes start at a random minute of the day), a pool of random basal rates, Philox CGM noise, fp64.

Timing legs (1 Mi, 256 Ki, 128 Ki envs): us per launch from events over >= 200 launches after a warm-up, env-steps/s, the
mean RHS evaluations per env-minute and the mean over waves (64 consecutive envs) of each wave's maximum -- what a wave
costs, since it runs until its slowest lane is done.  Accuracy leg: 1 024 env-days (24 h) replayed on the oracle's
dopri (the reference's numbers) and on a tight solve (classical RK4, 48 sub-steps): max / p99 / median of each env-day's
max |BG difference|.  The kernel's registers come from a resource-usage compile.

usage: dopri5_bench.py [--out FILE] [--launches N] [--no-accuracy]   (GPU box; prints one JSON document)"""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simglucose_amd.batch_env import BatchedT1DSimEnv  # noqa: E402
from simglucose_amd import params, scenario_batch  # noqa: E402


def make(n, days=2, seed=5, random_start=True):
    """random_start: every env's episode starts at a random minute of the day (as the bench's workload), so that a window
    of a few hundred minutes sees every phase of a day -- night, meals, the hours after them"""
    pid = np.arange(n) % 30
    env = BatchedT1DSimEnv(patient=pid, sensor="Navigator", seed=seed, extra_outputs=False, integrator="dopri5")
    start = 0
    if random_start:
        g0 = torch.Generator(device=env.device); g0.manual_seed(11)
        start = torch.randint(0, 1440, (n,), generator=g0, device=env.device, dtype=torch.int32)
    mt, ma = scenario_batch.random_meal_tables(n, days=days, start_minute_of_day=start, seed=3, device=env.device)
    env.set_meals(mt, ma)
    _, tab = params.patient_table()
    b0 = torch.as_tensor(tab[pid, params.P_COL["u2ss"]] * tab[pid, params.P_COL["BW"]] / 6000.0, device=env.device)
    g = torch.Generator(device=env.device); g.manual_seed(1)
    pool = [(b0 * 2 * torch.rand(n, generator=g, device=env.device, dtype=torch.float64)).contiguous() for _ in range(8)]
    env.reset()
    return env, pool, pid, mt, ma


def timing(n, launches, warmup=30):
    env, pool, *_ = make(n)
    for k in range(warmup):
        env.step(pool[k % 8])
    nf_sum = torch.zeros(n, dtype=torch.float64, device=env.device)
    wave_max = torch.zeros((n + 63) // 64, dtype=torch.float64, device=env.device)
    # the RHS counts, one pass (not timed): minutes warmup .. warmup + launches
    for k in range(launches):
        env.step(pool[k % 8])
        nf = env.nfev.double()
        nf_sum += nf
        pad = torch.nn.functional.pad(nf, (0, (-n) % 64))
        wave_max += pad.view(-1, 64).max(dim=1).values
    assert env.sync() == 0
    # the same minutes again from the same state, timed: a fresh env
    env, pool, *_ = make(n)
    for k in range(warmup):
        env.step(pool[k % 8])
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); s.record()
    for k in range(launches):
        env.step(pool[k % 8])
    e.record(); torch.cuda.synchronize()
    assert env.sync() == 0
    us = s.elapsed_time(e) * 1000.0 / launches
    mean_nf = float(nf_sum.mean()) / launches
    mean_wave = float(wave_max.mean()) / launches
    return {"n_envs": n, "launches": launches, "minutes": f"{warmup}..{warmup + launches}", "us_per_launch": round(us, 1),
            "env_steps_per_s": n / (us * 1e-6), "rhs_per_env_minute": round(mean_nf, 3),
            "rhs_per_wave_minute_max_lane": round(mean_wave, 3), "divergence_factor": round(mean_wave / mean_nf, 3)}


def accuracy(n=1024, minutes=1440):
    from oracle import t1d_oracle as O
    env, pool, pid, mt, ma = make(n, days=1, seed=7, random_start=False)
    z = env.philox_normals(1 + 10 * (1 + minutes // 150), draw0=0, episode=1).cpu().numpy()
    t_s, a_s = mt.cpu().numpy().astype(np.int64), ma.cpu().numpy()
    cho = np.zeros((minutes, n))
    for j in range(n):
        for tt, aa in zip(t_s[:, j], a_s[:, j]):
            if tt < minutes:
                cho[tt, j] = aa
    pool_h = [p.cpu().numpy() for p in pool]
    ref = O.OracleEnv(pid, sensor="Navigator", normals=z, integrator="dopri")
    tight = O.OracleEnv(pid, sensor="Navigator", normals=z, integrator="rk4", n_sub=48)
    ref.reset(); tight.reset()
    env.reset()
    w_ref = np.zeros(n); w_tight = np.zeros(n); ref_tight = np.zeros(n)
    for k in range(minutes):
        env.step(pool[k % 8])
        r = ref.step(pool_h[k % 8], None, cho[k:k + 1])
        rt = tight.step(pool_h[k % 8], None, cho[k:k + 1])
        bg = env.bg.cpu().numpy()
        w_ref = np.maximum(w_ref, np.abs(bg - r["bg"]))
        w_tight = np.maximum(w_tight, np.abs(bg - rt["bg"]))
        ref_tight = np.maximum(ref_tight, np.abs(r["bg"] - rt["bg"]))
    assert env.sync() == 0
    st = lambda w: {"max": float(w.max()), "p99": float(np.percentile(w, 99)), "median": float(np.median(w)),
                    "within_1e-3": float((w <= 1e-3).mean())}
    return {"env_days": n, "vs_scipy_dopri": st(w_ref), "vs_tight_rk4_48": st(w_tight), "scipy_vs_tight": st(ref_tight)}


def resources():
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", "--cuda-device-only",
                          "-c", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull,
                          os.path.join(ROOT, "simglucose_amd", "csrc", "t1d_abi.hip")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode()
    blk = [b for b in out.split("Function Name: ") if b.startswith("_ZN3t1d18dopri5_step_kernel")][0]
    get = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
    return {"vgprs": get("VGPRs"), "agprs": get("AGPRs"), "scratch_bytes_per_lane": get("ScratchSize [bytes/lane]"),
            "occupancy_waves_per_simd": get("Occupancy [waves/SIMD]")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--sizes", default="1048576,262144,131072")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    a = ap.parse_args()
    res = {"workload": "Navigator 1-min steps, fp64, random meal tables, random basal pool (8), Philox noise, t1d_step_dopri5",
           "device": torch.cuda.get_device_name(0)}
    res["timing"] = [timing(int(n), a.launches) for n in a.sizes.split(",")]
    print(json.dumps(res["timing"]), flush=True)
    if not a.no_accuracy:
        res["accuracy"] = accuracy()
    if not a.no_resources:
        res["kernel"] = resources()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
