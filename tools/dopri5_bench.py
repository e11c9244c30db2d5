#!/usr/bin/env python3
"""Cost and accuracy of the exact mode (t1d_step_dopri5: scipy's dopri5 as the reference drives it) on the bench's
workload: Navigator (one-minute steps), random meal tables (episodes start at a random minute of the day), a pool of random basal rates, Philox CGM noise, fp64.

Timing legs (1 Mi, 256 Ki, 128 Ki envs): us per launch from events over >= 200 launches after a warm-up, env-steps/s, the
mean RHS evaluations per env-minute and the mean over waves (64 consecutive envs) of each wave's maximum -- what a wave
costs, since it runs until its slowest lane is done.  Accuracy leg: 1 024 env-days (24 h) replayed on the oracle's
dopri (the reference's numbers) and on a tight solve (classical RK4, 48 sub-steps): max / p99 / median of each env-day's
max |BG difference|.  The kernel's registers come from the device assembly (tools/kernel_asm.py).

--rollout: the closed-loop leg instead (Dexcom steps, BB controller and PID with mild gains, 160 steps = 8 h, 1 Mi and 256 Ki
envs): a step() loop with the controller in torch on the device between the launches (what the exact mode offered before
the roll-out kernel; no host synchronisation inside the loop) against rollout_*_dopri5 for the same steps from the same
state, alternated --reps times in one process, every repetition reported; and the count model (tools/dopri5_counts.py)
on per-minute RHS counts of the same closed loop.

usage: dopri5_bench.py [--out FILE] [--launches N] [--no-accuracy]   (GPU box; prints one JSON document)
       dopri5_bench.py --rollout [--out FILE] [--reps 3] [--sizes 1048576,262144]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simglucose_amd.batch_env import BatchedT1DSimEnv  # noqa: E402
from simglucose_amd import _lib, params, scenario_batch  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_asm  # noqa: E402
from dopri5_counts import wave_costs  # noqa: E402


def make(n, days=2, seed=5, random_start=True, sensor="Navigator", extra_outputs=False):
    """random_start: every env's episode starts at a random minute of the day (as the bench's workload), so that a window
    of a few hundred minutes sees every phase of a day -- night, meals, the hours after them"""
    pid = np.arange(n) % 30
    env = BatchedT1DSimEnv(patient=pid, sensor=sensor, seed=seed, extra_outputs=extra_outputs, integrator="dopri5")
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


PID_MILD = (1.5e-4, 4e-7, 5e-4)
ROLLOUT_STEPS, ROLLOUT_WARMUP = 160, 10


def step_loop(env, kind, steps, per_minute=None):
    """the closed loop as a step() loop, the controller in torch on the device between the launches.  per_minute: a list
    that receives every minute's nfev (the step is then made of one-minute launches with the action held: the same
    integration, the step's means formed as the kernel forms them)"""
    st = float(env.minutes_per_step)
    zero = torch.zeros(env.n, dtype=torch.float64, device=env.device)
    obs = env.cgm.clone()
    if kind == "bb":
        c = env.bb_constants()
        meal = zero.clone()
    else:
        P, I, D = PID_MILD
        integ, prev = zero.clone(), zero.clone()
    for _ in range(steps):
        if kind == "bb":
            corr = torch.where(obs > 150.0, (obs - 140.0) / c["cf"], zero)
            basal, bolus = c["basal"], torch.where(meal > 0, ((meal * st) / c["cr"] + corr) / st, zero)
        else:
            basal, bolus = P * (obs - 140.0) + I * integ + D * (obs - prev) / st, zero
            prev = obs
            integ = integ + (obs - 140.0) * st
        if per_minute is None:
            env.step(basal, bolus)
            obs, meal = env.cgm.clone(), env.meal.clone()
        else:
            obs, meal = zero.clone(), zero.clone()
            for _m in range(env.minutes_per_step):
                env.step(basal, bolus, minutes=1)
                per_minute.append(env.nfev.to(torch.int16).cpu().numpy())
                obs = obs + env.cgm / st
                meal = meal + env.meal / st


def rollout_leg(n, reps):
    """both controllers at n envs: events around ROLLOUT_STEPS steps after ROLLOUT_WARMUP steps, the two legs alternated"""
    res = {"n_envs": n, "steps": ROLLOUT_STEPS, "warmup_steps": ROLLOUT_WARMUP}
    for kind in ("bb", "pid"):
        runs = {"step_loop_ms": [], "rollout_ms": []}
        for rep in range(reps):
            for leg in ("step_loop_ms", "rollout_ms"):
                env, *_ = make(n, sensor="Dexcom", extra_outputs=True)
                state = None
                if leg == "step_loop_ms":
                    step_loop(env, kind, ROLLOUT_WARMUP)
                elif kind == "bb":
                    state = env.rollout_bb_dopri5(ROLLOUT_WARMUP)
                else:
                    state = env.rollout_pid_dopri5(ROLLOUT_WARMUP, *PID_MILD)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); s.record()
                if leg == "step_loop_ms":
                    step_loop(env, kind, ROLLOUT_STEPS)
                elif kind == "bb":
                    env.rollout_bb_dopri5(ROLLOUT_STEPS, bb_state=state)
                else:
                    env.rollout_pid_dopri5(ROLLOUT_STEPS, *PID_MILD, pid_state=state)
                e.record(); torch.cuda.synchronize()
                assert env.sync() == 0
                runs[leg].append(round(s.elapsed_time(e), 2))
                del env
        a, b = np.array(runs["step_loop_ms"]), np.array(runs["rollout_ms"])
        runs["ratio_of_medians"] = round(float(np.median(a) / np.median(b)), 3)
        runs["ratio_worst_case"] = round(float(a.min() / b.max()), 3)
        res[kind] = runs
        print(json.dumps({"n_envs": n, kind: runs}), flush=True)
    return res


def rollout_counts(n, launch_minutes=240):
    """the three count figures for the closed loop of the timing legs (after the same warm-up), from per-minute nfev"""
    out = {"n_envs": n, "launch_minutes": launch_minutes}
    for kind in ("bb", "pid"):
        env, *_ = make(n, sensor="Dexcom", extra_outputs=True)
        step_loop(env, kind, ROLLOUT_WARMUP)
        rows = []
        step_loop(env, kind, ROLLOUT_STEPS, per_minute=rows)
        assert env.sync() == 0
        c = wave_costs(np.stack(rows), launch_minutes)
        c["count_ratio_lockstep_over_free_running"] = round(c["lockstep_wave_cost"] / c["free_running_wave_cost"], 3)
        out[kind] = {k: round(v, 3) for k, v in c.items()}
        del env
    return out


def resources(kernel="_ZN3t1d18dopri5_step_kernel"):
    k = [k for k in kernel_asm.kernels(kernel_asm.device_asm()).values() if k.name.startswith(kernel)][0]
    return {key: k.figures[key] for key in ("vgprs", "agprs", "scratch_bytes_per_lane", "occupancy_waves_per_simd")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--sizes", default="1048576,262144,131072")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--rollout", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--count-envs", type=int, default=262144)
    a = ap.parse_args()
    if a.rollout:
        sizes = "1048576,262144" if a.sizes == ap.get_default("sizes") else a.sizes
        res = {"workload": "Dexcom 3-min steps, fp64, random meal tables (episodes start at a random minute of the day), Philox "
                           "noise; BBController and PID %r; step() loop with the controller in torch against rollout_*_dopri5" % (PID_MILD,),
               "device": torch.cuda.get_device_name(0)}
        res["timing"] = [rollout_leg(int(n), a.reps) for n in sizes.split(",")]
        res["counts"] = rollout_counts(a.count_envs)
        print(json.dumps(res["counts"]), flush=True)
        if not a.no_resources:
            res["kernels"] = {"dopri5_rollout_kernel": resources("_ZN3t1d21dopri5_rollout_kernel"),
                              "dopri5_step_kernel": resources()}
        txt = json.dumps(res, indent=1)
        print(txt)
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt + "\n")
        return
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
