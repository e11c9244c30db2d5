"""Cost of a gym step with episodes that end: BatchedGymT1DSimEnv.step() on the hypo workload (child#001 / adult#001
alternating, basal 0.05 U/min, Dexcom, fp64) with
  none     auto_reset=False     -- the floor: finished envs are never restarted
  host     auto_reset=True      -- done.any() on the host, then new meal tables for the whole batch and reset(mask)
  device   auto_reset="device"  -- the step launch plus one launch of t1d_restart_done (finished envs collected in LDS and
                                   restarted with full waves)
  lanes    as device with set_option("restart_compact", 0): every lane restarts its own env
Every leg: fresh env, reset, `warmup` steps, then `steps` steps between two device synchronisations (host clock).  The legs
are alternated `reps` times.  One JSON line per batch size; --out writes them to a file as a list.

    python tools/autoreset_bench.py --out profiles/autoreset/autoreset_bench.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/autoreset_bench.py --n 1048576 --legs device --reps 1
"""
import argparse

import benchlib

LEGS = {"none": False, "host": True, "device": "device", "lanes": "device"}


def run_leg(leg, n, steps, warmup, seed):
    import torch
    from simglucose_amd.envs import BatchedGymT1DSimEnv
    env = BatchedGymT1DSimEnv(n, patient_name=["child#001", "adult#001"] * (n // 2), seed=seed, auto_reset=LEGS[leg])
    if leg == "lanes":
        env.env.set_option("restart_compact", 0)
    env.reset()
    a = torch.full((n,), 0.05, dtype=torch.float64, device=env.env.device)
    for _ in range(warmup):
        env.step(a)
    ep0 = env.env.episode.long().sum()

    def go():
        for _ in range(steps):
            env.step(a)
    ms = benchlib.timed_pass(go, "host")[1]
    restarted = int(env.env.episode.long().sum() - ep0)
    status = benchlib.close_leg(env.env)
    del env
    torch.cuda.empty_cache()
    return {"ms_per_step": ms / steps, "restarts_per_env_step": restarted / (n * steps), "status": status}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 20, 1 << 16])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", nargs="+", default=["none", "host", "device", "lanes"], choices=sorted(LEGS))
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    benchlib.require_gpu("autoreset_bench.py")
    import torch
    results = []
    for n in args.n:
        runs = benchlib.alternate(args.legs, args.reps, lambda leg: run_leg(leg, n, args.steps, args.warmup, args.seed))
        res = {"n_envs": n, "steps": args.steps, "warmup": args.warmup, "sensor": "Dexcom", "dtype": "float64",
               "basal_U_per_min": 0.05, "device": torch.cuda.get_device_name(0), "legs": {}}
        for leg, rr in runs.items():
            res["legs"][leg] = {**benchlib.summarise([r["ms_per_step"] for r in rr], "ms_per_step"),
                                "restarts_per_env_step": rr[-1]["restarts_per_env_step"], "status": max(r["status"] for r in rr)}
        benchlib.emit(results, res)
    benchlib.write(results, args.out)


if __name__ == "__main__":
    main()
