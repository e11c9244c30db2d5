"""Cost and use of per-env PID gains (rollout_pid / rollout_pid_dopri5 with arrays, t1d_rollout_pid_gains): fp64 Dexcom, all
30 patients, a random-meal day from 06:00, `steps` closed-loop steps per pass, in one of two modes

  cost    scalar  rollout_pid(steps, P, I, D, target) on n envs
          per_env the same call with the four numbers as [n] arrays filled with them: the same work plus the four arrays
  sweep   loop    SETS gain sets as SETS scalar roll-outs of n / SETS envs each (one env object, reset between the
                  roll-outs outside the clock): the loop a tuning run had to write
          batch   one per-env roll-out of n envs, set j on envs [j n / SETS, (j + 1) n / SETS)

--exact runs either mode through rollout_pid_dopri5 (an env with integrator="dopri5").  Every pass: reset (not timed), then
the roll-out between two device synchronisations (host clock), so a leg's launch overhead is in its figure.  The legs are
alternated `reps` times in one run after a warm-up pass each; the record has the median, the extremes and every run of each
leg and ratio = per_env / scalar (cost) or batch / loop (sweep) of the medians.  One JSON line per batch size; --out writes
them to a file as a list.

    python tools/pid_gains_bench.py --mode cost --out profiles/pid_gains/cost.json
    python tools/pid_gains_bench.py --mode sweep --out profiles/pid_gains/sweep.json
    python tools/pid_gains_bench.py --mode sweep --exact --out profiles/pid_gains/sweep_exact.json
"""
import argparse

import benchlib

STOCK = (1.5e-4, 4e-7, 5e-4, 140.0)
SETS = 16


def gain_sets():
    """a 4 x 4 grid around the stock gains: P x D, with the stock I and target"""
    return [(STOCK[0] * p, STOCK[1], STOCK[2] * d, STOCK[3]) for p in (0.5, 1.0, 1.5, 2.0) for d in (0.0, 1.0, 2.0, 4.0)]


def make_env(n, seed, exact):
    import numpy as np
    import torch
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    from simglucose_amd.scenario_batch import random_meal_tables
    e = BatchedT1DSimEnv(patient=np.arange(n) % 30, sensor="Dexcom", dtype=torch.float64, seed=seed,
                         integrator="dopri5" if exact else None)
    e.set_meals(*random_meal_tables(n, days=1, start_minute_of_day=360, seed=seed, device=e.device))
    return e


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("cost", "sweep"), default="cost")
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    benchlib.require_gpu("pid_gains_bench.py")
    import torch
    results = []
    sets = gain_sets()
    for n in args.n:
        if n % SETS:
            raise SystemExit("--n must be a multiple of %d" % SETS)
        big = make_env(n, args.seed, args.exact)
        small = make_env(n // SETS, args.seed, args.exact) if args.mode == "sweep" else None
        roll = lambda e, *a: (e.rollout_pid_dopri5 if args.exact else e.rollout_pid)(args.steps, *a)
        if args.mode == "cost":
            arrays = big.pid_gains(*STOCK)
            legs = {"scalar": lambda: roll(big, *STOCK), "per_env": lambda: roll(big, arrays)}
        else:
            block = torch.arange(n, device=big.device) // (n // SETS)
            arrays = big.pid_gains(*(torch.tensor([s[k] for s in sets], dtype=torch.float64, device=big.device)[block] for k in range(4)))
            legs = {"batch": lambda: roll(big, arrays)}

        def one(leg):
            if leg == "loop":                                # SETS x (reset outside the clock, scalar roll-out inside)
                ms = 0.0
                for s in sets:
                    small.reset()
                    ms += benchlib.timed_pass(lambda: roll(small, *s), "host")[1]
                return ms
            big.reset()
            return benchlib.timed_pass(legs[leg], "host")[1]

        names = ["scalar", "per_env"] if args.mode == "cost" else ["loop", "batch"]
        for leg in names:                                    # warm-up: tables, plans, allocator
            one(leg)
        runs = benchlib.alternate(names, args.reps, one)
        rec = {"mode": args.mode, "exact": args.exact, "n_envs": n, "steps": args.steps, "sensor": "Dexcom", "dtype": "float64",
               "gain_sets": 1 if args.mode == "cost" else SETS, "clock": "host", "device": torch.cuda.get_device_name(0), "legs": {}}
        for leg in names:
            rec["legs"][leg] = benchlib.summarise(runs[leg], "ms", spread=True)
        rec["ratio"] = rec["legs"][names[1]]["ms_median"] / rec["legs"][names[0]]["ms_median"]
        rec["status"] = max(benchlib.close_leg(e) for e in (big, small) if e is not None)
        benchlib.emit(results, rec)
        del big, small, legs, arrays
        torch.cuda.empty_cache()
    benchlib.write(results, args.out)


if __name__ == "__main__":
    main()
