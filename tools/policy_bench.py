"""Cost of a closed loop under a learned policy: 160 Dexcom steps, random-meal days, all 30 patients, with
  mlp      BatchedT1DSimEnv.rollout_mlp: features, network and step fused in one launch (t1d_rollout_mlp)
  host     the same policy as torch ops around one step() launch per step -- what a user does without rollout_mlp
  pid      rollout_pid: the no-network floor
Every leg: fresh env, reset, one warm-up pass of `warmup` steps, then `steps` steps between two device synchronisations
(host clock).  The legs are alternated `reps` times.  `net_share` is 1 - pid / mlp: the part of the fused launch the network,
the windows and the wider register budget cost.  One JSON line per (dtype, batch size); --out writes them as a list.

    python tools/policy_bench.py --out profiles/policy/policy_bench.json

--exact: the same three legs on an integrator="dopri5" env (fp64 only), in the same run:
  mlp      rollout_mlp_dopri5 (t1d_rollout_mlp_dopri5): the network inside the free-running DOPRI5 kernel
  host     policy_action() + step() per step -- the loop that gives the same words with one launch pair per step
  pid      rollout_pid_dopri5: the no-network floor
and `nfev_mean`, the RHS evaluations per env over the timed steps, for the two roll-outs.

    python tools/policy_bench.py --exact --out profiles/policy/exact_bench.json
"""
import argparse

import benchlib

START = 360


def make_env(n, dtype, seed, exact=False):
    import numpy as np
    import torch
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    from simglucose_amd.scenario_batch import random_meal_tables
    e = BatchedT1DSimEnv(patient=np.arange(n) % 30, sensor="Dexcom", dtype=dtype, seed=seed, integrator="dopri5" if exact else None)
    e.set_meals(*random_meal_tables(n, days=1, start_minute_of_day=START, seed=seed, dtype=dtype))
    e.start_minute = torch.full((n,), START, dtype=torch.int32, device=e.device)
    e.reset()
    return e


def run_leg(leg, n, dtype, pol, steps, warmup, seed, exact=False):
    import torch
    e = make_env(n, dtype, seed, exact)
    zero = torch.zeros(n, dtype=dtype, device=e.device)
    state = e.new_policy_state(pol)
    pid_state = None

    def go(k):
        nonlocal pid_state
        if exact and leg == "mlp":
            e.rollout_mlp_dopri5(k, pol, policy_state=state)
        elif exact and leg == "pid":
            pid_state = e.rollout_pid_dopri5(k, 1.5e-4, 4e-7, 5e-4, pid_state=pid_state)
        elif exact:
            for _ in range(k):
                e.step(e.policy_action(pol, state), zero)
                pol.shift(state["cgm_hist"], state["ins_hist"], e.cgm, e.insulin)
                state["prev_meal"].copy_(e.meal)
        elif leg == "mlp":
            e.rollout_mlp(k, pol, policy_state=state)
        elif leg == "pid":
            pid_state = e.rollout_pid(k, 1.5e-4, 4e-7, 5e-4, pid_state=pid_state)
        else:
            for _ in range(k):
                feat = pol.features(state["cgm_hist"], state["ins_hist"], state["prev_meal"], e.start_minute + e.t)
                e.step(pol.forward(feat), zero)
                pol.shift(state["cgm_hist"], state["ins_hist"], e.cgm, e.insulin)
                state["prev_meal"].copy_(e.meal)
    ms = benchlib.timed_leg(lambda: go(warmup), lambda: go(steps), "host")
    out = {"us_per_step": 1e3 * ms / steps, "mean_bg": float(e.bg.mean())}
    if exact:
        out["ms"] = ms
        if leg != "host":                        # a roll-out leaves the RHS evaluations of the whole call in nfev
            out["nfev_mean"] = float(e.nfev.double().mean())
    out["status"] = benchlib.close_leg(e)
    del e
    torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", nargs="+", default=["mlp", "host", "pid"], choices=["mlp", "host", "pid"])
    ap.add_argument("--history", type=int, default=4)
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 16, 1])
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--label", default=None, help="free text kept in the output (e.g. which build was measured)")
    ap.add_argument("--exact", action="store_true", help="the three legs in the exact mode (integrator='dopri5', fp64)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.exact:
        args.dtypes = ["float64"]
    benchlib.require_gpu("policy_bench.py")
    import torch
    pol = benchlib.random_policy(args.history, args.widths, hidden="tanh", output="logistic", out_scale=0.06)
    results = []
    for name in args.dtypes:
        dtype = getattr(torch, name)
        for n in args.n:
            runs = benchlib.alternate(args.legs, args.reps,
                                      lambda leg: run_leg(leg, n, dtype, pol, args.steps, args.warmup, args.seed, args.exact))
            res = {"n_envs": n, "dtype": name, "steps": args.steps, "warmup": args.warmup, "sensor": "Dexcom", "history": args.history,
                   "widths": args.widths, "label": args.label, "integrator": "dopri5" if args.exact else "fixed-step", "device": torch.cuda.get_device_name(0), "legs": {}}
            for leg, rr in runs.items():
                res["legs"][leg] = {**benchlib.summarise([r["us_per_step"] for r in rr], "us_per_step"),
                                    "status": max(r["status"] for r in rr), "mean_bg": rr[-1]["mean_bg"]}
                if args.exact:
                    res["legs"][leg].update(benchlib.summarise([r["ms"] for r in rr], "ms"))
                    if "nfev_mean" in rr[-1]:
                        res["legs"][leg]["nfev_mean"] = rr[-1]["nfev_mean"]
            med = {leg: v["us_per_step_median"] for leg, v in res["legs"].items()}
            if "mlp" in med and "host" in med:
                res["host_over_mlp"] = med["host"] / med["mlp"]
            if "mlp" in med and "pid" in med:
                res["net_share"] = 1.0 - med["pid"] / med["mlp"]
                if args.exact:
                    res["mlp_over_pid"] = med["mlp"] / med["pid"]
            benchlib.emit(results, res)
    benchlib.write(results, args.out)


if __name__ == "__main__":
    main()
