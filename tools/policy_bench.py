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

--meal-bolus: what the meal bolus of MLPController(meal_bolus=140) costs inside the launch and what one launch is worth
against the step loop, with or without --exact; the legs become
  mlp          rollout_mlp (rollout_mlp_dopri5) under the bolus-free policy: the yardstick for "no cost", in the same run
  collect      fixed-step only: collect_mlp(sigma=None, on_done="continue") under the bolus-free policy -- the kernel family
               t1d_rollout_mlp_bolus launches, without the bolus: what of `mlp_bolus - mlp` is the family and what the bolus
  mlp_bolus    the same call under the same weights with meal_bolus=140 (t1d_rollout_mlp_bolus / t1d_rollout_mlp_dopri5_bolus)
  loop_bolus   policy_action() + policy_bolus() + step(u, bolus) per step: the only hybrid there is without the new calls
and `finish_rate`: the share of env-steps that end an episode under the two policies with collect_mlp(on_done="restart") on
the meal workload of tools/collect_bench.py (child#001 / adult#001, random initial glucose, random-meal days, sigma 0.1), over
`steps` steps after 128 steps that mix the batch -- what the bolus buys a trainer (fixed-step mode only: the exact mode's
collector takes no meal bolus).

    python tools/policy_bench.py --meal-bolus --dtypes float64 --reps 5 --out profiles/policy/bolus_bench.json

--relative: what the per-env scale and bias of MLPController(relative_to="basal") cost inside the launch, beside the plain and the
*_bolus calls of the same run, with or without --exact; the legs become
  mlp, mlp_bolus    as above: the plain policy without and with meal_bolus=140, the two reference points
  rel, rel_bolus    the same weights with relative_to="basal" (out_scale 3: up to three basal rates), without and with
                    meal_bolus=140 (t1d_rollout_mlp_rel / t1d_rollout_mlp_dopri5_rel)
  loop_rel_bolus    policy_action() + policy_bolus() + step(u, bolus) per step under the relative hybrid policy

    python tools/policy_bench.py --relative --dtypes float64 --reps 5 --out profiles/policy/rel_bench.json
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
    if isinstance(pol, dict):                        # --meal-bolus, --relative: the policy of the leg
        pol = pol[leg]
    e = make_env(n, dtype, seed, exact)
    zero = torch.zeros(n, dtype=dtype, device=e.device)
    state = e.new_policy_state(pol)
    pid_state = None

    def go(k):
        nonlocal pid_state
        if leg in ("loop_bolus", "loop_rel_bolus"):
            for _ in range(k):
                e.step(e.policy_action(pol, state), e.policy_bolus(pol, state))
                pol.shift(state["cgm_hist"], state["ins_hist"], e.cgm, e.insulin)
                state["prev_meal"].copy_(e.meal)
        elif exact and leg in ("mlp", "mlp_bolus", "rel", "rel_bolus"):
            e.rollout_mlp_dopri5(k, pol, policy_state=state)
        elif exact and leg == "pid":
            pid_state = e.rollout_pid_dopri5(k, 1.5e-4, 4e-7, 5e-4, pid_state=pid_state)
        elif exact:
            for _ in range(k):
                e.step(e.policy_action(pol, state), zero)
                pol.shift(state["cgm_hist"], state["ins_hist"], e.cgm, e.insulin)
                state["prev_meal"].copy_(e.meal)
        elif leg in ("mlp", "mlp_bolus", "rel", "rel_bolus"):
            e.rollout_mlp(k, pol, policy_state=state)
        elif leg == "collect":
            e.collect_mlp(k, pol, policy_state=state)
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
        if leg not in ("host", "loop_bolus", "loop_rel_bolus"):    # a roll-out leaves the RHS evaluations of the whole call in nfev
            out["nfev_mean"] = float(e.nfev.double().mean())
    out["status"] = benchlib.close_leg(e)
    del e
    torch.cuda.empty_cache()
    return out


def finish_rate(n, pol, steps, seed, warm_steps=128, sigma=0.1):
    """the share of env-steps that end an episode under `pol` on benchlib.mixed_env, restarts on the device"""
    import torch
    e = benchlib.mixed_env(n, seed)
    state = e.collect_mlp(warm_steps, pol, sigma=sigma, on_done="restart", days=benchlib.DAYS)
    tr = e.new_trace(steps, columns=("done",))
    e.collect_mlp(steps, pol, sigma=sigma, policy_state=state, trace=tr, on_done="restart", days=benchlib.DAYS)
    rate = float(tr["done"][1:].sum()) / (steps * n)
    benchlib.close_leg(e)
    del e
    torch.cuda.empty_cache()
    return rate


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
    ap.add_argument("--meal-bolus", action="store_true", help="legs mlp, mlp_bolus, loop_bolus: the cost and the worth of the in-kernel meal bolus")
    ap.add_argument("--relative", action="store_true", help="legs mlp, mlp_bolus, rel, rel_bolus, loop_rel_bolus: the cost of the per-env output")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.exact:
        args.dtypes = ["float64"]
    benchlib.require_gpu("policy_bench.py")
    import torch
    pol = benchlib.random_policy(args.history, args.widths, hidden="tanh", output="logistic", out_scale=0.06)
    if args.meal_bolus:
        hybrid = benchlib.random_policy(args.history, args.widths, hidden="tanh", output="logistic", out_scale=0.06, meal_bolus=140.0)
        args.legs = ["mlp", "mlp_bolus", "loop_bolus"] if args.exact else ["mlp", "collect", "mlp_bolus", "loop_bolus"]
        pol = {"mlp": pol, "collect": pol, "mlp_bolus": hybrid, "loop_bolus": hybrid}
    if args.relative:
        mk = lambda **kw: benchlib.random_policy(args.history, args.widths, hidden="tanh", output="logistic", **kw)
        args.legs = ["mlp", "mlp_bolus", "rel", "rel_bolus", "loop_rel_bolus"]
        pol = {"mlp": mk(out_scale=0.06), "mlp_bolus": mk(out_scale=0.06, meal_bolus=140.0), "rel": mk(out_scale=3.0, relative_to="basal"),
               "rel_bolus": mk(out_scale=3.0, relative_to="basal", meal_bolus=140.0)}
        pol["loop_rel_bolus"] = pol["rel_bolus"]
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
            if args.meal_bolus:
                res["bolus_over_mlp"] = med["mlp_bolus"] / med["mlp"]
                res["loop_over_bolus"] = med["loop_bolus"] / med["mlp_bolus"]
                res["mlp_spread"] = [min(r["us_per_step"] for r in runs["mlp"]), max(r["us_per_step"] for r in runs["mlp"])]
                if not args.exact:
                    res["bolus_over_collect"] = med["mlp_bolus"] / med["collect"]
                    res["finish_rate"] = {leg: finish_rate(n, pol[leg], args.steps, args.seed) for leg in ("mlp", "mlp_bolus")}
            if args.relative:
                res["bolus_over_mlp"] = med["mlp_bolus"] / med["mlp"]
                res["rel_over_mlp"] = med["rel"] / med["mlp"]
                res["rel_bolus_over_mlp_bolus"] = med["rel_bolus"] / med["mlp_bolus"]
                res["loop_over_rel_bolus"] = med["loop_rel_bolus"] / med["rel_bolus"]
                res["mlp_spread"] = [min(r["us_per_step"] for r in runs["mlp"]), max(r["us_per_step"] for r in runs["mlp"])]
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
