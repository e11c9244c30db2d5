"""Cost of collecting K steps of trajectories in the exact mode (DOPRI5), fp64 Dexcom, child#001 / adult#001 with random
initial glucose -- tools/collect_bench.py for collect_mlp_dopri5, same envs, same two policies:
  net      a random 2 x 16 tanh net with logistic output on [0, 0.06] U/min, with exploration noise
  hypo     a constant 0.05 U/min (--hypo-basal): episodes end low all the time -- the hypo workload of profiles/collect
and four legs:
  collect  (a) collect_mlp_dopri5(K, on_done="restart") with every trace column: one launch per 240 simulated minutes
  loop     (b) what it replaces: K x (rollout_mlp_dopri5(1), restart_done, the torch reset of the policy windows, stacking
           reward and done)
  plain    collect_mlp_dopri5(K, on_done="continue", sigma=None), no new trace: the no-restart case
  rollout  (c) rollout_mlp_dopri5(K), no noise, no restarts: the floor, and what `plain` should cost
Every leg: fresh env, `warm_steps` steps so that the batch is mixed, one warm-up pass, then K steps between two events on the
stream, `reps` times (5), legs alternated; median, minimum and maximum are reported.  As in collect_bench.py the timed window
holds what a caller pays per batch of K steps, the allocation of the trace included.  `finish_rate` is the share of env-steps
of the timed window that ended an episode; every repetition builds the same env from the same seed, so it is the same in
each (`finish_rate_runs` shows it).  One JSON line per (policy, batch size); --out writes them as a list.

    python tools/collect_exact_bench.py --out profiles/collect/exact_collect_bench.json
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DAYS = 2
COLUMNS = ("bg", "cgm", "cho", "insulin", "action", "reward", "done", "eps", "features")


def make_policy(kind, history=4, basal=0.05):
    import torch
    from simglucose_amd.controller.mlp_ctrller import MLPController
    F = 2 * history + 3
    if kind == "hypo":
        return MLPController([(torch.zeros(1, F, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))], history=history,
                             output="identity", out_scale=1.0, out_bias=basal)
    g = torch.Generator().manual_seed(0)
    layers, n_in = [], F
    for w in (16, 16, 1):
        layers.append((torch.randn(1, w, n_in, generator=g, dtype=torch.float64) / math.sqrt(n_in),
                       0.1 * torch.randn(1, w, generator=g, dtype=torch.float64)))
        n_in = w
    return MLPController(layers, history=history, hidden="tanh", output="logistic", out_scale=0.06)


def make_env(n, seed):
    import torch
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    e = BatchedT1DSimEnv(patient=["child#001", "adult#001"] * (n // 2), sensor="Dexcom", dtype=torch.float64, seed=seed,
                         random_init_bg=True, integrator="dopri5")
    e.restart_done(mask=torch.ones(n, dtype=torch.uint8, device=e.device), days=DAYS, reset_outputs=True)
    return e


def run_leg(leg, n, pol, K, warm_steps, sigma, seed):
    import torch
    e = make_env(n, seed)
    state = e.collect_mlp_dopri5(warm_steps, pol, on_done="restart", days=DAYS) if warm_steps else e.new_policy_state(pol)
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    finished = torch.zeros((), dtype=torch.int64, device=e.device)

    def go():
        nonlocal finished
        if leg == "collect":
            tr = e.new_trace(K, columns=COLUMNS, history=pol.history)
            e.collect_mlp_dopri5(K, pol, sigma=sigma, policy_state=state, trace=tr, on_done="restart", days=DAYS)
            finished = tr["done"][1:].sum()
        elif leg == "loop":
            tr = e.new_trace(K, columns=COLUMNS[:5])
            rew, don = [], []
            for _ in range(K):
                e.rollout_mlp_dopri5(1, pol, policy_state=state, trace=tr)
                done = e.done.bool()
                rew.append(e.reward.clone()); don.append(e.done.clone())
                e.restart_done(days=DAYS)
                state["cgm_hist"].copy_(torch.where(done, e.cgm, state["cgm_hist"]))
                state["ins_hist"].copy_(torch.where(done, zero, state["ins_hist"]))
                state["prev_meal"].copy_(torch.where(done, zero, state["prev_meal"]))
            tr["reward"], tr["done"] = torch.stack(rew), torch.stack(don)
            finished = tr["done"].sum()
        elif leg == "plain":
            e.collect_mlp_dopri5(K, pol, policy_state=state)
        else:
            e.rollout_mlp_dopri5(K, pol, policy_state=state)
    go()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    go()
    t1.record()
    torch.cuda.synchronize()
    dt = 1e-3 * t0.elapsed_time(t1)
    status = e.sync(raise_on_status=False)
    rate = float(finished) / (K * n)
    e.close()
    del e
    torch.cuda.empty_cache()
    return {"ms": 1e3 * dt, "status": status, "finish_rate": rate}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--policies", nargs="+", default=["net", "hypo"], choices=["net", "hypo"])
    ap.add_argument("--legs", nargs="+", default=["collect", "loop", "plain", "rollout"], choices=["collect", "loop", "plain", "rollout"])
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warm-steps", type=int, default=160, help="steps before the timed window, so that episodes end inside it")
    ap.add_argument("--sigma", type=float, default=0.05, help="exploration std of the collect leg (pre-output space); 0 = none")
    ap.add_argument("--hypo-basal", type=float, default=0.05, help="U/min of the hypo policy: less insulin, fewer episodes end per step")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("collect_exact_bench.py measures on the GPU: none found")
    results = []
    for kind in args.policies:
        pol = make_policy(kind, basal=args.hypo_basal)
        # the constant policy stays constant: noise on 0.05 U/min would be another workload
        sigma = None if kind == "hypo" or args.sigma <= 0 else args.sigma
        for n in args.n:
            runs = {leg: [] for leg in args.legs}
            for _ in range(args.reps):
                for leg in args.legs:
                    runs[leg].append(run_leg(leg, n, pol, args.steps, args.warm_steps, sigma, args.seed))
            res = {"policy": kind, "hypo_basal": args.hypo_basal if kind == "hypo" else None, "n_envs": n, "dtype": "float64",
                   "steps": args.steps, "warm_steps": args.warm_steps, "sigma": sigma, "sensor": "Dexcom", "integrator": "dopri5", "label": args.label,
                   "device": torch.cuda.get_device_name(0), "legs": {}}
            for leg, rr in runs.items():
                ms = sorted(r["ms"] for r in rr)
                res["legs"][leg] = {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1], "ms_runs": [r["ms"] for r in rr],
                                    "status": max(r["status"] for r in rr), "finish_rate": rr[-1]["finish_rate"],
                                    "finish_rate_runs": [r["finish_rate"] for r in rr]}
            med = {leg: v["ms_median"] for leg, v in res["legs"].items()}
            if "collect" in med and "loop" in med:
                res["loop_over_collect"] = med["loop"] / med["collect"]
            if "plain" in med and "rollout" in med:
                res["plain_over_rollout"] = med["plain"] / med["rollout"]
                res["plain_minus_rollout_ms"] = med["plain"] - med["rollout"]
            print(json.dumps(res), flush=True)
            results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
