"""Cost of collecting K steps of trajectories for a policy-gradient trainer, fp64 Dexcom, child#001 / adult#001 with random
initial glucose (the envs of tools/autoreset_bench.py), two policies:
  net      a random 2 x 16 tanh net with logistic output on [0, 0.06] U/min, with exploration noise (1.3 % of the envs end per step)
  hypo     a constant 0.05 U/min (--hypo-basal): episodes end low all the time, 1.6 % of the envs per step once the batch is
           mixed; less insulin, fewer endings -- the sweep behind the break-even rate in profiles/collect/README.md
and four legs:
  collect  collect_mlp(K, on_done="restart") with all traces: one launch
  loop     what did the same before it: K x (rollout_mlp(1), restart_done, the torch reset of the policy windows, stacking
           reward and done)
  plain    collect_mlp(K, on_done="continue", sigma=None), no new trace
  rollout  rollout_mlp(K): what `plain` must not be slower than
Every leg: fresh env, `warm_steps` steps so that the batch is mixed, one warm-up pass, then K steps between two device
synchronisations (host clock), `reps` times, legs alternated; the median is reported.  The timed window holds what a caller
pays per batch of K steps, the allocation of the trace included.  `finish_rate` is the share of env-steps of the timed window
that ended an episode.  One JSON line per (policy, batch size); --out writes them as a list.

    python tools/collect_bench.py --out profiles/collect/collect_bench.json

--exact: the same legs in the exact mode (DOPRI5) on an integrator="dopri5" env: collect_mlp_dopri5 (one launch per 240
simulated minutes) and rollout_mlp_dopri5, K steps between two events on the stream; minimum and maximum are reported beside
the median, and `plain_minus_rollout_ms`.  Every repetition builds the same env from the same seed, so the finish rate is the
same in each (`finish_rate_runs` shows it).

    python tools/collect_bench.py --exact --out profiles/collect/exact_collect_bench.json

--limit: what a time limit costs (collect_mlp_limit, t1d_collect_mlp_limit), fixed-step mode, these legs instead:
  collect       as above: today's call, no limit
  limit_far     the same call with a limit nobody reaches (10^6 steps): the cost of the check, against `collect` of the same run
  limit         max_episode_steps = --limit-steps in the warm steps and in the window: the envs' clocks are spread by then, and
                about 1 / limit-steps of them are cut per step beside those that finish
  loop_limit    the reference loop: K x (the one-step call, cut = ~done & (t >= limit), policy_features into cut_features where
                cut, restart_done(mask = done | cut), the torch reset of the windows, stacking reward, done and truncated)
  collect_sync  `collect` on envs that all start together (no warm steps)
  limit_sync    the launch that holds the step in which envs that started together are all cut at once: no warm steps,
                max_episode_steps = K, so the last step of the window cuts every env that has not finished
`cut_rate` is the share of env-steps of the timed window that were cut.

    python tools/collect_bench.py --limit --policies net --out profiles/collect/limit_bench.json

--limit --exact: the first four of those legs in the exact mode (collect_mlp_dopri5_limit, t1d_collect_mlp_dopri5_limit; the loop's
one-step call is rollout_mlp_dopri5(1), with noise collect_mlp_dopri5(1)), between two events on the stream.

    python tools/collect_bench.py --limit --exact --policies hypo --out profiles/collect/exact_limit_bench.json
"""
import argparse

import benchlib
from benchlib import DAYS

COLUMNS = ("bg", "cgm", "cho", "insulin", "action", "reward", "done", "eps", "features")


def make_policy(kind, history=4, basal=0.05):
    if kind == "hypo":
        return benchlib.constant_policy(history, basal)
    return benchlib.random_policy(history, (16, 16, 1), hidden="tanh", output="logistic", out_scale=0.06)


def run_leg(leg, n, pol, K, warm_steps, sigma, seed, exact):
    import torch
    e = benchlib.mixed_env(n, seed, integrator="dopri5" if exact else None)
    collect, rollout = (e.collect_mlp_dopri5, e.rollout_mlp_dopri5) if exact else (e.collect_mlp, e.rollout_mlp)
    state = collect(warm_steps, pol, on_done="restart", days=DAYS) if warm_steps else e.new_policy_state(pol)
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    finished = torch.zeros((), dtype=torch.int64, device=e.device)

    def go():
        nonlocal finished
        if leg == "collect":
            tr = e.new_trace(K, columns=COLUMNS, history=pol.history)
            collect(K, pol, sigma=sigma, policy_state=state, trace=tr, on_done="restart", days=DAYS)
            finished = tr["done"][1:].sum()
        elif leg == "loop":
            tr = e.new_trace(K, columns=COLUMNS[:5])
            rew, don = [], []
            for _ in range(K):
                rollout(1, pol, policy_state=state, trace=tr)
                done = e.done.bool()
                rew.append(e.reward.clone()); don.append(e.done.clone())
                e.restart_done(days=DAYS)
                state["cgm_hist"].copy_(torch.where(done, e.cgm, state["cgm_hist"]))
                state["ins_hist"].copy_(torch.where(done, zero, state["ins_hist"]))
                state["prev_meal"].copy_(torch.where(done, zero, state["prev_meal"]))
            tr["reward"], tr["done"] = torch.stack(rew), torch.stack(don)
            finished = tr["done"].sum()
        elif leg == "plain":
            collect(K, pol, policy_state=state)
        else:
            rollout(K, pol, policy_state=state)
    ms = benchlib.timed_leg(go, go, "events" if exact else "host")
    status = benchlib.close_leg(e)
    rate = float(finished) / (K * n)
    del e, collect, rollout                      # the bound methods hold the env too
    torch.cuda.empty_cache()
    return {"ms": ms, "status": status, "finish_rate": rate}


LIMIT_LEGS = ("collect", "limit_far", "limit", "loop_limit", "collect_sync", "limit_sync")


def run_limit_leg(leg, n, pol, K, warm_steps, sigma, seed, limit_steps, exact=False):
    import torch
    e = benchlib.mixed_env(n, seed, integrator="dopri5" if exact else None)
    plain, limited, rollout = (e.collect_mlp_dopri5, e.collect_mlp_dopri5_limit, e.rollout_mlp_dopri5) if exact else \
        (e.collect_mlp, e.collect_mlp_limit, e.rollout_mlp)
    sync = leg.endswith("_sync")
    L = {"limit_far": 10 ** 6, "limit": limit_steps, "loop_limit": limit_steps, "limit_sync": K}.get(leg)
    cut_features = torch.zeros(2 * pol.history + 3, n, dtype=e.dtype, device=e.device)

    def collect(k, **kw):                       # today's call, or the one with the limit
        if L is None:
            return plain(k, pol, policy_state=state, on_done="restart", days=DAYS, **kw)
        return limited(k, pol, L, cut_features, policy_state=state, days=DAYS, **kw)
    state = e.new_policy_state(pol)
    left = 0 if sync else warm_steps
    while left:                                 # a call with a limit takes at most max_episode_steps steps
        k = min(left, L or left)
        collect(k)
        left -= k
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    finished = cuts = torch.zeros((), dtype=torch.int64, device=e.device)

    def go():
        nonlocal finished, cuts
        if leg != "loop_limit":
            tr = e.new_trace(K, columns=COLUMNS + (("truncated",) if L is not None else ()), history=pol.history)
            collect(K, sigma=sigma, trace=tr)
            finished = tr["done"][1:].sum()
            cuts = tr["truncated"][1:].sum() if L is not None else cuts
            return
        tr = e.new_trace(K, columns=COLUMNS if sigma is not None else COLUMNS[:5], history=pol.history)
        rew, don, trn = [], [], []
        for _ in range(K):
            if sigma is not None:
                plain(1, pol, sigma=sigma, policy_state=state, trace=tr)
            else:
                rollout(1, pol, policy_state=state, trace=tr)
            done = e.done.bool()
            cut = ~done & (e.t >= L * e.minutes_per_step)
            rew.append(e.reward.clone()); don.append(e.done.clone()); trn.append(cut)
            cut_features.copy_(torch.where(cut, e.policy_features(pol, state), cut_features))
            mask = done | cut
            e.restart_done(mask=mask, days=DAYS)
            state["cgm_hist"].copy_(torch.where(mask, e.cgm, state["cgm_hist"]))
            state["ins_hist"].copy_(torch.where(mask, zero, state["ins_hist"]))
            state["prev_meal"].copy_(torch.where(mask, zero, state["prev_meal"]))
        tr["reward"], tr["done"], tr["truncated"] = torch.stack(rew), torch.stack(don), torch.stack(trn)
        finished, cuts = tr["done"].sum(), tr["truncated"].sum()
    ms = benchlib.timed_leg(go, go, "events" if exact else "host")
    status = benchlib.close_leg(e)
    rates = float(finished) / (K * n), float(cuts) / (K * n)
    del e, plain, limited, rollout              # the bound methods hold the env too
    torch.cuda.empty_cache()
    return {"ms": ms, "status": status, "finish_rate": rates[0], "cut_rate": rates[1]}


def limit_main(args):
    import torch
    results = []
    for kind in args.policies:
        pol = make_policy(kind, basal=args.hypo_basal)
        sigma = None if kind == "hypo" or args.sigma <= 0 else args.sigma
        for n in args.n:
            legs = LIMIT_LEGS[:4] if args.exact else LIMIT_LEGS
            runs = benchlib.alternate(legs, args.reps, lambda leg: run_limit_leg(leg, n, pol, args.steps, args.warm_steps, sigma,
                                                                               args.seed, args.limit_steps, args.exact))
            res = {"policy": kind, "hypo_basal": args.hypo_basal if kind == "hypo" else None, "n_envs": n, "dtype": "float64",
                   "steps": args.steps, "warm_steps": args.warm_steps, "limit_steps": args.limit_steps, "sigma": sigma,
                   "sensor": "Dexcom"}
            if args.exact:
                res["integrator"] = "dopri5"
            res.update({"label": args.label, "device": torch.cuda.get_device_name(0), "legs": {}})
            for leg, rr in runs.items():
                res["legs"][leg] = {**benchlib.summarise([r["ms"] for r in rr], "ms", spread=True), "status": max(r["status"] for r in rr),
                                    "finish_rate": rr[-1]["finish_rate"], "cut_rate": rr[-1]["cut_rate"]}
            med = {leg: v["ms_median"] for leg, v in res["legs"].items()}
            res["limit_far_over_collect"] = med["limit_far"] / med["collect"]
            res["limit_over_collect"] = med["limit"] / med["collect"]
            res["loop_limit_over_limit"] = med["loop_limit"] / med["limit"]
            if "limit_sync" in med:
                res["limit_sync_over_collect_sync"] = med["limit_sync"] / med["collect_sync"]
            benchlib.emit(results, res)
    benchlib.write(results, args.out)


def main(argv=None):
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
    ap.add_argument("--exact", action="store_true", help="the four legs in the exact mode (integrator='dopri5'), timed with events")
    ap.add_argument("--limit", action="store_true", help="the legs of a time limit (collect_mlp_limit; with --exact collect_mlp_dopri5_limit) instead")
    ap.add_argument("--limit-steps", type=int, default=48, help="max_episode_steps of the limit and loop_limit legs (>= --steps)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    benchlib.require_gpu("collect_bench.py")
    if args.limit:
        if args.limit_steps < args.steps:
            raise SystemExit("--limit needs --limit-steps >= --steps")
        return limit_main(args)
    import torch
    results = []
    for kind in args.policies:
        pol = make_policy(kind, basal=args.hypo_basal)
        # the constant policy stays constant: noise on 0.05 U/min would be another workload
        sigma = None if kind == "hypo" or args.sigma <= 0 else args.sigma
        for n in args.n:
            runs = benchlib.alternate(args.legs, args.reps,
                                      lambda leg: run_leg(leg, n, pol, args.steps, args.warm_steps, sigma, args.seed, args.exact))
            res = {"policy": kind, "hypo_basal": args.hypo_basal if kind == "hypo" else None, "n_envs": n, "dtype": "float64",
                   "steps": args.steps, "warm_steps": args.warm_steps, "sigma": sigma, "sensor": "Dexcom"}
            if args.exact:
                res["integrator"] = "dopri5"
            res.update({"label": args.label, "device": torch.cuda.get_device_name(0), "legs": {}})
            for leg, rr in runs.items():
                res["legs"][leg] = {**benchlib.summarise([r["ms"] for r in rr], "ms", spread=args.exact),
                                    "status": max(r["status"] for r in rr), "finish_rate": rr[-1]["finish_rate"]}
                if args.exact:
                    res["legs"][leg]["finish_rate_runs"] = [r["finish_rate"] for r in rr]
            med = {leg: v["ms_median"] for leg, v in res["legs"].items()}
            if "collect" in med and "loop" in med:
                res["loop_over_collect"] = med["loop"] / med["collect"]
            if "plain" in med and "rollout" in med:
                res["plain_over_rollout"] = med["plain"] / med["rollout"]
                if args.exact:
                    res["plain_minus_rollout_ms"] = med["plain"] - med["rollout"]
            benchlib.emit(results, res)
    benchlib.write(results, args.out)


if __name__ == "__main__":
    main()
