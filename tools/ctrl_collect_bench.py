"""Cost of collecting K steps of trajectories while the basal-bolus controller drives the envs, fp64 Dexcom, child#001 /
adult#001 with random initial glucose (the envs of tools/collect_bench.py), every trace column, two workloads:
  stock    bb_constants() for every env: almost no episode ends
  hot      the upper half of the envs at basal = 0.05 U/min (the workload of tests/test_gpu_collect_ctrl.py): their episodes end
           low all the time
and two legs:
  collect  collect_bb(K, on_done="restart") with bg, cgm, cho, insulin, action, reward, done, features: one launch
  loop     the entry points that did the same before it (include/t1d.h, t1d_collect_bb): K x (policy_features, rollout_bb(1)
           through the generic roll-out kernel, the window shift, restart_done, the torch reset of windows and prev_meal,
           keeping reward, done and features); the loop has no action column, the roll-out records none
Every leg: fresh env, `warm_steps` steps so that the batch is mixed, one warm-up pass, then K steps between two device
synchronisations (host clock), `reps` times, legs alternated; the median is reported.  `finish_rate` is the share of env-steps of
the timed window that ended an episode.  One JSON line per (workload, batch size); --out writes them as a list.

    python tools/ctrl_collect_bench.py --out profiles/collect/ctrl_collect_bench.json

--exact: the exact mode (DOPRI5) on an integrator="dopri5" env, as tools/collect_bench.py --exact: collect_bb_dopri5 (one launch
per 240 simulated minutes) against the loop of policy_features, rollout_bb_dopri5(1), the window shift, restart_done and the
torch resets, and two more legs:
  plain    collect_bb_dopri5(K, on_done="continue") without a collector column
  rollout  rollout_bb_dopri5(K) of the same build: what `plain` is measured against
K steps between two events on the stream; minimum and maximum are reported beside the median, and `plain_minus_rollout_ms`.
Every repetition builds the same env from the same seed, so the finish rate is the same in each (`finish_rate_runs` shows it).

    python tools/ctrl_collect_bench.py --exact --out profiles/collect/exact_ctrl_collect_bench.json

--limit: what a time limit costs (collect_bb_limit; with --exact collect_bb_dopri5_limit), the legs of tools/collect_bench.py
--limit instead:
  collect       as above: the sibling call, no limit
  limit_far     the limit's kernel with a limit nobody reaches (10^6 steps): the cost of the check, against `collect` of the same run
  limit         max_episode_steps = --limit-steps in the warm steps and in the window: about 1 / limit-steps of the envs are cut per
                step beside those that finish
  loop_limit    the reference loop: `loop` with cut = ~done & (t >= limit), policy_features into cut_features where cut,
                restart_done(mask = done | cut) and the resets for the masked envs, stacking truncated too
`cut_rate` is the share of env-steps of the timed window that were cut.

    python tools/ctrl_collect_bench.py --limit --out profiles/collect/ctrl_limit_bench.json
    python tools/ctrl_collect_bench.py --limit --exact --out profiles/collect/exact_ctrl_limit_bench.json
"""
import argparse

import benchlib
from benchlib import DAYS

COLUMNS = ("bg", "cgm", "cho", "insulin", "action", "reward", "done", "features")


def run_leg(leg, workload, n, pol, K, warm_steps, hot_basal, seed, exact=False):
    import torch
    e = benchlib.mixed_env(n, seed, integrator="dopri5" if exact else None, options=[("rollout_launches", 0)])
    collect, rollout = (e.collect_bb_dopri5, e.rollout_bb_dopri5) if exact else (e.collect_bb, e.rollout_bb)
    bb = e.bb_constants()
    if workload == "hot":
        bb["basal"][n // 2:] = hot_basal
    bb["prev_meal"] = torch.zeros(n, dtype=e.dtype, device=e.device)
    state = e.new_policy_state(pol)
    if warm_steps:
        collect(warm_steps, features=pol, bb_state=bb, policy_state=state, on_done="restart", days=DAYS)
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    finished = torch.zeros((), dtype=torch.int64, device=e.device)

    def go():
        nonlocal finished
        if leg == "collect":
            tr = e.new_trace(K, columns=COLUMNS, history=pol.history)
            collect(K, features=pol, bb_state=bb, policy_state=state, trace=tr, on_done="restart", days=DAYS)
            finished = tr["done"][1:].sum()
        elif leg == "plain":
            collect(K, features=pol, bb_state=bb, policy_state=state)
        elif leg == "rollout":
            rollout(K, bb_state=bb)
        else:
            tr = e.new_trace(K, columns=COLUMNS[:4])
            rew, don, feat = [], [], []
            for _ in range(K):
                feat.append(e.policy_features(pol, state))
                rollout(1, bb_state=bb, trace=tr)
                pol.shift(state["cgm_hist"], state["ins_hist"], e.cgm, e.insulin)
                state["prev_meal"].copy_(e.meal)
                done = e.done.bool()
                rew.append(e.reward.clone()); don.append(e.done.clone())
                e.restart_done(days=DAYS)
                state["cgm_hist"].copy_(torch.where(done, e.cgm, state["cgm_hist"]))
                state["ins_hist"].copy_(torch.where(done, zero, state["ins_hist"]))
                state["prev_meal"].copy_(torch.where(done, zero, state["prev_meal"]))
                bb["prev_meal"].copy_(torch.where(done, zero, bb["prev_meal"]))
            tr["reward"], tr["done"], tr["features"] = torch.stack(rew), torch.stack(don), torch.stack(feat)
            finished = tr["done"].sum()
    ms = benchlib.timed_leg(go, go, "events" if exact else "host")
    status = benchlib.close_leg(e)
    rate = float(finished) / (K * n)
    del e, collect, rollout                      # the bound methods hold the env too
    torch.cuda.empty_cache()
    return {"ms": ms, "status": status, "finish_rate": rate}


LIMIT_LEGS = ("collect", "limit_far", "limit", "loop_limit")


def run_limit_leg(leg, workload, n, pol, K, warm_steps, hot_basal, seed, exact, limit_steps):
    import torch
    e = benchlib.mixed_env(n, seed, integrator="dopri5" if exact else None, options=[("rollout_launches", 0)])
    plain, limited, rollout = (e.collect_bb_dopri5, e.collect_bb_dopri5_limit, e.rollout_bb_dopri5) if exact else \
        (e.collect_bb, e.collect_bb_limit, e.rollout_bb)
    L = {"limit_far": 10 ** 6, "limit": limit_steps, "loop_limit": limit_steps}.get(leg)
    bb = e.bb_constants()
    if workload == "hot":
        bb["basal"][n // 2:] = hot_basal
    bb["prev_meal"] = torch.zeros(n, dtype=e.dtype, device=e.device)
    state = e.new_policy_state(pol)
    cut_features = torch.zeros(2 * pol.history + 3, n, dtype=e.dtype, device=e.device)

    def collect(k, **kw):                       # the sibling call, or the one with the limit
        if L is None:
            return plain(k, features=pol, bb_state=bb, policy_state=state, on_done="restart", days=DAYS, **kw)
        return limited(k, L, cut_features, features=pol, bb_state=bb, policy_state=state, days=DAYS, **kw)
    left = warm_steps
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
            collect(K, trace=tr)
            finished = tr["done"][1:].sum()
            cuts = tr["truncated"][1:].sum() if L is not None else cuts
            return
        tr = e.new_trace(K, columns=COLUMNS[:4])
        rew, don, trn, feat = [], [], [], []
        for _ in range(K):
            feat.append(e.policy_features(pol, state))
            rollout(1, bb_state=bb, trace=tr)
            pol.shift(state["cgm_hist"], state["ins_hist"], e.cgm, e.insulin)
            state["prev_meal"].copy_(e.meal)
            done = e.done.bool()
            cut = ~done & (e.t >= L * e.minutes_per_step)
            rew.append(e.reward.clone()); don.append(e.done.clone()); trn.append(cut)
            cut_features.copy_(torch.where(cut, e.policy_features(pol, state), cut_features))
            mask = done | cut
            e.restart_done(mask=mask, days=DAYS)
            state["cgm_hist"].copy_(torch.where(mask, e.cgm, state["cgm_hist"]))
            state["ins_hist"].copy_(torch.where(mask, zero, state["ins_hist"]))
            state["prev_meal"].copy_(torch.where(mask, zero, state["prev_meal"]))
            bb["prev_meal"].copy_(torch.where(mask, zero, bb["prev_meal"]))
        tr["reward"], tr["done"], tr["truncated"], tr["features"] = torch.stack(rew), torch.stack(don), torch.stack(trn), torch.stack(feat)
        finished, cuts = tr["done"].sum(), tr["truncated"].sum()
    ms = benchlib.timed_leg(go, go, "events" if exact else "host")
    status = benchlib.close_leg(e)
    rates = float(finished) / (K * n), float(cuts) / (K * n)
    del e, plain, limited, rollout              # the bound methods hold the env too
    torch.cuda.empty_cache()
    return {"ms": ms, "status": status, "finish_rate": rates[0], "cut_rate": rates[1]}


def limit_main(args, pol):
    import torch
    results = []
    for workload in args.workloads:
        for n in args.n:
            runs = benchlib.alternate(LIMIT_LEGS, args.reps,
                                      lambda leg: run_limit_leg(leg, workload, n, pol, args.steps, args.warm_steps, args.hot_basal,
                                                                args.seed, args.exact, args.limit_steps))
            res = {"controller": "bb", "workload": workload, "hot_basal": args.hot_basal if workload == "hot" else None, "n_envs": n,
                   "dtype": "float64", "steps": args.steps, "warm_steps": args.warm_steps, "limit_steps": args.limit_steps,
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
            benchlib.emit(results, res)
    benchlib.write(results, args.out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--workloads", nargs="+", default=["stock", "hot"], choices=["stock", "hot"])
    ap.add_argument("--legs", nargs="+", default=None, choices=["collect", "loop", "plain", "rollout"],
                    help="default: collect loop; with --exact also plain rollout, which only the exact mode has")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warm-steps", type=int, default=160, help="steps before the timed window, so that episodes end inside it")
    ap.add_argument("--hot-basal", type=float, default=0.05, help="U/min of the upper half of the envs on the hot workload")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--label", default=None)
    ap.add_argument("--exact", action="store_true", help="the legs in the exact mode (integrator='dopri5'), timed with events")
    ap.add_argument("--limit", action="store_true", help="the legs of a time limit (collect_bb_limit; with --exact collect_bb_dopri5_limit) instead")
    ap.add_argument("--limit-steps", type=int, default=48, help="max_episode_steps of the limit and loop_limit legs (>= --steps)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.limit and args.limit_steps < args.steps:
        ap.error("--limit needs --limit-steps >= --steps")
    if args.legs is None:
        args.legs = ["collect", "loop", "plain", "rollout"] if args.exact else ["collect", "loop"]
    if not args.exact and set(args.legs) & {"plain", "rollout"}:
        ap.error("the plain and rollout legs belong to --exact")
    benchlib.require_gpu("ctrl_collect_bench.py")
    import torch
    # only history and the feature scales matter to collect_bb; policy_features (the loop) asks for a complete network
    pol = benchlib.constant_policy(4, 0.0)
    if args.limit:
        return limit_main(args, pol)
    results = []
    for workload in args.workloads:
        for n in args.n:
            runs = benchlib.alternate(args.legs, args.reps,
                                      lambda leg: run_leg(leg, workload, n, pol, args.steps, args.warm_steps, args.hot_basal, args.seed,
                                                          args.exact))
            res = {"controller": "bb", "workload": workload, "hot_basal": args.hot_basal if workload == "hot" else None, "n_envs": n,
                   "dtype": "float64", "steps": args.steps, "warm_steps": args.warm_steps, "sensor": "Dexcom"}
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
                res["plain_minus_rollout_ms"] = med["plain"] - med["rollout"]
            benchlib.emit(results, res)
    benchlib.write(results, args.out)


if __name__ == "__main__":
    main()
