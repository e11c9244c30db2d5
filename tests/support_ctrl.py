"""What test_gpu_collect_ctrl.py shares: the workloads under which the PID and the basal-bolus controller end episodes, the
collectors' runs (collect_pid / collect_bb in cuts) and their reference, the loop of existing entry points that the header
names.  Imported by bare name beside support.py; importing it touches no device.  Every run is made once per argument set
and shared by the tests: treat what comes back as read-only."""
import functools

from support import DAYS, episode_stats, gpu_torch, gym_env, identity_policy, stats

COLS = ("bg", "cgm", "cho", "insulin", "action", "reward", "done", "features")
CTRL_STATE = {"pid": ("integ", "prev"), "bb": ("basal", "cr", "cf", "prev_meal")}
CTRL_RESET = {"pid": ("integ", "prev"), "bb": ("prev_meal",)}     # what PIDController.reset / BBController.reset zero

# PID workloads: (P, I, D, target).  "stock": gains of the size test_gpu_features.py uses.  "high": no insulin at all, episodes end
# above 350.  "hot": proportional to the CGM itself (target 0), about 0.05 U/min at 150 mg/dL -- the rate at which a constant
# basal ends episodes low (test_gpu_collect.py) -- with small I and D terms so that integ and prev matter after a restart.  On the
# loop of entry points, 400 steps, 256 envs, both dtypes: 212 envs restart, one of them 12 times, 1428 endings below 70 and 4
# above 350.
PID = {"stock": (1.5e-4, 4e-7, 5e-4, 140.0), "high": (0.0, 0.0, 0.0, 140.0), "hot": (3.3e-4, 1e-8, 1e-4, 0.0)}
# basal-bolus workloads: "stock" = bb_constants() for every env; "hot" = envs with global id >= hot_from get basal = 0.05 U/min;
# "high" = no basal and no bolus to speak of (cr = cf = 1e30)


def feature_policy(history=4):
    """the MLPController whose history and scales form the features; its (8, 1) identity network is run by nobody but the
    reference's t1d_mlp_features, which asks for a complete policy"""
    return identity_policy(history=history, widths=(8, 1), seed=5)


def ctrl_state(e, kind, workload, hot_from=128):
    """the controller state of a fresh episode for env e under `workload`, by global env id (so a shard gets its slice)"""
    torch = gpu_torch()
    z = lambda: torch.zeros(e.n, dtype=e.dtype, device=e.device)
    if kind == "pid":
        return {"integ": z(), "prev": z()}
    st = e.bb_constants()
    if workload == "hot":
        gid = torch.arange(e.n, device=e.device) + int(e.env_offset)
        st["basal"] = torch.where(gid >= hot_from, torch.full_like(st["basal"], 0.05), st["basal"]).contiguous()
    elif workload == "high":
        st["basal"] = z(); st["cr"] = z() + 1e30; st["cf"] = z() + 1e30
    st["prev_meal"] = z()
    return st


def _call(e, kind, workload, collect, k, pol, cs, ps, **kw):
    """k steps of the controller: the collector (collect=True) or the roll-out entry point"""
    if kind == "pid":
        P, I, D, target = PID[workload]
        if collect:
            return e.collect_pid(k, P, I, D, target, features=pol, pid_state=cs, policy_state=ps, **kw)
        return e.rollout_pid(k, P, I, D, target, pid_state=cs, **kw), ps
    if collect:
        return e.collect_bb(k, features=pol, bb_state=cs, policy_state=ps, **kw)
    return e.rollout_bb(k, bb_state=cs, **kw), ps


def run_collector(e, kind, workload, pol, cuts, on_done="restart", hot_from=128, cols=COLS):
    """collect_pid / collect_bb on env e in launches of `cuts` steps -> dict(e, cs = controller state, ps = policy state,
    acc, es, term, tr)"""
    torch = gpu_torch()
    K = sum(cuts)
    acc, es, term = stats(e), episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
    tr = e.new_trace(K, columns=cols, history=pol.history)
    cs, ps = ctrl_state(e, kind, workload, hot_from), None
    for k in cuts:
        cs, ps = _call(e, kind, workload, True, k, pol, cs, ps, stats=acc, trace=tr, on_done=on_done, days=DAYS, terminal_obs=term,
                       episode_stats=es)
    assert e.sync() == 0
    assert tr["row"] == K + 1 and (on_done == "continue" or e._clock is None)
    return dict(e=e, cs=cs, ps=ps, acc=acc, es=es, term=term, tr=tr)


def run_loop(e, kind, workload, pol, K, hot_from=128):
    """The loop of entry points of include/t1d.h, K times: t1d_mlp_features; t1d_rollout_pid(1) / t1d_rollout_bb(1) through the
    generic roll-out kernel; the window shift with prev_meal = batch.meal; t1d_restart_done; the reset of windows and controller
    state of the envs that were done.  -> run_collector's dict (tr without "action": the entry points record none) and
    host_feat [K + 1, F, n] = MLPController.features of the windows before every step, first [K + 1, n] = batch.cgm after every
    step's restart, before = {obs, the controller's state words} [K + 1, n] as every step found them, restarts per env, low and
    high endings"""
    torch = gpu_torch()
    e.set_option("rollout_launches", 0)
    acc, es, term = stats(e), episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
    tr = e.new_trace(K, columns=tuple(c for c in COLS if c != "action"), history=pol.history)
    host_feat, first = torch.full_like(tr["features"], float("nan")), torch.full_like(tr["cgm"], float("nan"))
    cs, ps = ctrl_state(e, kind, workload, hot_from), e.new_policy_state(pol)
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    before = {k: torch.full_like(first, float("nan")) for k in ("obs",) + CTRL_RESET[kind]}
    low = high = 0
    for _ in range(K):
        row = tr["row"]
        before["obs"][row] = e.cgm
        for k in CTRL_RESET[kind]:
            before[k][row] = cs[k]
        tr["features"][row] = e.policy_features(pol, ps)
        host_feat[row] = pol.features(ps["cgm_hist"], ps["ins_hist"], ps["prev_meal"], e.start_minute + e.t)
        _call(e, kind, workload, False, 1, pol, cs, ps, stats=acc, trace=tr)
        pol.shift(ps["cgm_hist"], ps["ins_hist"], e.cgm, e.insulin)
        ps["prev_meal"].copy_(e.meal)
        done = e.done.bool()
        tr["reward"][row] = e.reward; tr["done"][row] = e.done
        low = low + (done & (e.bg < 70)).sum(); high = high + (done & (e.bg > 350)).sum()
        e.restart_done(days=DAYS, terminal_obs=term, episode_stats=es)
        first[row] = e.cgm
        ps["cgm_hist"].copy_(torch.where(done, e.cgm, ps["cgm_hist"]))          # new_policy_state for the envs that restarted
        ps["ins_hist"].copy_(torch.where(done, zero, ps["ins_hist"]))
        ps["prev_meal"].copy_(torch.where(done, zero, ps["prev_meal"]))
        for k in CTRL_RESET[kind]:
            cs[k].copy_(torch.where(done, zero, cs[k]))
    assert e.sync() == 0
    return dict(e=e, cs=cs, ps=ps, acc=acc, es=es, term=term, tr=tr, host_feat=host_feat, first=first, before=before,
                restarts=(e.episode - 1).cpu().numpy(), low=int(low), high=int(high))


@functools.lru_cache(maxsize=None)
def loop_run(kind, workload, dtype_name, K, n=256, history=4, hot_from=128):
    torch = gpu_torch()
    return run_loop(gym_env(n, getattr(torch, dtype_name)), kind, workload, feature_policy(history), K, hot_from)


@functools.lru_cache(maxsize=None)
def collector_run(kind, workload, dtype_name, cuts, n=256, history=4, hot_from=128, env_offset=0, on_done="restart"):
    torch = gpu_torch()
    return run_collector(gym_env(n, getattr(torch, dtype_name), env_offset=env_offset), kind, workload, feature_policy(history), cuts,
                         on_done, hot_from)
