"""What test_gpu_collect_ctrl_dopri5.py shares: the exact-mode runs of the controllers' collectors (collect_pid_dopri5 /
collect_bb_dopri5 in cuts) and their reference, the loop of exact-mode entry points that the header names.  Workloads, feature
policy and controller state are support_ctrl.py's.  Imported by bare name beside support.py; importing it touches no device.
Every run is made once per argument set and shared by the tests: treat what comes back as read-only."""
import functools

from support import DAYS, episode_stats, gpu_torch, gym_env, stats
from support_ctrl import COLS, CTRL_RESET, PID, ctrl_state, feature_policy


def call(e, kind, workload, collect, k, pol, cs, ps, **kw):
    """k steps of the controller in the exact mode: the collector (collect=True) or the roll-out entry point"""
    if kind == "pid":
        P, I, D, target = PID[workload]
        if collect:
            return e.collect_pid_dopri5(k, P, I, D, target, features=pol, pid_state=cs, policy_state=ps, **kw)
        return e.rollout_pid_dopri5(k, P, I, D, target, pid_state=cs, **kw), ps
    if collect:
        return e.collect_bb_dopri5(k, features=pol, bb_state=cs, policy_state=ps, **kw)
    return e.rollout_bb_dopri5(k, bb_state=cs, **kw), ps


def run_collector(e, kind, workload, pol, cuts, on_done="restart", hot_from=128, cols=COLS, **kw):
    """collect_pid_dopri5 / collect_bb_dopri5 on env e in calls of `cuts` steps (**kw to them) -> dict(e, cs = controller
    state, ps = policy state, acc, es, term, tr, nfev = RHS evaluations summed over the calls)"""
    torch = gpu_torch()
    K = sum(cuts)
    acc, es, term = stats(e), episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
    tr = e.new_trace(K, columns=cols, history=pol.history)
    cs, ps = ctrl_state(e, kind, workload, hot_from), None
    nf = torch.zeros(e.n, dtype=torch.int64, device=e.device)
    for k in cuts:
        cs, ps = call(e, kind, workload, True, k, pol, cs, ps, stats=acc, trace=tr, on_done=on_done, days=DAYS, terminal_obs=term,
                      episode_stats=es, **kw)
        nf += e.nfev
    assert e.sync() == 0
    assert tr["row"] == K + 1 and (on_done == "continue" or e._clock is None)
    return dict(e=e, cs=cs, ps=ps, acc=acc, es=es, term=term, tr=tr, nfev=nf)


def run_loop(e, kind, workload, pol, K, hot_from=128):
    """The loop of entry points of include/t1d.h, K times: t1d_mlp_features; t1d_rollout_pid_dopri5(1) / t1d_rollout_bb_dopri5(1);
    the window shift with prev_meal = batch.meal; t1d_restart_done with h_carry; the reset of windows and controller state of
    the envs that were done.  -> run_collector's dict (tr without "action": the entry points record none) and first [K + 1, n] =
    batch.cgm after every step's restart, before = {obs, the controller's state words} [K + 1, n] as every step found them,
    restarts per env, low and high endings"""
    torch = gpu_torch()
    acc, es, term = stats(e), episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
    tr = e.new_trace(K, columns=tuple(c for c in COLS if c != "action"), history=pol.history)
    first = torch.full_like(tr["cgm"], float("nan"))
    cs, ps = ctrl_state(e, kind, workload, hot_from), e.new_policy_state(pol)
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    before = {k: torch.full_like(first, float("nan")) for k in ("obs",) + CTRL_RESET[kind]}
    nf = torch.zeros(e.n, dtype=torch.int64, device=e.device)
    low = high = 0
    for _ in range(K):
        row = tr["row"]
        before["obs"][row] = e.cgm
        for k in CTRL_RESET[kind]:
            before[k][row] = cs[k]
        tr["features"][row] = e.policy_features(pol, ps)
        call(e, kind, workload, False, 1, pol, cs, ps, stats=acc, trace=tr)
        nf += e.nfev
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
    return dict(e=e, cs=cs, ps=ps, acc=acc, es=es, term=term, tr=tr, nfev=nf, first=first, before=before,
                restarts=(e.episode - 1).cpu().numpy(), low=int(low), high=int(high))


@functools.lru_cache(maxsize=None)
def loop_run(kind, workload, K, n=256, history=4, hot_from=128):
    return run_loop(gym_env(n, exact=True), kind, workload, feature_policy(history), K, hot_from)


@functools.lru_cache(maxsize=None)
def collector_run(kind, workload, cuts, n=256, history=4, hot_from=128, env_offset=0, on_done="restart", max_minutes_per_launch=240):
    return run_collector(gym_env(n, env_offset=env_offset, exact=True), kind, workload, feature_policy(history), cuts, on_done,
                         hot_from, max_minutes_per_launch=max_minutes_per_launch)
