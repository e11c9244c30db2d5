"""What test_time_limit_all_host.py and test_gpu_time_limit_all.py share: the five collectors that got a time limit after
collect_mlp_limit -- collect_pid_limit, collect_bb_limit (fixed-step), collect_mlp_dopri5_limit, collect_pid_dopri5_limit,
collect_bb_dopri5_limit (exact) -- their runs in cuts, and their reference, the loop of existing entry points with the cut mask
that include/t1d.h names.  Workloads, feature policy and controller state are support_ctrl.py's.  Imported by bare name beside
support.py; importing it touches no device.  Every run is made once per argument set and shared by the tests: treat what comes
back as read-only."""
import functools

import support
import support_ctrl
import support_ctrl_exact
from support import DAYS, ST, episode_stats, gpu_torch, gym_env, stats

# method -> (its sibling without the limit, the arguments in front of max_episode_steps, the sibling's parameter behind which
# the sibling's list goes on, exact mode?)
METHODS = {"collect_pid_limit": ("collect_pid", ("n_steps", "P", "I", "D"), "target", False),
           "collect_bb_limit": ("collect_bb", ("n_steps",), "target", False),
           "collect_mlp_dopri5_limit": ("collect_mlp_dopri5", ("n_steps", "policy"), "sigma", True),
           "collect_pid_dopri5_limit": ("collect_pid_dopri5", ("n_steps", "P", "I", "D"), "target", True),
           "collect_bb_dopri5_limit": ("collect_bb_dopri5", ("n_steps",), "target", True)}
ENTRY_POINTS = tuple("t1d_" + m for m in METHODS)
SENTINEL = -77.0
CTRL_COLS = support_ctrl.COLS + ("truncated",)
MLP_COLS = support.MLP_TRACE + ("reward", "done", "eps", "features", "truncated")
ENV_KEYS = support.STATE + ("meal_time", "meal_amt", "start_minute", "episode", "cgm0")
SIGMA, EXPLORE_SEED = 0.3, 0xC0FFEE
FAR = 10 ** 6                                 # a limit nobody reaches


def front(method, n_steps, pol):
    """the positional arguments of `method` in front of max_episode_steps, with the "hot" PID gains and the policy `pol`"""
    P, I, D, _ = support_ctrl.PID["hot"]
    return {"n_steps": (n_steps,), "P": (P,), "I": (I,), "D": (D,), "policy": (pol,)}, METHODS[method][1]


def call_limit(e, method, n_steps, L, cut_features=None, pol=None, **kw):
    """e.<method>(n_steps, [P, I, D | policy], L, cut_features, **kw); the controllers get pol as features="""
    words, names = front(method, n_steps, pol)
    args = sum((words[k] for k in names), ())
    if "policy" not in names and pol is not None:
        kw.setdefault("features", pol)
    if "P" in names:
        kw.setdefault("target", support_ctrl.PID["hot"][3])
    return getattr(e, method)(*args, L, cut_features, **kw)


def limit_mode_refusal(method):
    """support.mode_refusal for a *_limit method: the T1DError text with which it turns away an env of the other mode, a bare
    object that has its integrator and nothing else.  Needs no device."""
    import pytest
    from simglucose_amd import _lib
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    e = object.__new__(BatchedT1DSimEnv)
    e.integrator = None if METHODS[method][3] else "dopri5"
    with pytest.raises(_lib.T1DError) as err:
        call_limit(e, method, 1, 10)
    return str(err.value)


def sentinel(e, history=4):
    torch = gpu_torch()
    return torch.full((2 * history + 3, e.n), SENTINEL, dtype=e.dtype, device=e.device)


def env(n, dtype_name="float64", exact=False, env_offset=0):
    torch = gpu_torch()
    return gym_env(n, getattr(torch, dtype_name), env_offset=env_offset, exact=exact)


# ------------------------------------------------------------------------------------------------ the controllers
def ctrl_method(kind, exact, limit=True):
    return "collect_%s%s%s" % (kind, "_dopri5" if exact else "", "_limit" if limit else "")


def ctrl_loop(e, kind, pol, K, L, exact, hot_from=128):
    """The loop of entry points under the "hot" workload, K times: policy_features; rollout_pid(1) / rollout_bb(1) with
    rollout_launches = 0, or rollout_*_dopri5(1); the window shift with prev_meal = batch.meal; cut = ~done & (t >= L ST);
    policy_features where cut; restart_done(mask = done | cut); the torch reset of windows, prev_meal and controller state of the
    masked envs -> dict(e, cs, ps, acc, es, term, tr (no "action": the entry points record none), cut_features, nfev)"""
    torch = gpu_torch()
    if not exact:
        e.set_option("rollout_launches", 0)
    call = support_ctrl_exact.call if exact else support_ctrl._call
    acc, es, term = stats(e), episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
    tr = e.new_trace(K, columns=tuple(c for c in CTRL_COLS if c != "action"), history=pol.history)
    cs, ps = support_ctrl.ctrl_state(e, kind, "hot", hot_from), e.new_policy_state(pol)
    cut_features = sentinel(e, pol.history)
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    nf = torch.zeros(e.n, dtype=torch.int64, device=e.device)
    for _ in range(K):
        row = tr["row"]
        tr["features"][row] = e.policy_features(pol, ps)
        call(e, kind, "hot", False, 1, pol, cs, ps, stats=acc, trace=tr)
        nf += e.nfev if exact else 0
        pol.shift(ps["cgm_hist"], ps["ins_hist"], e.cgm, e.insulin)
        ps["prev_meal"].copy_(e.meal)
        done = e.done.bool()
        tr["reward"][row] = e.reward; tr["done"][row] = e.done
        cut = ~done & (e.t >= L * ST)
        tr["truncated"][row] = cut
        cut_features.copy_(torch.where(cut, e.policy_features(pol, ps), cut_features))
        mask = done | cut
        e.restart_done(mask=mask, days=DAYS, terminal_obs=term, episode_stats=es)
        ps["cgm_hist"].copy_(torch.where(mask, e.cgm, ps["cgm_hist"]))          # new_policy_state for the envs that restarted
        ps["ins_hist"].copy_(torch.where(mask, zero, ps["ins_hist"]))
        ps["prev_meal"].copy_(torch.where(mask, zero, ps["prev_meal"]))
        for k in support_ctrl.CTRL_RESET[kind]:
            cs[k].copy_(torch.where(mask, zero, cs[k]))
    assert e.sync() == 0
    return dict(e=e, cs=cs, ps=ps, acc=acc, es=es, term=term, tr=tr, cut_features=cut_features, nfev=nf)


def ctrl_collector(e, kind, pol, cuts, L, exact, hot_from=128, **kw):
    """collect_<kind>[_dopri5]_limit under the "hot" workload in calls of `cuts` steps (**kw to them); L = None: the sibling
    without a limit, on_done="restart" -> ctrl_loop's dict"""
    torch = gpu_torch()
    K = sum(cuts)
    acc, es, term = stats(e), episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
    tr = e.new_trace(K, columns=CTRL_COLS, history=pol.history)
    cs, ps = support_ctrl.ctrl_state(e, kind, "hot", hot_from), None
    cut_features = sentinel(e, pol.history)
    nf = torch.zeros(e.n, dtype=torch.int64, device=e.device)
    common = dict(stats=acc, trace=tr, days=DAYS, terminal_obs=term, episode_stats=es, **kw)
    for k in cuts:
        if L is None:
            cs, ps = (support_ctrl_exact.call if exact else support_ctrl._call)(e, kind, "hot", True, k, pol, cs, ps, on_done="restart",
                                                                                **common)
        else:
            key = "pid_state" if kind == "pid" else "bb_state"
            cs, ps = call_limit(e, ctrl_method(kind, exact), k, L, cut_features, pol=pol, policy_state=ps, **{key: cs}, **common)
        nf += e.nfev if exact else 0
    assert e.sync() == 0
    assert tr["row"] == K + 1 and e._clock is None
    return dict(e=e, cs=cs, ps=ps, acc=acc, es=es, term=term, tr=tr, cut_features=cut_features, nfev=nf)


def ctrl_same(A, B, kind, exact, sl=slice(None), action=True):
    """run B is the envs `sl` of run A, bit for bit: env state (h_carry in the exact mode), policy windows, controller state,
    accumulators, episode statistics, terminal_obs, cut_features, every trace column both runs have, and the summed nfev"""
    support.same_env(A["e"], B["e"], keys=ENV_KEYS + (("h_carry",) if exact else ()), sl=sl)
    support.same_dicts(A["ps"], B["ps"], support.POLICY_STATE, sl=sl)
    support.same_dicts(A["cs"], B["cs"], support_ctrl.CTRL_STATE[kind], sl=sl)
    support.same_dicts(A["acc"], B["acc"], support.STATS, sl=sl)
    support.same_dicts(A["es"], B["es"], support.EPISODE_STATS, sl=sl)
    support.same_dicts(A, B, ("term", "cut_features", "nfev"), sl=sl)
    support.same_dicts(A["tr"], B["tr"], tuple(c for c in CTRL_COLS if action or c != "action"), sl=sl)
    assert A["tr"]["row"] == B["tr"]["row"]


@functools.lru_cache(maxsize=None)
def ctrl_first_ending(kind, dtype_name, exact):
    """s*, the first row in which any env terminates in the no-limit reference loop (support_ctrl's / support_ctrl_exact's
    400-step loop under "hot", the run their own test files share), and the first env that terminates there"""
    ref = support_ctrl_exact.loop_run(kind, "hot", 400) if exact else support_ctrl.loop_run(kind, "hot", dtype_name, 400)
    return first_ending(ref["tr"]["done"], "%s %s%s" % (kind, dtype_name, " exact" if exact else ""))


def first_ending(done, what):
    rows = done.bool().any(dim=1).nonzero().flatten()
    assert rows.numel() > 0, "no env terminates"
    s = int(rows[0])
    print("\n[time limit %s] first termination in row s* = %d (%d envs)" % (what, s, int(done[s].sum())))
    assert 2 <= s <= 300, s
    return s, int(done[s].nonzero().flatten()[0])


def launches(s):
    return tuple(k for k in (s, s - 2, 5) if k > 0)


@functools.lru_cache(maxsize=None)
def ctrl_limited(kind, dtype_name, exact, n=256, env_offset=0, max_minutes_per_launch=None):
    """the collector under max_episode_steps = s* in launches of (s*, s* - 2, 5) steps on n envs from env_offset"""
    s, _ = ctrl_first_ending(kind, dtype_name, exact)
    kw = {} if max_minutes_per_launch is None else dict(max_minutes_per_launch=max_minutes_per_launch)
    return ctrl_collector(env(n, dtype_name, exact, env_offset), kind, support_ctrl.feature_policy(), launches(s), s, exact, **kw)


@functools.lru_cache(maxsize=None)
def ctrl_limited_loop(kind, dtype_name, exact):
    s, _ = ctrl_first_ending(kind, dtype_name, exact)
    return ctrl_loop(env(256, dtype_name, exact), kind, support_ctrl.feature_policy(), 2 * s + 3, s, exact)


# ------------------------------------------------------------------------------------------------ the exact MLP collector
def mlp_policy(kind):
    """plain: 0.05 U/min whatever the net sees; noisy: two hypo-leaning weight sets, run with sigma = 0.3"""
    return support.constant_policy(0.05) if kind == "plain" else support.hypo_leaning_policies(2)


def mlp_sigma(kind):
    return SIGMA if kind == "noisy" else None


def mlp_loop(e, pol, K, L, sigma):
    """What a trainer does without the limit's collector in the exact mode, K times: the one-step call (rollout_mlp_dopri5(1);
    with sigma collect_mlp_dopri5(1, on_done="continue")), cut = ~done & (t >= L ST), policy_features where cut,
    restart_done(mask = done | cut), the torch reset of the masked envs' windows.  L = None: no limit -> dict(e, st, acc, es,
    term, tr, cut_features, nfev)"""
    torch = gpu_torch()
    st = e.new_policy_state(pol)
    acc, es, term = stats(e), episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
    tr = e.new_trace(K, columns=MLP_COLS, history=pol.history)
    cut_features = sentinel(e, pol.history)
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    nf = torch.zeros(e.n, dtype=torch.int64, device=e.device)
    for _ in range(K):
        row = tr["row"]
        if sigma is None:
            tr["features"][row] = e.policy_features(pol, st)
            e.rollout_mlp_dopri5(1, pol, policy_state=st, stats=acc, trace=tr)
            tr["reward"][row] = e.reward; tr["done"][row] = e.done; tr["eps"][row] = 0
        else:
            e.collect_mlp_dopri5(1, pol, sigma=sigma, explore_seed=EXPLORE_SEED, policy_state=st, stats=acc, trace=tr, on_done="continue")
        nf += e.nfev
        done = e.done.bool()
        cut = ~done & (e.t >= L * ST) if L is not None else torch.zeros_like(done)
        tr["truncated"][row] = cut
        if L is not None:
            cut_features.copy_(torch.where(cut, e.policy_features(pol, st), cut_features))
        mask = done | cut
        e.restart_done(mask=mask, days=DAYS, terminal_obs=term, episode_stats=es)
        st["cgm_hist"].copy_(torch.where(mask, e.cgm, st["cgm_hist"]))             # new_policy_state for the envs that restarted
        st["ins_hist"].copy_(torch.where(mask, zero, st["ins_hist"]))
        st["prev_meal"].copy_(torch.where(mask, zero, st["prev_meal"]))
    assert e.sync() == 0
    return dict(e=e, st=st, acc=acc, es=es, term=term, tr=tr, cut_features=cut_features, nfev=nf)


def mlp_collector(e, pol, cuts, L, sigma, **kw2):
    """collect_mlp_dopri5_limit in calls of `cuts` steps (**kw2 to them); L = None: collect_mlp_dopri5(on_done="restart")
    -> the same dict"""
    torch = gpu_torch()
    acc, es, term = stats(e), episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
    tr = e.new_trace(sum(cuts), columns=MLP_COLS, history=pol.history)
    cut_features = sentinel(e, pol.history)
    nf = torch.zeros(e.n, dtype=torch.int64, device=e.device)
    st = None
    kw = dict(sigma=sigma, explore_seed=EXPLORE_SEED, stats=acc, trace=tr, days=DAYS, terminal_obs=term, episode_stats=es, **kw2)
    for k in cuts:
        if L is not None:
            st = e.collect_mlp_dopri5_limit(k, pol, L, cut_features, policy_state=st, **kw)
        else:                                                                        # no limit: "truncated" stays 0
            st = e.collect_mlp_dopri5(k, pol, policy_state=st, on_done="restart", **kw)
        nf += e.nfev
    assert e.sync() == 0
    assert e._clock is None
    return dict(e=e, st=st, acc=acc, es=es, term=term, tr=tr, cut_features=cut_features, nfev=nf)


def mlp_same(A, B, sl=slice(None)):
    """run B is the envs `sl` of run A, bit for bit"""
    support.same_env(A["e"], B["e"], keys=ENV_KEYS + ("h_carry",), sl=sl)
    support.same_dicts(A["st"], B["st"], support.POLICY_STATE, sl=sl)
    support.same_dicts(A["acc"], B["acc"], support.STATS, sl=sl)
    support.same_dicts(A["es"], B["es"], support.EPISODE_STATS, sl=sl)
    support.same_dicts(A, B, ("term", "cut_features", "nfev"), sl=sl)
    support.same_dicts(A["tr"], B["tr"], MLP_COLS, sl=sl)
    assert A["tr"]["row"] == B["tr"]["row"]


@functools.lru_cache(maxsize=None)
def mlp_first_ending(kind):
    """s* of the exact MLP collector under the policy of `kind`: the no-limit reference loop, 300 steps from the common start"""
    tr = mlp_loop(env(256, exact=True), mlp_policy(kind), 300, None, mlp_sigma(kind))["tr"]
    return first_ending(tr["done"], "mlp %s exact" % kind)


@functools.lru_cache(maxsize=None)
def mlp_limited(kind, n=256, env_offset=0, max_minutes_per_launch=None, half=None):
    """the exact MLP collector under max_episode_steps = s* in launches of (s*, s* - 2, 5) steps; half: weight set `half` alone"""
    s, _ = mlp_first_ending(kind)
    pol = mlp_policy(kind)
    if half is not None:
        pol = type(pol)([(w[half:half + 1], b[half:half + 1]) for w, b in zip(pol.W, pol.b)], history=pol.history, hidden=pol.hidden,
                        output=pol.output, out_scale=pol.out_scale, out_bias=pol.out_bias)
    kw = {} if max_minutes_per_launch is None else dict(max_minutes_per_launch=max_minutes_per_launch)
    return mlp_collector(env(n, exact=True, env_offset=env_offset), pol, launches(s), s, mlp_sigma(kind), **kw)


@functools.lru_cache(maxsize=None)
def mlp_limited_loop(kind):
    s, _ = mlp_first_ending(kind)
    return mlp_loop(env(256, exact=True), mlp_policy(kind), 2 * s + 3, s, mlp_sigma(kind))


# ------------------------------------------------------------------------------------------------ what the comparison covers
def check_reference(B, s, i0, n=256):
    """the preconditions on the reference loop alone, so that no comparison passes on nothing"""
    done, trunc = B["tr"]["done"].bool(), B["tr"]["truncated"].bool()
    assert int((done & trunc).sum()) == 0                                             # never both
    assert not bool(done[:s].any()) and not bool(trunc[:s].any())
    assert bool(done[s, i0]) and not bool(trunc[s, i0])                               # done wins in the row of the limit
    assert bool((trunc[s] | done[s]).all()) and int(trunc[s].sum()) == n - int(done[s].sum()) > 0   # every other env is cut there
    assert int(trunc[2 * s].sum()) > 0                                                # second cuts, mid-launch (row s* closes a launch)
    assert bool((trunc[2 * s] | done[s + 1:2 * s + 1].any(dim=0)).all())
    sent = support.bits(sentinel(B["e"]))
    written = (support.bits(B["cut_features"]) != sent).any(dim=0)
    assert bool((written == trunc.any(dim=0)).all())                                  # written for cut envs only
    assert int(B["es"]["last_length"].max()) <= s and int((B["es"]["last_length"] == s).sum()) > 0
