"""The exact-mode trajectory collector on the GPU (BatchedT1DSimEnv.collect_mlp_dopri5 -> t1d_collect_mlp_dopri5,
csrc/t1d_dopri5.hpp): pinned bit for bit to rollout_mlp_dopri5 (no noise, no episode ends) and to the per-step loop of
rollout_mlp_dopri5(1), restart_done and the torch reset of the policy state (episodes that end, lanes of a wave in different
steps and episodes); the draws replayed through t1d_philox_normals; the noisy step teacher-forced through step(); the top of
the policy's range; cut, shard and neighbour invariance; the argument checks; a solver that gives up.
fp64, Dexcom.  The gym envs, policies, comparisons and reference loops are those of test_gpu_collect.py with exact=True, the
host-noise envs those of test_gpu_policy_dopri5.py: all from support.py."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import support
from support import (DAYS, EPISODE_STATS, MLP_TRACE, POLICY_STATE, ST, STATS, TRACES, bits as _bits,
                     constant_policy as _constant_policy, draw_of_pair as _draw_of_pair, episode_stats as _episode_stats,
                     exact_inputs as _inputs, gpu_torch as _torch, host_noise_env as _env,
                     hypo_leaning_policies as _hypo_leaning_policies, random_policy as _policy, same_dicts as _same_dicts,
                     same_env as _same_env, stats as _stats)

pytestmark = pytest.mark.gpu
STATE = support.STATE_EXACT
GYM_STATE = support.GYM_STATE + ("h_carry",)
_mk_gym = functools.partial(support.gym_env, exact=True)              # fp64 unless told otherwise
_restart_pair = functools.partial(support.restart_pair, exact=True)
_noisy_run = functools.partial(support.noisy_run, exact=True)


# ---------------------------------------------------------------------------------------------------------- 1
def test_without_noise_and_episode_ends_it_is_rollout_mlp_dopri5_bit_for_bit():
    torch = _torch()
    n, K = 192, 60
    inp = _inputs(n, K)
    pol = _policy(widths=(16, 1), n_policies=3, seed=1)             # three weight sets of 64 envs
    a, b, c = _env(*inp), _env(*inp), _env(*inp)
    sa, ta = _stats(a), a.new_trace(K, columns=MLP_TRACE)
    st = a.rollout_mlp_dopri5(20, pol, stats=sa, trace=ta)
    nfa = a.nfev.long().clone()
    a.rollout_mlp_dopri5(K - 20, pol, policy_state=st, stats=sa, trace=ta)
    nfa += a.nfev
    assert a.sync() == 0
    sb, tb = _stats(b), b.new_trace(K, columns=MLP_TRACE + ("reward", "done", "eps"))
    sb2 = b.collect_mlp_dopri5(20, pol, stats=sb, trace=tb)
    nfb = b.nfev.long().clone()
    assert b.collect_mlp_dopri5(K - 20, pol, policy_state=sb2, stats=sb, trace=tb, sigma=None, on_done="continue") is sb2
    nfb += b.nfev
    assert b.sync() == 0
    _same_env(a, b, STATE)
    _same_dicts(st, sb2, POLICY_STATE)
    _same_dicts(sa, sb, STATS)
    _same_dicts(ta, tb, MLP_TRACE)
    assert torch.equal(nfa, nfb)
    assert tb["row"] == K + 1 and float(tb["insulin"][1:].max()) > 0 and float(tb["action"][1:].std(dim=0).max()) > 0
    assert bool((tb["cho"][1:] > 0).any()) and bool((tb["eps"][1:] == 0).all())
    sc = None
    for s in range(1, K + 1):                                       # reward and done of every step
        sc = c.rollout_mlp_dopri5(1, pol, policy_state=sc)
        assert torch.equal(_bits(tb["reward"][s]), _bits(c.reward)), s
        assert torch.equal(tb["done"][s], c.done), s
    assert c.sync() == 0
    _same_env(a, c, STATE)
    assert float(tb["reward"][1:].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------- 2
def test_restart_is_the_loop_of_existing_entry_points_bit_for_bit():
    """400 Dexcom steps under a constant 0.05 U/min (episodes end low) in launches of 150 and 250 steps, and 400 steps without
    insulin (episodes end high), each launch cut again at 240 simulated minutes."""
    restarts_lo, low_lo, high_lo = _restart_pair(_constant_policy(0.05), (150, 250))
    restarts_hi, low_hi, high_hi = _restart_pair(_constant_policy(0.0), (400,))
    print("\nrestarted envs %d / %d of 256, max restarts per env %d / %d, endings < 70: %d / %d, > 350: %d / %d"
          % ((restarts_lo > 0).sum(), (restarts_hi > 0).sum(), restarts_lo.max(), restarts_hi.max(), low_lo, low_hi, high_lo, high_hi))
    # asserted on the reference loop, so that the comparison cannot pass on nothing
    assert (restarts_lo > 0).sum() >= 0.05 * 256
    assert restarts_lo.max() >= 2
    assert high_lo + high_hi > 0


# ---------------------------------------------------------------------------------------------------------- 3
def test_exploration_draws_are_keyed_by_env_episode_and_clock():
    torch = _torch()
    n, K, warm, explore_seed = 256, 40, 150, 0x1234ABCD5678
    pol = _constant_policy(0.05)
    e = _mk_gym(n)
    st = e.collect_mlp_dopri5(warm, pol, on_done="restart", days=DAYS)
    ep0, t0 = e.episode.cpu().numpy().astype(np.int64), e.t.cpu().numpy().astype(np.int64)
    tr = e.new_trace(K, columns=("done", "eps"))
    e.collect_mlp_dopri5(K, pol, sigma=0.3, explore_seed=explore_seed, policy_state=st, trace=tr, on_done="restart", days=DAYS)
    assert e.sync() == 0
    done = tr["done"][1:].cpu().numpy().astype(np.int64)
    eps = tr["eps"][1:]
    k, m = np.empty((K, n), np.int64), np.empty((K, n), np.int64)
    ep, t = ep0.copy(), t0.copy()
    for s in range(K):
        k[s], m[s] = ep, t
        ep = ep + done[s]
        t = np.where(done[s] != 0, 0, t + ST)
    assert np.array_equal(ep, e.episode.cpu().numpy()) and np.array_equal(t, e.t.cpu().numpy())
    assert done.sum() > 0 and k.max() >= 2 and (m[1:] == 0).any()       # steps after a restart inside the launch
    d = _draw_of_pair(m)
    want = np.empty((K, n))
    normals = {}
    for kk in np.unique(k):
        out = torch.empty(int(d.max()) + 1, n, dtype=torch.float64, device=e.device)
        with torch.cuda.device(e.device):
            assert e._L.t1d_philox_normals(e._ctx, explore_seed, e.env_offset, n, int(kk), 0, out.shape[0],
                                           C.c_void_p(out.data_ptr()), e._stream()) == 0
        normals[int(kk)] = out.cpu().numpy()
        sel = k == kk
        want[sel] = normals[int(kk)][d[sel], np.broadcast_to(np.arange(n), (K, n))[sel]]
    assert torch.equal(_bits(eps), _bits(torch.as_tensor(want, dtype=torch.float64).to(e.device)))
    assert not torch.equal(eps[:, 0], eps[:, 1]) and not torch.equal(eps[0], eps[1])
    assert len(torch.unique(eps)) > 0.99 * eps.numel()
    assert 0.9 < float(eps.std()) < 1.1 and abs(float(eps.mean())) < 0.05
    tr0 = e.new_trace(3, columns=("eps",))                              # without sigma no draw is made and the rows are 0
    e.collect_mlp_dopri5(3, pol, policy_state=st, trace=tr0, on_done="restart", days=DAYS)
    assert e.sync() == 0 and bool((tr0["eps"][1:] == 0).all())


# ---------------------------------------------------------------------------------------------------------- 4
def test_with_noise_the_step_is_the_exact_mode_step_on_the_recorded_action():
    """A: warm-up and 120 traced steps in two launches, two policies with their own sigma, restarts on.  B: the same envs
    driven by step(recorded action, 0) + restart_done over the whole run: state, h_carry, the output rows and the restart
    outputs bit for bit.  The recorded action against the host's ordered forward pass on the recorded features plus sigma eps,
    and the recorded features against MLPController.features of the policy state rebuilt from B, at the fp64 bounds of
    tests/test_gpu_collect.py::test_action_and_features_are_what_the_contract_says (1e-13 of the output range; features
    0 .. 2 H bit for bit, the two time-of-day features within 1e-14)."""
    torch = _torch()
    from simglucose_amd.controller.mlp_ctrller import MLPController
    n, warm, K, P = 128, 150, 120, 2
    pol = _hypo_leaning_policies(P, widths=(8, 8, 1))
    H = pol.history
    pre = MLPController(list(zip(pol.W, pol.b)), history=H, hidden=pol.hidden, output="identity", out_scale=1.0, out_bias=0.0)
    sigma = torch.tensor([0.1, 0.4], dtype=torch.float64)
    A, B = _mk_gym(n), _mk_gym(n)
    z = lambda: torch.zeros(n, dtype=torch.float64, device=A.device)
    terma, esa, termb, esb = z(), _episode_stats(A), z(), _episode_stats(B)
    tr = A.new_trace(warm + K, columns=TRACES, history=H)
    kw = dict(sigma=sigma, explore_seed=17, trace=tr, on_done="restart", days=DAYS, terminal_obs=terma, episode_stats=esa)
    st = A.collect_mlp_dopri5(warm, pol, **kw)
    A.collect_mlp_dopri5(K, pol, policy_state=st, **kw)
    assert A.sync() == 0
    sg = sigma.repeat_interleave(n // P).to(A.device)
    zero = z()
    cgm_hist, ins_hist, meal = B.cgm.unsqueeze(0).repeat(H, 1), torch.zeros(H, n, dtype=torch.float64, device=B.device), z()
    worst = worst_tod = 0.0
    restarted_in_window = 0
    for s in range(1, warm + K + 1):
        if s > warm:
            feat = tr["features"][s]
            y = pre.forward(feat, ordered=True)
            want = pol.out_scale * (y + sg * tr["eps"][s]) + pol.out_bias
            worst = max(worst, float((tr["action"][s] - want).abs().max()))
            minute = B.start_minute + B.t
            ref = pol.features(cgm_hist, ins_hist, meal, minute)
            assert torch.equal(_bits(feat[:2 * H + 1]), _bits(ref[:2 * H + 1])), s
            ang = (minute % 1440).double() * (2.0 * math.pi / 1440.0)
            worst_tod = max(worst_tod, float((feat[2 * H + 1] - torch.sin(ang)).abs().max()),
                            float((feat[2 * H + 2] - torch.cos(ang)).abs().max()))
        B.step(tr["action"][s], zero)
        for key, t in (("cgm", B.cgm), ("bg", B.bg), ("cho", B.meal), ("insulin", B.insulin), ("reward", B.reward), ("done", B.done)):
            assert torch.equal(_bits(tr[key][s]), _bits(t)), (key, s)
        done = B.done.bool()
        pol.shift(cgm_hist, ins_hist, B.cgm, B.insulin)
        meal = B.meal.clone()
        B.restart_done(days=DAYS, terminal_obs=termb, episode_stats=esb)
        cgm_hist = torch.where(done, B.cgm, cgm_hist); ins_hist = torch.where(done, zero, ins_hist); meal = torch.where(done, zero, meal)
        if s > warm:
            restarted_in_window += int(done.sum())
    assert B.sync() == 0
    _same_env(B, A, keys=GYM_STATE + ("episode",))
    _same_dicts(esb, esa, EPISODE_STATS)
    assert torch.equal(_bits(termb), _bits(terma))
    _same_dicts({"cgm_hist": cgm_hist, "ins_hist": ins_hist, "prev_meal": meal}, st, POLICY_STATE)
    print("\nmax |action - host| = %.3e U/min (out_scale %.2f), max |time-of-day feature - sin, cos| = %.3e, %d restarts in the window"
          % (worst, pol.out_scale, worst_tod, restarted_in_window))
    assert restarted_in_window > 0
    assert worst <= pol.out_scale * 1e-13
    assert worst_tod <= 1e-14
    assert float(tr["action"][warm + 1:].std()) > 0 and float(tr["eps"][warm + 1:].std()) > 0.5


# ---------------------------------------------------------------------------------------------------------- 5
def test_top_of_the_range():
    """H = 12, widths (32, 32, 32, 1): 56 rows per lane -- the workgroup shrinks.  Restarts on; the loop of test 2.  The envs
    start 150 steps into a hypo-leaning run, so that episodes end within the 60 steps."""
    pol = _hypo_leaning_policies(1, history=12, widths=(32, 32, 32, 1), hidden="relu")
    restarts, low, high = _restart_pair(pol, (150, 60))
    assert (restarts > 0).sum() > 0


# ---------------------------------------------------------------------------------------------------------- 6
def test_cuts_shards_and_neighbours_change_nothing_with_noise_and_restarts_on():
    torch = _torch()
    from simglucose_amd.controller.mlp_ctrller import MLPController
    n, epp, K = 256, 128, 40
    pol = _hypo_leaning_policies(n // epp)
    sigma = torch.tensor([0.1, 0.4], dtype=torch.float64)
    runs = []
    for chunks, kw2 in (((K,), {"max_minutes_per_launch": 10 ** 6}), ((10,) * 4, {}), ((1, 39), {}), ((K,), {"max_minutes_per_launch": 21})):
        e = _mk_gym(n)
        runs.append((e,) + _noisy_run(e, pol, sigma, 150, chunks, **kw2))
    e0, st0, stats0, es0, tr0 = runs[0]
    assert int(tr0["done"][1:].sum()) > 0 and int(e0.episode.max()) >= 2
    more = EPISODE_STATS + ("terminal_obs", "nfev")
    for e, st, stats, es, tr in runs[1:]:
        _same_env(e0, e, keys=GYM_STATE + ("episode",))
        _same_dicts(st0, st, POLICY_STATE)
        _same_dicts(stats0, stats, STATS)
        _same_dicts(es0, es, more)
        _same_dicts(tr0, tr, TRACES)
    for a, b in ((0, 128), (128, 256)):
        pa, pb = a // epp, b // epp
        sub = MLPController([(W[pa:pb], bb[pa:pb]) for W, bb in zip(pol.W, pol.b)], history=pol.history, hidden=pol.hidden,
                            output=pol.output, out_scale=pol.out_scale, out_bias=pol.out_bias)
        e = _mk_gym(b - a, env_offset=a)
        s2, stats2, es2, tr2 = _noisy_run(e, sub, sigma[pa:pb], 150, (K,))
        sl = slice(a, b)
        _same_env(e0, e, GYM_STATE + ("episode",), sl)
        _same_dicts(st0, s2, POLICY_STATE, sl)
        _same_dicts(stats0, stats2, STATS, sl)
        _same_dicts(es0, es2, more, sl)
        _same_dicts(tr0, tr2, TRACES, sl)


# ---------------------------------------------------------------------------------------------------------- 7
def test_rejections_change_nothing():
    torch = _torch()
    from simglucose_amd import _lib
    e = _mk_gym(128)
    pol = _policy(history=3, widths=(8, 1))
    e.collect_mlp_dopri5(2, pol, on_done="restart", days=DAYS)        # a state with a carried step in it
    st = e.new_policy_state(pol)
    params = pol.flat_params().to(e.device)
    other_time, other_amt = e.meal_time.clone(), e.meal_amt.clone()
    scratch = torch.zeros(13, e.n, dtype=torch.float64, device=e.device)
    tr = e.new_trace(2, columns=TRACES, history=pol.history)
    keys = GYM_STATE + ("episode",)
    before = {k: getattr(e, k).clone() for k in keys}
    before.update({k: v.clone() for k, v in st.items()})
    before.update({"tr_" + k: tr[k].clone() for k in TRACES})
    assert bool((before["h_carry"] != 0).all())
    L = e._L

    def mlp(env=e, state=st, prm=params):
        p = _lib.Mlp()
        pol.fill_struct(p)
        p.n_policies, p.envs_per_policy, p.n_params = 1, env.n, prm.shape[1]
        p.params = prm.data_ptr()
        for k in POLICY_STATE:
            setattr(p, k, state[k].data_ptr())
        p.start_minute = env.start_minute.data_ptr()
        for k, f in (("bg", "bg_trace"), ("cgm", "cgm_trace"), ("cho", "cho_trace"), ("insulin", "insulin_trace"), ("action", "action_trace")):
            setattr(p, f, tr[k].data_ptr())
        p.trace_row = 1
        return p

    def restart(env=e):
        r = _lib.Restart()
        r.days, r.random_init_bg, r.reset_outputs, r.reserved = DAYS, 1, 0, 0
        r.meal_time, r.meal_amt, r.start_minute = env.meal_time.data_ptr(), env.meal_amt.data_ptr(), env.start_minute.data_ptr()
        return r

    def collect(r, on_done=1):
        g = _lib.Collect()
        g.explore_seed, g.on_done, g.reserved = 7, on_done, 0
        g.restart = C.pointer(r) if r is not None else None
        for k, f in (("reward", "reward_trace"), ("done", "done_trace"), ("eps", "eps_trace"), ("features", "feat_trace")):
            setattr(g, f, tr[k].data_ptr())
        return g

    def batch(env=e, **kw):
        b = _lib.Batch()
        C.memmove(C.byref(b), C.byref(env._b), C.sizeof(b))
        for k, v in kw.items():
            setattr(b, k, v)
        return b

    def call(p, g, b=None, n_steps=2, minutes=3, h_carry=e.h_carry, env=e):
        with torch.cuda.device(env.device):
            return L.t1d_collect_mlp_dopri5(env._ctx, C.byref(b if b is not None else env._b), C.byref(p) if p is not None else None,
                                            C.byref(g) if g is not None else None,
                                            C.c_void_p(h_carry.data_ptr() if h_carry is not None else None), None, n_steps, minutes,
                                            env._stream())
    r = restart()
    bad = []
    # whatever t1d_rollout_mlp_dopri5 rejects
    for field, value in (("history", 0), ("history", 13), ("n_layers", 5), ("hidden_act", 2), ("params", None), ("cgm_hist", None),
                         ("n_policies", 2), ("envs_per_policy", 64), ("n_params", params.shape[1] + 1)):
        p = mlp(); setattr(p, field, value)
        for on_done in (0, 1):
            bad.append(("mlp." + field, value, p, collect(r, on_done), None, {}))
    bad += [("mlp", None, None, collect(r), None, {}), ("n_steps", 0, mlp(), collect(r), None, {"n_steps": 0}),
            ("minutes", 0, mlp(), collect(r), None, {"minutes": 0}), ("minutes", 100001, mlp(), collect(r), None, {"minutes": 100001}),
            ("h_carry", None, mlp(), collect(r), None, {"h_carry": None}),
            ("batch.cho", "set", mlp(), collect(r), batch(cho=scratch.data_ptr()), {})]
    # whatever t1d_collect_mlp rejects of collect
    bad += [("batch.episode", None, mlp(), collect(r), batch(episode=None), {}),
            ("batch.normals", "set", mlp(), collect(r), batch(normals=scratch.data_ptr(), n_normals=13), {}),
            ("batch.x0_override", "set", mlp(), collect(r), batch(x0_override=scratch.data_ptr()), {})]
    keep = [r]
    for field, value in (("meal_time", other_time.data_ptr()), ("meal_amt", other_amt.data_ptr()), ("meal_time", None),
                         ("start_minute", None), ("days", 3), ("days", 0), ("reserved", 1), ("h_carry", scratch.data_ptr())):
        r2 = restart(); setattr(r2, field, value); keep.append(r2)
        bad.append(("restart." + field, value, mlp(), collect(r2), None, {}))
    bad += [("collect.on_done", 2, mlp(), collect(r, 2), None, {}), ("collect.on_done", -1, mlp(), collect(r, -1), None, {}),
            ("collect.restart", None, mlp(), collect(None, 1), None, {}), ("collect", None, mlp(), None, None, {})]
    p = mlp(); p.start_minute = scratch.data_ptr()
    bad.append(("mlp.start_minute", "not restart.start_minute", p, collect(r), None, {}))
    for on_done in (0, 1):
        g = collect(r, on_done); g.reserved = 1; bad.append(("collect.reserved", 1, mlp(), g, None, {}))
    for what, value, p, g, b, kw in bad:
        assert call(p, g, b, **kw) == -1, (what, value)
        assert L.t1d_last_error().startswith(b"t1d_collect_mlp_dopri5: "), (what, value, L.t1d_last_error())
        assert len(L.t1d_last_error()) > len(b"t1d_collect_mlp_dopri5: "), (what, value)
    # an fp32 batch
    f32 = _mk_gym(128, exact=False, dtype=torch.float32)
    st32, prm32 = f32.new_policy_state(pol), params.float()
    keys32 = ("state", "istate", "cgm", "bg")
    before32 = {k: getattr(f32, k).clone() for k in keys32}
    hc32 = torch.full((128,), 0.25, dtype=torch.float64, device=f32.device)
    g32 = _lib.Collect(); g32.explore_seed = 7
    p32 = mlp(f32, st32, prm32); p32.bg_trace = p32.cgm_trace = p32.cho_trace = p32.insulin_trace = p32.action_trace = None
    assert call(p32, g32, env=f32, h_carry=hc32) == -1 and b"fp64" in L.t1d_last_error()
    assert f32.sync() == 0
    for k in keys32:
        assert torch.equal(getattr(f32, k), before32[k]), k
    assert bool((hc32 == 0.25).all())
    # host normals with restart, through the method; the two methods on the wrong kind of env
    hn = _env(*_inputs(64, 4))
    with pytest.raises(_lib.T1DError, match="host normals"):
        hn.collect_mlp_dopri5(2, pol, on_done="restart")
    with pytest.raises(_lib.T1DError, match="collect_mlp_dopri5"):
        e.collect_mlp(2, pol)
    with pytest.raises(_lib.T1DError, match="dopri5"):
        f32.collect_mlp_dopri5(2, pol)
    with pytest.raises(ValueError):
        e.collect_mlp_dopri5(2, _policy(n_policies=4))              # 128 envs / 4 = 32 per policy
    with pytest.raises(ValueError):
        e.collect_mlp_dopri5(0, pol)
    with pytest.raises(ValueError):
        e.collect_mlp_dopri5(2, pol, on_done="stop")
    with pytest.raises(ValueError):
        e.collect_mlp_dopri5(2, pol, trace={"row": 0, "done": torch.zeros(4, e.n, dtype=torch.float64, device=e.device)})
    assert e.sync() == 0
    for k in keys:
        assert torch.equal(getattr(e, k), before[k]), k
    for k in st:
        assert torch.equal(st[k], before[k]), k
    for k in TRACES:
        assert torch.equal(_bits(tr[k]), _bits(before["tr_" + k])), k
    # and the good ones run: restart->h_carry NULL or the call's own
    r5 = restart(); r5.h_carry = e.h_carry.data_ptr()
    assert call(mlp(), collect(r, 1)) == 0 and call(mlp(), collect(r5, 1)) == 0 and call(mlp(), collect(None, 0)) == 0 and e.sync() == 0
    assert int(e.t.max()) == 8 * ST


# ---------------------------------------------------------------------------------------------------------- 8
def test_solver_failure_inside_a_collection():
    """kabs x 1e6 for one env in three (tests/test_gpu_policy_dopri5.py::test_solver_failure_inside_a_rollout): the status bit,
    a finite state, and the normal envs as if the stiff ones were not there.  Without noise: a draw is keyed by the env's id,
    which differs between the two batches."""
    torch = _torch()
    from simglucose_amd import _lib
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    from oracle import t1d_oracle as O
    names, tab = O.patient_table()
    rows = tab[[names.index("adult#001"), names.index("adult#001")]].copy()
    rows[1, O.IDX["kabs"]] *= 1e6
    n, K = 192, 10
    pid = (np.arange(n) % 3 == 1).astype(np.int64)
    normal = np.where(pid == 0)[0]                                  # 128 envs, spread over all three waves
    rs = np.random.RandomState(9)
    z = rs.randn(21, n)
    mt = np.stack([np.full(n, 4), np.full(n, 17)]).astype(np.int64)
    ma = rs.uniform(30.0, 60.0, size=(2, n))
    pol = _policy(widths=(16, 1), seed=5)
    cols = MLP_TRACE + ("reward", "done", "features")
    out = []
    for sel in (np.arange(n), normal):
        e = BatchedT1DSimEnv(patient=pid[sel], patient_table=rows, sensor="Dexcom", noise="host", normals=z[:, sel], integrator="dopri5")
        e.set_meals(torch.as_tensor(mt[:, sel]), torch.as_tensor(ma[:, sel]))
        e.reset()
        tr = e.new_trace(K, columns=cols, history=pol.history)
        e.collect_mlp_dopri5(K, pol, trace=tr)
        out.append((e, tr, e.sync(raise_on_status=False)))
    (ea, tra, sta), (eb, trb, stb) = out
    assert sta & _lib.T1D_ST_SOLVER_FAILED and not (sta & _lib.T1D_ST_NONFINITE), sta
    assert stb == 0
    assert bool(torch.isfinite(ea.x).all()) and int(ea.t.min()) == K * ST == int(ea.t.max())
    nidx = torch.as_tensor(normal, device=ea.device)
    for k in cols:
        assert torch.equal(_bits(tra[k][1:][..., nidx]), _bits(trb[k][1:])), k
    for k in ("x", "t", "cgm", "bg", "reward", "last_cgm", "prev_risk", "planned", "h_carry"):
        assert torch.equal(getattr(ea, k)[..., nidx], getattr(eb, k)), k
    assert bool((trb["cho"][1:] > 0).any()) and float(trb["action"][1:].std(dim=0).max()) > 0
