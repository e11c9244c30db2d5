"""GPU suite of the patient-relative policy output: basal = fma(scale[i], g(y), bias[i]) with a scale and a bias per env
(t1d_rollout_mlp_rel, t1d_collect_mlp_rel, t1d_rollout_mlp_dopri5_rel, t1d_mlp_action_rel; MLPController(relative_to="basal")).
  1  ONE weight set with last bias 1 and meal_bolus=140 is rollout_bb / rollout_bb_dopri5 for a mixed cohort, bit for bit
  2  a single-patient cohort equals the plain call under out_scale basal, out_bias basal
  3  the roll-out is the loop of policy_action, policy_bolus and step(u, bolus), fixed step and exact
  4  the action word is scale * y in torch, bit for bit (identity output, out_bias 0)
  5  the collector with noise and restarts against the loop of one-step entry points
  6  collect_mlp_dopri5 refuses such a policy and touches nothing; the library refuses a wrong split"""
import ctypes as C

import numpy as np
import pytest

import support

pytestmark = pytest.mark.gpu

# Test 1: 320 envs -- one full 256-thread workgroup and a 64-lane remainder -- of the patients (2, 7, 13, 21, 28) interleaved lane
# by lane (patient_idx[i] = P[i % 5]), so every wave holds all five.  Seed and the meal tables of support.exact_inputs (four
# meals of 15 - 90 g per env) were run through the CPU oracle's basal-bolus loop in this layout beforehand: over 100 fixed-step
# steps 799 bolus steps start from CGM > 150 and 469 from CGM <= 150, 30 412 steps are meal-free (exact mode, 60 steps: 879, 354
# and 17 647).
PATIENTS = (2, 7, 13, 21, 28)
SEED = 3
TARGET = 140.0
N1 = 320


def _mixed_inputs(K):
    _, z, mt, ma = support.exact_inputs(N1, K, seed=SEED)
    return np.array(PATIENTS)[np.arange(N1) % len(PATIENTS)], z, mt, ma


def _unit_net(**kw):
    """one zero-weight weight set with identity output whose last bias is 1: under relative_to="basal" every env's own basal rate"""
    torch = support.gpu_torch()
    from simglucose_amd.controller.mlp_ctrller import MLPController
    H = 4
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    return MLPController([(z(8, 2 * H + 3), z(8)), (z(1, 8), torch.ones(1, dtype=torch.float64))], history=H, output="identity",
                         out_scale=1.0, out_bias=0.0, relative_to="basal", **kw)


def _bb_pair(dtype, exact, K, cuts):
    torch = support.gpu_torch()
    inp = _mixed_inputs(K)
    kw = {} if dtype is None else {"dtype": dtype}
    A, B = (support.host_noise_env(*inp, exact=exact, **kw) for _ in range(2))
    pol = _unit_net(meal_bolus=TARGET)
    assert pol.n_policies == 1
    basal = B.bb_constants()["basal"]
    assert len(set(basal[:64].tolist())) == len(PATIENTS) and float(basal.max() / basal.min()) > 1.5     # every wave is mixed
    sa, sb = support.stats(A), support.stats(B)
    ta, tb = A.new_trace(K), B.new_trace(K)
    pa = pb = None
    nfa, nfb = (torch.zeros(A.n, dtype=torch.int64, device=A.device) for _ in range(2))
    for k in cuts:
        if exact:
            pa = A.rollout_mlp_dopri5(k, pol, policy_state=pa, stats=sa, trace=ta)
            pb = B.rollout_bb_dopri5(k, target=TARGET, bb_state=pb, stats=sb, trace=tb)
            nfa += A.nfev; nfb += B.nfev
        else:
            pa = A.rollout_mlp(k, pol, policy_state=pa, stats=sa, trace=ta)
            pb = B.rollout_bb(k, target=TARGET, bb_state=pb, stats=sb, trace=tb)
    assert A.sync() == 0 and B.sync() == 0
    # what happened, on rollout_bb's side: step r >= 2 starts from the observation and the announced meal of row r - 1
    pm, obs = tb["cho"][1:K], tb["cgm"][1:K]
    hi, lo, free = int(((pm > 0) & (obs > 150)).sum()), int(((pm > 0) & (obs <= 150)).sum()), int((pm == 0).sum())
    print("\n[policy rel] %s %s: bolus steps from CGM > 150: %d, <= 150: %d, meal-free steps: %d"
          % ("exact" if exact else "fixed", A.dtype, hi, lo, free), end="")
    assert hi > 0 and lo > 0 and free > 0
    support.same_env(A, B, support.STATE_EXACT if exact else support.STATE)
    support.same_dicts(sa, sb, support.STATS)
    support.same_dicts(ta, tb, ("bg", "cgm", "cho", "insulin"))
    assert torch.equal(support.bits(pa["prev_meal"]), support.bits(pb["prev_meal"]))
    assert torch.equal(nfa, nfb) and (not exact or int(nfa.min()) > 0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_one_weight_set_is_rollout_bb_for_a_mixed_cohort_bit_for_bit(dtype):
    """320 envs, five patients interleaved, Dexcom, 100 steps cut as 40 + 60: env state, outputs, accumulators, the four trace
    columns and prev_meal of rollout_mlp under ONE unit network with relative_to="basal" and meal_bolus=140 are rollout_bb's"""
    torch = support.gpu_torch()
    _bb_pair(getattr(torch, dtype), False, 100, (40, 60))


def test_one_weight_set_is_rollout_bb_dopri5_for_a_mixed_cohort_bit_for_bit():
    """the same in the exact mode, 60 steps: rollout_mlp_dopri5 against rollout_bb_dopri5, h_carry and nfev included"""
    _bb_pair(None, True, 60, (60,))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_single_patient_cohort_equals_the_plain_call(dtype):
    """128 envs of one patient, a random 16-wide policy with logistic output and out_bias != 0, 40 steps: the relative policy
    against the plain one built with out_scale * basal and out_bias * basal (the float64 products, rounded once to the env's
    dtype on both sides) -- env, policy state and every trace column bit for bit"""
    torch = support.gpu_torch()
    n, K, patient = 128, 40, 7
    _, z, mt, ma = support.exact_inputs(n, K, seed=SEED)
    inp = (np.full(n, patient), z, mt, ma)
    basal64 = float(support.basal_of(np.array([patient]))[0])
    scale, bias = 1.8, 0.4
    rel = support.random_policy(widths=(16, 16, 1), seed=6, out_scale=scale, out_bias=bias, relative_to="basal")
    plain = support.random_policy(widths=(16, 16, 1), seed=6, out_scale=scale * basal64, out_bias=bias * basal64)
    assert torch.equal(rel.flat_params(), plain.flat_params()) and rel.output == "logistic"
    a, b = (support.host_noise_env(*inp, exact=False, dtype=getattr(torch, dtype)) for _ in range(2))
    ta, tb = a.new_trace(K, columns=support.MLP_TRACE), b.new_trace(K, columns=support.MLP_TRACE)
    sa, sb = a.rollout_mlp(K, rel, trace=ta), b.rollout_mlp(K, plain, trace=tb)
    assert a.sync() == 0 and b.sync() == 0
    assert float(ta["action"][1:].std()) > 0
    support.same_env(a, b, support.STATE)
    support.same_dicts(sa, sb, support.POLICY_STATE)
    support.same_dicts(ta, tb, support.MLP_TRACE)


@pytest.mark.parametrize("exact", [False, True], ids=["fixed_step", "exact"])
def test_rel_rollout_is_the_policy_action_policy_bolus_step_loop_bit_for_bit(exact):
    """192 envs, three random 16-wide policies of 64, all 30 patients, four meals per env, 40 Dexcom steps, relative_to="basal"
    with meal_bolus: rollout_mlp (exact: rollout_mlp_dopri5) against the loop of policy_action(), policy_bolus(), step(u, bolus)
    and the window shift -- env, policy state and every trace row, "action" and "bolus" included, bit for bit"""
    torch = support.gpu_torch()
    n, K = 192, 40
    inp = support.exact_inputs(n, K, seed=SEED)
    pol = support.random_policy(widths=(16, 1), n_policies=3, seed=4, out_scale=3.0, out_bias=0.25, relative_to="basal", meal_bolus=TARGET)
    a, b = (support.host_noise_env(*inp, exact=exact) for _ in range(2))
    cols = support.MLP_TRACE + ("bolus",)
    sa = a.new_policy_state(pol)
    rows = {c: [] for c in cols}
    for _ in range(K):
        u, bolus = a.policy_action(pol, sa), a.policy_bolus(pol, sa)
        a.step(u, bolus)
        pol.shift(sa["cgm_hist"], sa["ins_hist"], a.cgm, a.insulin)
        sa["prev_meal"] = a.meal.clone()
        for key, t in (("bg", a.bg), ("cgm", a.cgm), ("cho", a.meal), ("insulin", a.insulin), ("action", u), ("bolus", bolus)):
            rows[key].append(t.clone())
    tr = b.new_trace(K, columns=cols)
    sb = (b.rollout_mlp_dopri5 if exact else b.rollout_mlp)(K, pol, trace=tr)
    assert a.sync() == 0 and b.sync() == 0
    act, bol = torch.stack(rows["action"]), torch.stack(rows["bolus"])
    # the action follows the patient: relative to each env's basal rate it stays inside the logistic's span
    rel = act / a.bb_constants()["basal"]
    assert float(rel.min()) >= 0.25 - 1e-6 and float(rel.max()) <= 3.25 + 1e-6 and float(rel.std()) > 0
    assert int((bol > 0).sum()) > 0 and int((bol == 0).sum()) > 0
    for c in cols:
        assert torch.equal(support.bits(torch.stack(rows[c])), support.bits(tr[c][1:])), c
    support.same_env(a, b, ("x", "t", "cgm", "bg", "reward", "last_cgm", "prev_risk", "planned", "meal", "insulin") +
                     (("h_carry",) if exact else ()), by="value")
    support.same_dicts(sa, sb, support.POLICY_STATE, by="value")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_action_is_scale_times_the_pre_output_value(dtype):
    """identity output, out_bias 0: the collector's "action" row is scale[i] * mlp_pre_output(params, features) in torch, bit for
    bit -- fma(s, y, 0) is the one rounding of s * y, so there is no tolerance.  128 envs of all 30 patients under two policies."""
    torch = support.gpu_torch()
    from simglucose_amd.controller import mlp_pre_output
    n, K = 128, 12
    inp = support.exact_inputs(n, K, seed=SEED)
    e = support.host_noise_env(*inp, exact=False, dtype=getattr(torch, dtype))
    pol = support.random_policy(widths=(16, 1), n_policies=2, seed=9, output="identity", bias_gain=1.0, out_scale=0.7, out_bias=0.0,
                                relative_to="basal")
    tr = e.new_trace(K, columns=("action", "features"), history=pol.history)
    e.collect_mlp(K, pol, trace=tr)
    assert e.sync() == 0
    y = mlp_pre_output(pol.device_params(e.device, e.dtype), tr["features"][1:].contiguous(), pol)
    scale = torch.as_tensor(0.7 * support.basal_of(inp[0]), dtype=e.dtype, device=e.device)
    want = scale * y
    assert bool((y != 0).all()) and float(y.std()) > 0
    assert torch.equal(support.bits(tr["action"][1:]), support.bits(want))


def _loop_of_one_step_collects(e, pol, K, sigma, explore_seed, acc, tr, term, es):
    """support.loop_of_entry_points with the draw: per step collect_mlp(1, on_done="continue"), restart_done, the torch reset of
    the policy state.  The draw is keyed by env, episode and clock, so the loop's eps are the one launch's."""
    torch = support.gpu_torch()
    st = e.new_policy_state(pol)
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    for _ in range(K):
        e.collect_mlp(1, pol, sigma=sigma, explore_seed=explore_seed, policy_state=st, stats=acc, trace=tr, on_done="continue")
        done = e.done.bool()
        e.restart_done(days=support.DAYS, terminal_obs=term, episode_stats=es)
        st["cgm_hist"].copy_(torch.where(done, e.cgm, st["cgm_hist"]))
        st["ins_hist"].copy_(torch.where(done, zero, st["ins_hist"]))
        st["prev_meal"].copy_(torch.where(done, zero, st["prev_meal"]))
    assert e.sync() == 0
    return st


def test_rel_collector_with_noise_and_restarts_is_the_loop_of_entry_points():
    """256 envs of child#001 / adult#001 alternating (every wave mixed), four policies asking for about four times the basal rate
    with meal_bolus, sigma 0.1, on_done="restart", launches of 7 + 60 + 1 + 102 steps against the loop of one-step calls with
    restart_done in between: env, policy state, accumulators, episode statistics, terminal observations and every trace column
    bit for bit.  Noise-free, support.restart_pair compares the same policy with the loop of rollout_mlp(1)."""
    torch = support.gpu_torch()
    pol = support.random_policy(widths=(8, 1), n_policies=4, seed=11, output="identity", gain=0.02, out_scale=1.0, out_bias=4.0,
                                relative_to="basal", meal_bolus=TARGET)
    cuts, n = (7, 60, 1, 102), 256
    K = sum(cuts)
    cols = support.MLP_TRACE + ("reward", "done", "eps", "bolus")
    A, B = (support.gym_env(n) for _ in range(2))
    z = lambda e: torch.zeros(n, dtype=e.dtype, device=e.device)
    sa, ta, terma, esa = support.stats(A), A.new_trace(K, columns=cols), z(A), support.episode_stats(A)
    sb, tb, termb, esb = support.stats(B), B.new_trace(K, columns=cols), z(B), support.episode_stats(B)
    sta = None
    for k in cuts:
        sta = A.collect_mlp(k, pol, sigma=0.1, explore_seed=77, policy_state=sta, stats=sa, trace=ta, on_done="restart",
                            days=support.DAYS, terminal_obs=terma, episode_stats=esa)
    assert A.sync() == 0
    stb = _loop_of_one_step_collects(B, pol, K, 0.1, 77, sb, tb, termb, esb)
    restarts = int((B.episode - 1).sum())
    print("\n[policy rel] collector: restarts %d in %d env-steps, bolus steps %d" % (restarts, n * K, int((tb["bolus"][1:] > 0).sum())), end="")
    assert restarts >= 0.05 * n and int((tb["bolus"][1:] > 0).sum()) > 0 and float(tb["eps"][1:].std()) > 0.5
    support.same_env(B, A, keys=support.STATE + ("meal_time", "meal_amt", "start_minute", "episode", "cgm0"))
    support.same_dicts(stb, sta, support.POLICY_STATE)
    support.same_dicts(sb, sa, support.STATS)
    support.same_dicts(esb, esa, support.EPISODE_STATS)
    assert torch.equal(support.bits(termb), support.bits(terma))
    support.same_dicts(tb, ta, cols)
    restarts2, _, _ = support.restart_pair(pol, (60, 110))
    assert (restarts2 > 0).sum() >= 0.05 * n


def test_exact_collector_refuses_a_relative_policy_and_changes_nothing():
    torch = support.gpu_torch()
    from simglucose_amd import _lib
    e = support.gym_env(128, exact=True)
    pol = support.random_policy(widths=(8, 1), n_policies=2, seed=11, output="identity", gain=0.02, out_scale=1.0, out_bias=4.0,
                                relative_to="basal")
    st = e.new_policy_state(pol)
    tr = e.new_trace(4, columns=support.MLP_TRACE + ("bolus",))
    keys = support.STATE_EXACT + ("meal_time", "meal_amt", "start_minute", "episode", "cgm0", "nfev")
    before = {k: getattr(e, k).clone() for k in keys}
    st0 = {k: v.clone() for k, v in st.items()}
    tr0 = {k: (v.clone() if k != "row" else v) for k, v in tr.items()}
    with pytest.raises(_lib.T1DError) as err:
        e.collect_mlp_dopri5(4, pol, sigma=0.1, policy_state=st, trace=tr, on_done="restart", days=support.DAYS)
    assert "relative_to" in str(err.value) and "t1d_collect_mlp_dopri5_rel" in str(err.value)
    assert e.sync() == 0
    support.same_dicts(before, {k: getattr(e, k) for k in keys}, keys)
    support.same_dicts(st0, st, support.POLICY_STATE)
    support.same_dicts(tr0, tr, support.MLP_TRACE + ("bolus",))
    assert tr["row"] == tr0["row"] == 1
    # the library's own check of the split, under the call's name, before anything is launched
    o = e._env_output_struct(pol)
    p, params = e._mlp_struct("test", pol, st)
    p.n_policies = 3
    with torch.cuda.device(e.device):
        rc = e._L.t1d_rollout_mlp_dopri5_rel(e._ctx, C.byref(e._b), C.byref(p), C.byref(o), None, C.c_void_p(e.h_carry.data_ptr()), None,
                                             2, 3, e._stream())
        assert rc == -1 and e._L.t1d_last_error().startswith(b"t1d_rollout_mlp_dopri5_rel:") and b"n_policies" in e._L.t1d_last_error()
        rc = e._L.t1d_mlp_action_rel(e._ctx, C.byref(e._b), C.byref(p), C.byref(o), C.c_void_p(e.h_carry.data_ptr()), e._stream())
        assert rc == -1 and e._L.t1d_last_error().startswith(b"t1d_mlp_action_rel:")
    assert e.sync() == 0
    support.same_dicts(before, {k: getattr(e, k) for k in keys}, keys)
    # the same policy is served where the relative output exists, without a meal bolus here
    e.rollout_mlp_dopri5(2, pol, policy_state=st, trace={k: v for k, v in tr.items() if k != "bolus"})
    assert e.sync() == 0 and bool(torch.isfinite(tr["action"][1:3]).all())
