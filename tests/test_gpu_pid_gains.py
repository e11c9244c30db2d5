"""Per-env PID gains on the device (t1d_rollout_pid_gains / t1d_rollout_pid_dopri5_gains through rollout_pid /
rollout_pid_dopri5): an env under gains g inside a mixed batch is, bit for bit, that env of a batch run entirely under g by
the scalar call -- in the all-steps-in-one-launch kernel, in the launch-per-step kernel and in the exact mode --, arrays
filled with one set give the scalar call's result, every lane follows the CPU oracle's closed loop under its own gains, and
the scalar call itself gives what it gave.

150 envs (two full waves and a partial chunk), five patients interleaved (i % 5), four gain sets interleaved lane by lane
(i % 4; 20 = lcm: every patient meets every set), Dexcom, a random-meal day from 06:00 as support.meal_day_env makes it, 40
steps in calls of 1, 7 and 32.  SEED was picked on the CPU oracle (oracle/t1d_streams.py for the normals and the meals):
under it six lanes of "hot" end their episode low within the 40 steps (the first in step 33) and 27 lanes ask for a
negative rate at some step, so `done` and the pump's clamp are both in the comparison.  Every run is made once and shared:
what run() returns is read-only."""
import functools

import numpy as np
import pytest

from support import START, STATE, STATE_EXACT, STATS, ST, dense_cho, gpu_torch, stats
from support_ctrl import PID

pytestmark = pytest.mark.gpu

N, K, CUTS, SEED = 150, 40, (1, 7, 32), 9
PATIENTS = (0, 6, 12, 18, 24)                                    # rows of the patient table: adolescents, adults, children
SETS = {"stock": PID["stock"], "high": PID["high"], "hot": PID["hot"], "target110": PID["stock"][:3] + (110.0,)}
ORDER = ("stock", "high", "hot", "target110")                    # lane i runs under ORDER[i % 4]
TRACE = ("bg", "cgm", "cho", "insulin")
# form -> (dtype, exact mode?, options set before reset, max_minutes_per_launch).  The exact mode's second form cuts the
# calls of 7 and 32 steps into launches of 5 steps (15 minutes).
FORMS = {"one_launch_f64": ("float64", False, (("rollout_launches", 0),), None),
         "one_launch_f32": ("float32", False, (("rollout_launches", 0),), None),
         "per_step_f64": ("float64", False, (("rollout_launches", 2), ("multi_minute_kernel", 2)), None),
         "per_step_f32": ("float32", False, (("rollout_launches", 2), ("multi_minute_kernel", 2)), None),
         "exact": ("float64", True, (), 240),
         "exact_cut": ("float64", True, (), 5 * ST)}


def _pid():
    return np.array(PATIENTS)[np.arange(N) % len(PATIENTS)]


def _lanes(name):
    return np.arange(ORDER.index(name), N, len(ORDER))


def _env(form):
    torch = gpu_torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    from simglucose_amd.scenario_batch import random_meal_tables
    dtype_name, exact, options, _ = FORMS[form]
    dtype = getattr(torch, dtype_name)
    e = BatchedT1DSimEnv(patient=_pid(), sensor="Dexcom", dtype=dtype, seed=SEED, n_sub=4, integrator="dopri5" if exact else None)
    e.start_minute = torch.full((N,), START, dtype=torch.int32, device=e.device)
    e.set_meals(*random_meal_tables(N, days=1, start_minute_of_day=e.start_minute, seed=SEED, dtype=dtype))
    for name, value in options:
        e.set_option(name, value)
    e.reset()
    return e


def _mixed(e, how):
    """the four arguments of the mixed batch: float64 arrays of the sets' own doubles, lane by lane"""
    g = np.array([SETS[ORDER[i % len(ORDER)]] for i in range(N)], dtype=np.float64).T
    if how == "dict":
        return (e.pid_gains(*g),)
    return tuple(g)


@functools.lru_cache(maxsize=None)
def run(form, gains, how="arrays"):
    """The 40 steps of `form` under `gains`: "mixed" (the four sets interleaved), or a set's name with how = "scalar" (the
    scalar call) or "constant" (arrays filled with the set).  -> dict of what the run left, on the host"""
    torch = gpu_torch()
    _, exact, _, mm = FORMS[form]
    e = _env(form)
    if gains == "mixed":
        args = _mixed(e, how)
    elif how == "scalar":
        args = SETS[gains]
    else:
        args = tuple(np.full(N, v) if k % 2 else torch.full((N,), v, dtype=torch.float64) for k, v in enumerate(SETS[gains]))
    acc, tr, state = stats(e), e.new_trace(K, columns=TRACE), None
    total = torch.zeros(N, dtype=torch.int64, device=e.device)
    for k in CUTS:
        if exact:
            state = e.rollout_pid_dopri5(k, *args, pid_state=state, stats=acc, trace=tr, max_minutes_per_launch=mm)
            total += e.nfev
        else:
            state = e.rollout_pid(k, *args, pid_state=state, stats=acc, trace=tr)
    assert e.sync() == 0
    assert tr["row"] == K + 1 and int(e.t.min()) == K * ST == int(e.t.max())
    out = {k: getattr(e, k).cpu() for k in (STATE_EXACT if exact else STATE)}
    out.update({k: state[k].cpu() for k in ("integ", "prev")})
    out.update({k: acc[k].cpu() for k in STATS})
    out.update({"trace_" + k: tr[k].cpu() for k in TRACE})
    if exact:
        out["nfev"] = total.cpu()
    return out


def _same(a, b, lanes, what):
    """every word of run a in `lanes` is that of run b, bit for bit"""
    torch = gpu_torch()
    from support import bits
    idx = torch.as_tensor(lanes)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(bits(a[k])[..., idx], bits(b[k])[..., idx]), (what, k)


def test_the_workload_ends_episodes_and_asks_for_negative_rates():
    """on the mixed fp64 run itself: some lane of "hot" sets done within the 40 steps, some command is below 0 (the pump
    clamps it: the insulin row is 0 there), and the four sets do different things"""
    r = run("one_launch_f64", "mixed")
    bg, cgm, ins = r["trace_bg"].numpy(), r["trace_cgm"].numpy(), r["trace_insulin"].numpy()
    hot = _lanes("hot")
    assert ((bg[1:, hot] < 70) | (bg[1:, hot] > 350)).any()
    assert r["n_low"][hot].sum() > 0
    # the command of step r from the trace: obs = the CGM row before it
    P, I, D, T = np.array([SETS[ORDER[i % 4]] for i in range(N)]).T
    obs, integ, prev, neg = cgm[0].copy(), np.zeros(N), np.zeros(N), np.zeros(N, bool)
    for k in range(K):
        u = P * (obs - T) + I * integ + D * (obs - prev) / ST
        neg |= (u < -1e-9) & (ins[1 + k] == 0.0)
        prev, integ, obs = obs.copy(), integ + (obs - T) * ST, cgm[1 + k]
    assert neg.any() and not neg[_lanes("high")].any()
    assert (ins[1:, _lanes("high")] == 0).all() and (ins[1:, _lanes("stock")] > 0).any()


@pytest.mark.parametrize("name", ORDER)
@pytest.mark.parametrize("form", list(FORMS))
def test_mixed_batch_equals_the_scalar_batches(form, name):
    _same(run(form, "mixed"), run(form, name, "scalar"), _lanes(name), (form, name))


@pytest.mark.parametrize("form", ["one_launch_f64", "per_step_f32", "exact"])
def test_the_dict_of_pid_gains_is_the_four_arrays(form):
    _same(run(form, "mixed", "dict"), run(form, "mixed"), np.arange(N), form)


@pytest.mark.parametrize("name", ["stock", "hot"])
@pytest.mark.parametrize("form", list(FORMS))
def test_constant_arrays_equal_the_scalar_call(form, name):
    _same(run(form, name, "constant"), run(form, name, "scalar"), np.arange(N), (form, name))


@functools.lru_cache(maxsize=None)
def _oracle():
    """the CPU oracle's closed loop of the mixed batch: the device's own normals and meal tables, the host PID recurrence on
    arrays with each lane's gains -> (bg [K, N], cgm [K, N])"""
    from oracle import t1d_oracle as O
    e = _env("one_launch_f64")
    z = e.philox_normals(1 + 10 * (2 + K * ST // 150), draw0=0, episode=1).cpu().numpy()
    cho = dense_cho(e.meal_time, e.meal_amt, np.arange(N), K * ST)
    orc = O.OracleEnv(_pid(), sensor="Dexcom", normals=z, integrator="split_adaptive", n_sub=4)
    r = orc.reset()
    P, I, D, T = np.array([SETS[ORDER[i % 4]] for i in range(N)]).T
    obs, integ, prev = r["cgm"].copy(), np.zeros(N), np.zeros(N)
    bg, cgm = np.empty((K, N)), np.empty((K, N))
    for k in range(K):
        u = P * (obs - T) + I * integ + D * (obs - prev) / ST            # pid_ctrller.py:17-36
        prev = obs.copy(); integ = integ + (obs - T) * ST
        o = orc.step(u, None, cho[k * ST:(k + 1) * ST])
        obs = o["cgm"]; bg[k] = o["bg"]; cgm[k] = o["cgm"]
    return bg, cgm


@pytest.mark.parametrize("form", ["one_launch_f64", "per_step_f64"])
def test_every_lane_follows_the_oracle_under_its_own_gains(form):
    """1e-8 mg/dL on bg and cgm for the lanes under stock, high and the target-110 set, 1e-6 for those under hot (the
    wind-up regime of config 5): the bounds of tests/test_gpu_configs.py"""
    ref_bg, ref_cgm = _oracle()
    r = run(form, "mixed")
    for name in ORDER:
        lanes, bound = _lanes(name), 1e-6 if name == "hot" else 1e-8
        for k, ref in (("bg", ref_bg), ("cgm", ref_cgm)):
            err = np.abs(r["trace_" + k][1:].numpy()[:, lanes] - ref[:, lanes]).max()
            print(form, name, k, "max |device - oracle| = %.3g mg/dL (bound %.0e)" % (err, bound))
            assert err < bound, (form, name, k, err)


@pytest.mark.parametrize("form", list(FORMS))
def test_scalar_path_is_untouched(form):
    """rollout_pid(K, *stock) in one call, on a fresh env: the scalar leg of the first test, which ran in calls of 1, 7 and
    32: the scalar call cut anywhere gives one result, as it always has"""
    torch = gpu_torch()
    _, exact, _, mm = FORMS[form]
    e = _env(form)
    acc, tr = stats(e), e.new_trace(K, columns=TRACE)
    if exact:
        state = e.rollout_pid_dopri5(K, *SETS["stock"], stats=acc, trace=tr, max_minutes_per_launch=mm)
    else:
        state = e.rollout_pid(K, *SETS["stock"], stats=acc, trace=tr)
    assert e.sync() == 0
    ref = run(form, "stock", "scalar")
    from support import bits
    for k in (STATE_EXACT if exact else STATE):
        assert torch.equal(bits(getattr(e, k).cpu()), bits(ref[k])), (form, k)
    for k in ("integ", "prev"):
        assert torch.equal(bits(state[k].cpu()), bits(ref[k])), (form, k)
    for k in STATS:
        assert torch.equal(acc[k].cpu(), ref[k]), (form, k)
    for k in TRACE:
        assert torch.equal(bits(tr[k].cpu()), bits(ref["trace_" + k])), (form, k)
    if exact:
        assert torch.equal(e.nfev.cpu().long(), ref["nfev"]), form
