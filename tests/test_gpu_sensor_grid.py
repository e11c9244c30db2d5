"""The sensor grid off its three stock points.  t1d_ctx_create takes any whole sample_time from 1 to 150 minutes and
BatchedT1DSimEnv(sensor_row=...) hands a custom row through; the device has compile-time paths for st in {1, 3, 5} and
S = 150 // st in {150, 50, 30} (divmod_uniform), a spline cache that is refetched per 15-minute interval (noise_sample),
and four places that decide when a noise block opens (refill_kernel, the host's shadow clock, plan_call's split_refill and
the inline refill).  Here every step path, the closed loops and launches that are not one sample long run at other sample
times -- samples that skip spline intervals (st = 20), sit on the last knot (150), leave a block shorter than 150 minutes
(4, 7) -- against the CPU oracle (OracleEnv(sensor_row_override=...), whose spline operator test_sensor_grid_host.py pins to
SciPy's interp1d) and against each other.

Inputs (support.grid_inputs): the Dexcom row with another sample_time, 150 envs (two full 64-env chunks and a partial one),
all 30 patients, host normals, K = max(5, 2 S + 1) steps so that a third noise block opens, 60 g in every third env, an
action that moves with the step.  The MLP roll-outs take 192 envs (a policy needs a multiple of 64).

Tolerances are the project's own: TOL_ORACLE (test_gpu_parity.py) on BG, CGM and last_cgm, the same figure relative to
max(1, |x|) on the states, 1e-6 on reward and risk; the exact mode as test_gpu_dopri5.py holds a heterogeneous batch to
its oracle (95 % of the envs within 1e-8, none beyond 5e-4: an accept/reject decision of the solver may fall the other
way at the last bit); fp32 against fp64 TOL_F32 (test_gpu_step_trim.py); kernel against kernel 1e-9 on outputs
and 1e-7 on the states (fp32: 5e-3), as test_multi_minute_kernel_equals_generic_kernel.

Worst values on an MI355X (every case prints its own; the tables are in profiles/sensor_grid/README.md):
  step paths against the oracle, the same for all paths and for the Philox replay: BG and CGM 0.94e-9 (st = 20) to
    2.6e-9 (st = 150), last_cgm up to 3.0e-9, states 5.3e-10 relative, reward 1.6e-10, risk 5.2e-10, no done flip;
  the multi-minute kernel's overflow path (315 envs in one workgroup, all fed, 64 records): BG and CGM 1.1e-9 to 2.9e-9;
  exact mode: 145 of 150 envs within 1e-8 at every st but 4 (all 150), the other five -- patient 24 -- up to 6.7e-5 (st = 150),
    done equal on all;
  fp32 against fp64: BG and CGM 6.4e-4 to 1.9e-3;
  roll-outs against their loops: states, BG, meal, insulin identical, CGM within 5.7e-14 (one launch) and 1.0e-12 (a launch
    per step, st = 150); rollout_mlp, rollout_mlp_dopri5 and the collector with restarts bit for bit;
  uneven launches against whole steps: states identical, last_cgm and prev_risk within 1.6e-13, the 14-minute launch at st = 7
    within 2.3e-13 of the mean of its two steps; shadow clock against the envs' own clocks bit for bit; fp32 identical.
No case is over its bound.  rollout_mlp against its step() loop was not bit for bit before noise_sample wrote its spline
sum with explicit fma (that README, "What was found").
"""
import numpy as np
import pytest

import support
from support import GRID_OUT, GRID_STS, gpu_torch as _torch, grid_action, grid_env, grid_inputs, grid_oracle, grid_sensor_row
from test_gpu_parity import TOL_ORACLE
from test_gpu_step_trim import TOL_F32

pytestmark = pytest.mark.gpu

TOL_KERNELS, TOL_KERNELS_X = 1e-9, 1e-7          # test_multi_minute_kernel_equals_generic_kernel, fp64
TOL_KERNELS_F32, TOL_KERNELS_X_F32 = 5e-3, 0.2   # outputs: ..odd_shapes..; states: the tighter of the two tests' fp32 bounds
SMALL_PARK = (("multi_minute_kernel", 2), ("park_cap", 64), ("s1_blocks", 3))
PATHS = {"generic": (), "refill_inline": (("split_refill", 0),), "multi_minute": (("multi_minute_kernel", 2),),
         "multi_minute_small_park": SMALL_PARK}
CASES = [(st, path) for st in GRID_STS for path in ("generic", "refill_inline", "multi_minute")] + \
        [(st, "multi_minute_small_park") for st in (4, 20, 150)]
# the multi-minute kernel's overflow path: one workgroup (s1_blocks = 1) over five chunks, every env fed, 64 records
OVERFLOW_N, OVERFLOW_CAP = 64 * 5 - 5, 64
OVERFLOW = (("multi_minute_kernel", 2), ("park_cap", OVERFLOW_CAP), ("s1_blocks", 1))


def _run(e, inp, cast=None):
    """K steps of the grid's actions -> GRID_OUT as arrays [K + 1, n] (row 0: after reset), x, t, last_cgm"""
    torch = _torch()
    rows = {k: [getattr(e, k).clone()] for k in GRID_OUT}
    for k in range(inp["K"]):
        e.step(torch.as_tensor(grid_action(inp, k), dtype=e.dtype, device=e.device))
        for key in GRID_OUT:
            rows[key].append(getattr(e, key).clone())
    assert e.sync() == 0                                        # no normal missing, nothing non-finite, no stall
    out = {k: torch.stack(v).double().cpu().numpy() for k, v in rows.items()}
    out.update(x=e.x.double().cpu().numpy(), t=e.t.cpu().numpy(), last_cgm=e.last_cgm.double().cpu().numpy())
    return out


def _worst(got, ref):
    w = {k: float(np.abs(got[k] - ref[k]).max()) for k in ("cgm", "bg", "reward", "risk", "last_cgm")}
    w["x"] = float((np.abs(got["x"] - ref["x"]) / np.maximum(1.0, np.abs(ref["x"]))).max())
    w["done"] = int((got["done"] != ref["done"]).sum())
    return w


def _follows_oracle(label, got, ref, K, st):
    w = _worst(got, ref)
    print("\n[sensor grid] %s: worst |device - oracle| cgm %.2e bg %.2e last_cgm %.2e reward %.2e risk %.2e x(rel) %.2e, done flips %d"
          % (label, w["cgm"], w["bg"], w["last_cgm"], w["reward"], w["risk"], w["x"], w["done"]))
    assert np.isfinite(got["cgm"]).all() and np.isfinite(got["bg"]).all() and np.isfinite(got["x"]).all()
    assert (got["t"] == K * st).all() and (ref["t"] == K * st).all()
    assert w["cgm"] < TOL_ORACLE and w["bg"] < TOL_ORACLE and w["last_cgm"] < TOL_ORACLE, w
    assert w["x"] < TOL_ORACLE, w
    assert w["reward"] < 1e-6 and w["risk"] < 1e-6, w
    assert w["done"] == 0


@pytest.fixture(scope="module")
def shared():
    """reference runs that several cases compare with, each computed by the first case that asks and kept on the host"""
    return {}


def _once(shared, key, make):
    if key not in shared:
        shared[key] = make()
    return shared[key]


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("st,path", CASES)
def test_step_paths_follow_the_oracle(st, path):
    """reset and K steps of st minutes through the generic kernel (the default at 150 envs), the generic kernel with the
    refill inlined and the persistent multi-minute kernel, fp64, against the oracle's restatement of the default scheme:
    every output after reset and after every step, the state at the end.  multi_minute_small_park is the multi-minute kernel
    with 64 records and a 3-block grid: at 150 envs every workgroup owns one chunk and can leave at most 64 records, so
    nothing overflows there -- the overflow path has its own test below."""
    inp = grid_inputs(st)
    got = _run(grid_env(st, options=PATHS[path]), inp)
    _follows_oracle("st %3d %s" % (st, path), got, grid_oracle(st), inp["K"], st)


@pytest.mark.parametrize("st", (4, 20, 150))
def test_multi_minute_overflow_path_follows_the_oracle(st):
    """The multi-minute kernel where a workgroup's lanes of level 2 outnumber its records: 315 envs in one workgroup, 60 g
    in every env, 64 records.  A lane leaves at most one record per launch (at its first minute of level 2), so the launch
    that holds the meal parks 64 lanes and sends the others through the redo map: taken again from their loads, all
    minutes of the launch in place -- at st = 150 a launch of 150 minutes that opens a noise block on its last minute.
    Checked on the host first, from the oracle's level counts per step."""
    lanes = support.grid_level2_lanes(st, OVERFLOW_N, feed=1)
    print("\n[sensor grid] st %3d overflow: envs with a minute of level 2, per step: %s" % (st, lanes[:6]))
    assert lanes.max() > OVERFLOW_CAP and lanes.max() - OVERFLOW_CAP >= 64      # more than a wave's worth goes through the redo map
    inp = grid_inputs(st, OVERFLOW_N, feed=1)
    got = _run(grid_env(st, OVERFLOW_N, options=OVERFLOW, feed=1), inp)
    _follows_oracle("st %3d multi_minute_overflow" % st, got, support.grid_oracle_run(st, n=OVERFLOW_N, feed=1), inp["K"], st)


@pytest.mark.parametrize("st", GRID_STS)
def test_exact_mode_follows_the_oracles_dopri5(st):
    """t1d_step_dopri5 at the custom sample time against the oracle's DOPRI5.  Per env the largest |difference| of BG and
    CGM over the run, held to the bound of test_gpu_dopri5.py's heterogeneous batch (test_large_batch_sampled_envs_match_
    oracle): 95 % of the envs within 1e-8, none beyond 5e-4 -- an accept/reject decision of the solver falls the other way
    at the last bit.  That file's bound for 64 envs (none beyond 1e-5) does not describe these inputs: the oracle itself
    moves by 5.7e-5 mg/dL (st = 7) when its initial state changes by one ulp, on the envs of patient 24 -- the envs on
    which the device is 5.6e-5 away (test_sensor_grid_host.py measures it on the CPU).  The envs within 1e-8 also meet the
    fixed-step bounds on reward, risk, done and the final state."""
    inp = grid_inputs(st)
    got = _run(grid_env(st, integrator="dopri5"), inp)
    ref = grid_oracle(st, "dopri")
    worst = np.maximum(np.abs(got["bg"] - ref["bg"]).max(0), np.abs(got["cgm"] - ref["cgm"]).max(0))
    near = worst <= 1e-8
    print("\n[sensor grid] st %3d exact: %d of %d envs within 1e-8 of the oracle, max %.3e" % (st, near.sum(), len(near), worst.max()))
    assert (got["t"] == inp["K"] * st).all()
    assert np.array_equal(got["done"], ref["done"])             # every env, also the few that are 1e-5 away
    assert near.mean() >= 0.95 and worst.max() <= 5e-4, (near.mean(), worst.max())
    w = _worst({k: v[..., near] for k, v in got.items()}, {k: ref[k][..., near] for k in got})
    print("[sensor grid] st %3d exact, those envs: reward %.2e risk %.2e last_cgm %.2e x(rel) %.2e, done flips %d"
          % (st, w["reward"], w["risk"], w["last_cgm"], w["x"], w["done"]))
    assert w["reward"] < 1e-6 and w["risk"] < 1e-6 and w["last_cgm"] < 1e-8 and w["x"] < 1e-6 and w["done"] == 0, w


@pytest.mark.parametrize("st", GRID_STS)
def test_philox_noise_replays_through_host_normals_and_the_oracle(st):
    """Philox mode at S = 150 // st samples per block: the normals t1d_philox_normals exports, fed back as host normals,
    reproduce the run bit for bit, and the oracle follows on them -- block index -> draw index."""
    torch = _torch()
    inp = grid_inputs(st)
    e1 = grid_env(st, noise="philox", seed=99, env_offset=1000)
    z = e1.philox_normals(inp["z"].shape[0], draw0=0, episode=1)
    got = _run(e1, inp)
    host = _run(grid_env(st, z=z), inp)
    for k in GRID_OUT + ("x", "last_cgm", "t"):
        assert np.array_equal(got[k], host[k]), k
    _follows_oracle("st %3d philox" % st, got, support.grid_oracle_run(st, z=z.cpu().numpy()), inp["K"], st)
    assert float(np.std(got["cgm"] - got["bg"])) > 1.0          # the sensor noise is there


def _fp64_generic(shared, st):
    return _once(shared, ("fp64", st), lambda: _run(grid_env(st), grid_inputs(st)))


@pytest.mark.parametrize("path", ["generic", "multi_minute"])
@pytest.mark.parametrize("st", GRID_STS)
def test_fp32_tracks_fp64(shared, st, path):
    """the fp32 instantiations of the generic and the multi-minute kernel against the fp64 device run"""
    torch = _torch()
    inp = grid_inputs(st)
    got = _run(grid_env(st, dtype=torch.float32, options=PATHS[path]), inp)
    ref = _fp64_generic(shared, st)
    w = {k: float(np.abs(got[k] - ref[k]).max()) for k in ("bg", "cgm")}
    print("\n[sensor grid] st %3d fp32 %s: worst |fp32 - fp64| bg %.2e cgm %.2e" % (st, path, w["bg"], w["cgm"]))
    assert (got["t"] == ref["t"]).all()
    assert w["bg"] < TOL_F32 and w["cgm"] < TOL_F32, w


# ---------------------------------------------------------------------------------------------------------- 2
CLOSED_STS = (2, 7, 20, 150)
PID = (0.001, 0.00001, 0.001, 140.0)                            # P, I, D, target of test_rollout_pid_matches_step_by_step_and_oracle
LOOP_KEYS = ("x", "t", "cgm", "bg", "last_cgm", "prev_risk", "reward", "planned", "meal", "insulin")


def _step_by_step(st, ctrl, e=None, K=None, before=None):
    """K x (controller on the host with the custom sample time + t1d_step) -> the env's LOOP_KEYS and the controller state,
    on the host.  e, K: another env of sample time st and its number of steps (test_gpu_edge_states.py), None: the grid's;
    before(k): called ahead of step k"""
    torch = _torch()
    K = grid_inputs(st)["K"] if K is None else K
    e = grid_env(st) if e is None else e
    n = e.n
    obs = e.cgm.clone()
    if ctrl == "pid":
        P, I, D, target = PID
        integ = torch.zeros(n, dtype=torch.float64, device=e.device); prev = torch.zeros_like(integ)
        for k in range(K):                                      # pid_ctrller.py:17-36
            if before is not None:
                before(k)
            u = P * (obs - target) + I * integ + D * (obs - prev) / float(st)
            prev = obs.clone(); integ = integ + (obs - target) * float(st)
            e.step(u, torch.zeros_like(u))
            obs = e.cgm.clone()
        state = {"integ": integ, "prev": prev}
    else:
        c = e.bb_constants()
        meal = torch.zeros(n, dtype=torch.float64, device=e.device)
        boluses = 0
        for k in range(K):                                      # basal_bolus_ctrller.py:34-80
            if before is not None:
                before(k)
            bolus = torch.where(meal > 0, ((meal * st) / c["cr"] + (obs > 150) * (obs - 140.0) / c["cf"]) / st, torch.zeros_like(meal))
            boluses += int((bolus > 0).sum())
            e.step(c["basal"], bolus)
            obs, meal = e.cgm.clone(), e.meal.clone()
        assert boluses >= n // 3                                # the meals were announced and answered
        state = {"prev_meal": meal}
    assert e.sync() == 0
    out = {k: getattr(e, k).clone().cpu() for k in LOOP_KEYS}
    out.update({k: v.cpu() for k, v in state.items()})
    return out


@pytest.mark.parametrize("form", ["one_launch", "launch_per_step"])
@pytest.mark.parametrize("ctrl", ["pid", "bb"])
@pytest.mark.parametrize("st", CLOSED_STS)
def test_rollouts_match_step_by_step(shared, st, ctrl, form):
    """t1d_rollout_pid / t1d_rollout_bb in calls of 1, 2 and K - 3 steps -- all steps of a call in one launch of the generic
    roll-out kernel, or one launch of the multi-minute kernel per step with the controller in its prologue -- against the
    step() loop with the controller on the host: T(sen.st) in the PID's D and I terms and in the basal-bolus prev_meal * st."""
    torch = _torch()
    K = grid_inputs(st)["K"]
    ref = _once(shared, ("loop", st, ctrl), lambda: _step_by_step(st, ctrl))
    e = grid_env(st, options=(("rollout_launches", 0),) if form == "one_launch" else (("rollout_launches", 2), ("multi_minute_kernel", 2)))
    state = None
    for chunk in (1, 2, K - 3):
        state = e.rollout_pid(chunk, *PID[:3], PID[3], pid_state=state) if ctrl == "pid" else e.rollout_bb(chunk, bb_state=state)
    assert e.sync() == 0
    worst = {k: float((getattr(e, k).double().cpu() - ref[k].double()).abs().max()) for k in LOOP_KEYS}
    ctl = {k: float((state[k].cpu() - ref[k]).abs().max()) for k in (("integ", "prev") if ctrl == "pid" else ("prev_meal",))}
    print("\n[sensor grid] st %3d rollout_%s %s: worst |roll-out - loop| %s  controller %s"
          % (st, ctrl, form, " ".join("%s %.1e" % kv for kv in worst.items()), " ".join("%s %.1e" % kv for kv in ctl.items())))
    assert worst["t"] == 0 and int(e.t[0]) == K * st
    for k in LOOP_KEYS:
        assert worst[k] < 1e-9, (k, worst)
    if ctrl == "pid":
        assert ctl["integ"] < 1e-6 and ctl["prev"] < 1e-9, ctl
    else:
        assert ctl["prev_meal"] < 1e-12, ctl


@pytest.mark.parametrize("exact", [False, True], ids=["fixed_step", "exact"])
@pytest.mark.parametrize("st", (7, 150))
def test_mlp_rollout_is_the_policy_action_step_loop_bit_for_bit(st, exact):
    """rollout_mlp(K) (exact: rollout_mlp_dopri5) against the loop of policy_action() and step(), 192 envs, three policies
    of 64: env, policy state and every trace row bit for bit, in both modes.  In the fixed-step mode step() and the roll-out
    are different instantiations of noise_sample; its spline sum is written with explicit fma so that they round alike
    (before that: 121 CGM words differed at st = 7, by at most 1.1e-13 mg/dL, 252 at Dexcom's own 3 minutes)."""
    torch = _torch()
    n = 192
    K = grid_inputs(st, n)["K"]
    pol = support.random_policy(widths=(16, 1), n_policies=3, seed=4)
    kw = dict(integrator="dopri5") if exact else {}
    a, b = grid_env(st, n, **kw), grid_env(st, n, **kw)
    sa = a.new_policy_state(pol)
    zero = torch.zeros(n, dtype=a.dtype, device=a.device)
    rows = {k: [] for k in support.MLP_TRACE}
    for _ in range(K):
        u = a.policy_action(pol, sa)
        a.step(u, zero)
        pol.shift(sa["cgm_hist"], sa["ins_hist"], a.cgm, a.insulin)
        sa["prev_meal"] = a.meal.clone()
        for key, t in (("bg", a.bg), ("cgm", a.cgm), ("cho", a.meal), ("insulin", a.insulin), ("action", u)):
            rows[key].append(t.clone())
    tr = b.new_trace(K, columns=support.MLP_TRACE)
    sb = (b.rollout_mlp_dopri5 if exact else b.rollout_mlp)(K, pol, trace=tr)
    assert a.sync() == 0 and b.sync() == 0
    assert int(b.t.min()) == K * st == int(b.t.max())
    for k in support.MLP_TRACE:
        d = (torch.stack(rows[k]) - tr[k][1:]).abs()
        print("\n[sensor grid] st %3d mlp %s: %s words that differ %d, max %.2e" % (st, "exact" if exact else "fixed", k, int((d != 0).sum()), float(d.max())), end="")
    assert float(torch.stack(rows["action"]).std()) > 0 and float(torch.stack(rows["cho"]).max()) > 0
    for k in support.MLP_TRACE:
        assert torch.equal(torch.stack(rows[k]), tr[k][1:]), k
    support.same_env(a, b, ("x", "t", "cgm", "bg", "reward", "last_cgm", "prev_risk", "planned", "meal", "insulin") +
                     (("h_carry",) if exact else ()), by="value")
    support.same_dicts(sa, sb, support.POLICY_STATE, by="value")


def test_collector_with_restarts_is_the_loop_of_entry_points_at_7_minutes():
    """collect_mlp(on_done="restart") at st = 7 in launches of 60 and 110 steps (1 190 minutes) against
    support.loop_of_entry_points, bit for bit, under policies around 0.05 U/min so that episodes end"""
    restarts, low, high = support.restart_pair(support.hypo_leaning_policies(4), (60, 110), sensor_row=grid_sensor_row(7))
    print("\n[sensor grid] st 7 collector: restarted envs %d of 256, max restarts per env %d, endings < 70: %d, > 350: %d"
          % ((restarts > 0).sum(), restarts.max(), low, high))
    assert (restarts > 0).sum() >= 0.05 * 256 and low > 0        # asserted on the reference loop: the comparison covers restarts


# ---------------------------------------------------------------------------------------------------------- 3
CUT_KEYS = ("x", "last_cgm", "planned", "last_qsto", "last_food", "prev_risk")
CUT_FORMS = {"default": (), "deferred_refinement": (("adaptive_gut", 3),), "multi_minute": (("multi_minute_kernel", 2),)}


def _cut_meals(st, n):
    """60 g at the first minute of step 1 in every third env, 45 g at minute 100 + i % 7 in every env -> tables [2, n]"""
    from simglucose_amd import _lib
    i = np.arange(n)
    mt = np.stack([np.where(i % 3 == 0, st, 100 + i % 7), np.where(i % 3 == 0, 100 + i % 7, _lib.MEAL_UNUSED)]).astype(np.int64)
    ma = np.stack([np.where(i % 3 == 0, 60.0, 45.0), np.where(i % 3 == 0, 45.0, 0.0)])
    return mt, ma


def _cut_env(st, options=(), dtype=None):
    torch = _torch()
    e = grid_env(st, options=options, meals=False, dtype=dtype or torch.float64)
    mt, ma = _cut_meals(st, e.n)
    e.set_meals(torch.as_tensor(mt), torch.as_tensor(ma))
    e.reset()
    return e


def _cut_run(e, st, cuts, own_clocks=False):
    """the launches `cuts` under the env's constant basal -> per launch bg, cgm, meal, insulin [len(cuts), n], the final state,
    on the host"""
    torch = _torch()
    basal = torch.as_tensor(grid_inputs(st)["basal"], dtype=e.dtype, device=e.device)
    if own_clocks:
        e.invalidate_clock()
    rows = {k: [] for k in ("bg", "cgm", "meal", "insulin")}
    for m in cuts:
        e.step(basal, minutes=m)
        assert own_clocks == (e._clock is None)
        for k in rows:
            rows[k].append(getattr(e, k).clone())
    assert e.sync() == 0
    out = {k: torch.stack(v).cpu() for k, v in rows.items()}
    out.update({k: getattr(e, k).cpu() for k in CUT_KEYS + ("t", "meta", "next_meal")})
    return out


def _whole_steps(shared, st, dtype_name="float64"):
    torch = _torch()
    return _once(shared, ("whole", st, dtype_name),
                 lambda: _cut_run(_cut_env(st, dtype=getattr(torch, dtype_name)), st, [st] * grid_inputs(st)["K"]))


def _same_end(label, a, b, tol, tol_x):
    torch = _torch()
    for k in ("t", "meta", "next_meal"):
        assert torch.equal(a[k], b[k]), k
    worst = {k: float((a[k].double() - b[k].double()).abs().max()) for k in CUT_KEYS}
    print("\n[sensor grid] %s: worst |cuts - whole steps| %s" % (label, " ".join("%s %.1e" % kv for kv in worst.items())))
    for k in CUT_KEYS:
        assert worst[k] < (tol_x if k == "x" else tol), (k, worst)


@pytest.mark.parametrize("st", (3, 7))
def test_whole_steps_of_the_cut_inputs_follow_the_oracle(shared, st):
    """env A, K steps of st minutes under a constant basal: its final x and last_cgm against the oracle"""
    from oracle import t1d_oracle as O
    torch = _torch()
    inp = grid_inputs(st)
    mt, ma = _cut_meals(st, inp["n"])
    cho = support.dense_cho(torch.as_tensor(mt), torch.as_tensor(ma), np.arange(inp["n"]), inp["K"] * st)
    orc = O.OracleEnv(inp["pid"], normals=inp["z"], integrator="split_adaptive", n_sub=4, sensor_row_override=inp["row"])
    orc.reset()
    for k in range(inp["K"]):
        orc.step(inp["basal"], None, cho[k * st:(k + 1) * st])
    a = _whole_steps(shared, st)
    wx = float((np.abs(a["x"].cpu().numpy() - orc.x) / np.maximum(1.0, np.abs(orc.x))).max())
    wc = float(np.abs(a["last_cgm"].cpu().numpy() - orc.last_cgm).max())
    print("\n[sensor grid] st %d whole steps: worst |device - oracle| x(rel) %.2e last_cgm %.2e; level counts %s" % (st, wx, wc, orc.level_count))
    assert orc.level_count[2] > 0 and cho.sum() > 0
    assert wx < TOL_ORACLE and wc < TOL_ORACLE


@pytest.mark.parametrize("form", list(CUT_FORMS))
@pytest.mark.parametrize("st", (3, 7))
def test_launch_lengths_that_are_not_the_sample_time(shared, st, form):
    """env B, the same K st minutes in launches of (1, 2, st + 1, 2 st, 1, st - 1, 3 st + 2) minutes repeated: launches
    without a sample, launches with several, and one that opens a noise block in its middle.  One-minute launches take the
    persistent single-minute kernel (with adaptive_gut = 3: its deferred form), launches of up to st minutes the generic
    kernel or (multi_minute_kernel = 2) the multi-minute kernel, longer ones the generic kernel with the refill inline.
    The state ends where K whole steps put it; a launch of 2 st minutes that spans two whole steps reports their mean."""
    torch = _torch()
    inp = grid_inputs(st)
    K, S = inp["K"], inp["S"]
    cuts = support.uneven_cuts(st, K * st)
    assert sum(cuts) == K * st
    t0, found = 0, False
    for m in cuts:                                              # a launch with two samples or more, one of which opens a block inside it
        samples = [t1 for t1 in range(t0 + 1, t0 + m + 1) if t1 % st == 0]
        found = found or (len(samples) >= 2 and any((1 + t1 // st) % S == 0 and t1 < t0 + m for t1 in samples))
        t0 += m
    assert found
    a = _whole_steps(shared, st)
    b = _cut_run(_cut_env(st, CUT_FORMS[form]), st, cuts)
    assert int(b["t"][0]) == K * st
    _same_end("st %d cuts %s" % (st, form), b, a, TOL_KERNELS, TOL_KERNELS_X)
    pair = support.whole_pair_launch(st, cuts)
    if pair is not None:                                        # st = 7 (test_sensor_grid_host.py: st = 3 has none)
        j, k = pair
        for key in ("bg", "cgm", "meal", "insulin"):
            d = float((b[key][j] - 0.5 * (a[key][k] + a[key][k + 1])).abs().max())
            print("[sensor grid] st %d cuts %s: launch %d of 2 st minutes against the mean of steps %d, %d: %s %.1e" % (st, form, j, k, k + 1, key, d))
            assert d < TOL_KERNELS, (key, d)
    else:
        assert st == 3


@pytest.mark.parametrize("st", (3, 7))
def test_shadow_clock_and_the_envs_own_clocks_open_the_same_blocks(st):
    """the cut run once under the host's shadow clock (int(150 // sample_time) samples per block) and once after
    invalidate_clock(), where refill_kernel reads every env's own clock ahead of every launch: bit for bit"""
    torch = _torch()
    cuts = support.uneven_cuts(st, grid_inputs(st)["K"] * st)
    b = _cut_run(_cut_env(st), st, cuts)
    c = _cut_run(_cut_env(st), st, cuts, own_clocks=True)
    for k in b:
        assert torch.equal(b[k], c[k]), k


@pytest.mark.parametrize("st", (3, 7))
def test_launch_lengths_that_are_not_the_sample_time_fp32(shared, st):
    torch = _torch()
    cuts = support.uneven_cuts(st, grid_inputs(st)["K"] * st)
    a = _whole_steps(shared, st, "float32")
    b = _cut_run(_cut_env(st, dtype=torch.float32), st, cuts)
    _same_end("st %d cuts fp32" % st, b, a, TOL_KERNELS_F32, TOL_KERNELS_X_F32)
