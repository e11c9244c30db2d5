"""The device status word and non-finite data through every stepping kernel.

The suite holds every kernel family to the oracle on finite data.  Here one env of a batch stops being finite -- a state
word, or the action -- and the only signal the design leaves for that, the status word of t1d_sync (include/t1d.h, T1D_ST_*),
is held to its header: T1D_ST_NONFINITE is raised by exactly the launches that leave a non-finite word in some env's stored
x[12]; the word clears on read; the env itself reads `cgm` = sensor min and `done` = 0 (pinned as documented behaviour, not
endorsed); and no other env of the batch moves by a bit, whichever wave, list or LDS record the poisoned lane went through.

Inputs (support.status_inputs): 150 envs -- two full 64-env chunks and a partial one -- of all 30 patients, host normals,
70 g at the first minute of step 1 in every third env, an action that moves with the step.  Two envs A and B are built
alike and stepped twice; then a word of three lanes of A is made non-finite (support.status_lanes: one lane in chunk 0, one
in the partial chunk, one that the oracle's step-size rule puts at level 2 in the next minute, so that it goes through the
set-aside list / the LDS records), and three more steps follow.  The multi-minute kernel's overflow case feeds every env,
at the first minute of the first step after the poison: that minute puts all 150 lanes at level 2, against 64 records, so
the poisoned lanes and their neighbours go through the records and the redo map (test_status_host.py counts them).
The MLP paths take 256 envs under two policies (a policy needs a multiple of 64 envs) with Philox noise, which the
collector's restarts need.

References.  Which envs hold a non-finite x[12] and BG after which step, whether `done` is raised and which end of its range
the sensor reads is what the CPU oracle says after the same poison in the same scheme (support.status_oracle, pinned on the
host by test_status_host.py): in the fixed-step scheme every poisoned word reaches x[12] within the first minute and stays;
in the exact mode the solver gives up at once (T1D_ST_SOLVER_FAILED), the env keeps its last accepted state, and so a
poisoned x[0] or x[5] never reaches x[12] while x[12] = +Inf stays +Inf (BG above 350: done, sensor max).  That is a property
of where the word sits, not of the action or the sensor noise (a poisoned env's observation is the finite sensor min, so a
closed loop keeps giving it finite actions): the closed-loop paths and the MLP paths, whose inputs the oracle does not
restate, take the same per-lane answer.  Everything outside the poisoned lanes is compared with the clean twin B bit for
bit; B itself is held to the oracle by the rest of the suite.

One combination is left out: collect_mlp_dopri5(on_done="restart") with x[12] = +Inf.  There the env ends high, is restarted
inside the launch and ends the launch finite, which the oracle (no restarts) does not restate.

Every comparison is exact (sets of envs, bit patterns, the two clamp ends); there is no tolerance in this file."""
import ctypes as C

import numpy as np
import pytest

import support
from support import POISONS, STATUS_N, STATUS_POST, STATUS_PRE, gpu_torch as _torch, grid_action
from test_gpu_sensor_grid import OVERFLOW, PID, SMALL_PARK

pytestmark = pytest.mark.gpu

EXHAUSTED, NONFINITE, BAD_INDEX, SOLVER_FAILED = 1, 2, 4, 16
MLP_N, MLP_LANES = 256, (5, 250, 69)
GYM_KEYS = ("meal_time", "meal_amt", "start_minute", "episode", "cgm0")


def test_status_constants_are_the_headers():
    from simglucose_amd import _lib
    assert (_lib.T1D_ST_NORMALS_EXHAUSTED, _lib.T1D_ST_NONFINITE, _lib.T1D_ST_BAD_INDEX, _lib.T1D_ST_SOLVER_FAILED) == \
        (EXHAUSTED, NONFINITE, BAD_INDEX, SOLVER_FAILED)


def _dtype(name):
    return getattr(_torch(), name)


def _raised_status(e):
    """sync() with the default raise_on_status=True raises; -> the status word its message carries"""
    from simglucose_amd import _lib
    with pytest.raises(_lib.T1DError) as info:
        e.sync()
    return int(str(info.value).rsplit(" ", 1)[1])


# ------------------------------------------------------------------------------------------------ what drives an env
class _Step:
    """step() with the status inputs' action of every step"""
    calls = (1,) * STATUS_POST

    def __init__(self, e, inp, exact=False):
        self.e, self.inp, self.k = e, inp, 0

    def run(self, steps):
        torch = _torch()
        for _ in range(steps):
            self.e.step(torch.as_tensor(grid_action(self.inp, self.k), dtype=self.e.dtype, device=self.e.device))
            self.k += 1

    def extras(self):
        return {}


class _Rollout:
    """rollout_pid / rollout_bb (exact: their _dopri5 twins) with accumulators and a trace"""
    calls = (1, STATUS_POST - 1)

    def __init__(self, e, inp, exact=False, ctrl="pid"):
        self.e, self.ctrl, self.state = e, ctrl, None
        self.stats, self.trace = support.stats(e), e.new_trace(STATUS_PRE + STATUS_POST)
        self.fn = getattr(e, "rollout_%s%s" % (ctrl, "_dopri5" if exact else ""))

    def run(self, steps):
        if self.ctrl == "pid":
            self.state = self.fn(steps, *PID[:3], PID[3], pid_state=self.state, stats=self.stats, trace=self.trace)
        else:
            self.state = self.fn(steps, bb_state=self.state, stats=self.stats, trace=self.trace)

    def extras(self):
        d = {k: v for k, v in self.state.items()}
        d.update(self.stats)
        d.update({"trace_" + k: v for k, v in self.trace.items() if k != "row"})
        return d


class _Mlp:
    """rollout_mlp, or collect_mlp with exploration noise and on_done="restart" (exact: their _dopri5 twins)"""
    calls = (1, STATUS_POST - 1)

    def __init__(self, e, pol, exact=False, collect=False):
        torch = _torch()
        self.e, self.pol, self.collect, self.state = e, pol, collect, None
        self.stats = support.stats(e)
        cols = support.TRACES if collect else support.MLP_TRACE
        self.trace = e.new_trace(STATUS_PRE + STATUS_POST, columns=cols, history=pol.history)
        self.es, self.term = support.episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
        self.fn = getattr(e, ("collect_mlp" if collect else "rollout_mlp") + ("_dopri5" if exact else ""))

    def run(self, steps):
        if self.collect:
            self.state = self.fn(steps, self.pol, sigma=0.1, explore_seed=77, policy_state=self.state, stats=self.stats,
                                 trace=self.trace, on_done="restart", days=support.DAYS, terminal_obs=self.term, episode_stats=self.es)
        else:
            self.state = self.fn(steps, self.pol, policy_state=self.state, stats=self.stats, trace=self.trace)

    def extras(self):
        d = {k: v for k, v in self.state.items()}
        d.update(self.stats); d.update(self.es); d["terminal_obs"] = self.term
        d.update({"trace_" + k: v for k, v in self.trace.items() if k != "row"})
        return d


# ------------------------------------------------------------------------------------------------ 1(a) poisoned state
def _poisoned_pair(A, B, da, db, lanes, poison, expect, exact, keys, vmin, st):
    """A and B alike; STATUS_PRE steps; the word POISONS[poison] of A's `lanes`; then da.calls, after each of which:
    expect(steps since the poison) -> dict(x12_bad, bg_bad, done, last_cgm (None: not stated), gave_up) for the lanes."""
    torch = _torch()
    da.run(STATUS_PRE); db.run(STATUS_PRE)
    assert A.sync() == 0 and B.sync() == 0
    word, value = POISONS[poison]
    L = torch.as_tensor(lanes, device=A.device)
    A.x[word, L] = value
    clean = torch.as_tensor(np.setdiff1d(np.arange(A.n), lanes), device=A.device)
    lanes = np.asarray(lanes)
    steps = 0
    for j, k in enumerate(da.calls):
        da.run(k); db.run(k)
        steps += k
        want = expect(steps)
        stored = ~torch.isfinite(A.x[12])                       # read back: the flag is a promise about the stored state
        bits = (NONFINITE if bool(stored.any()) else 0) | (SOLVER_FAILED if want["gave_up"] else 0)
        # the word of this launch alone; it clears on read; the default sync() raises on it
        got = _raised_status(A) if j == len(da.calls) - 1 and bits else A.sync(raise_on_status=False)
        assert got == bits, (poison, j, got, bits)
        assert A.sync(raise_on_status=False) == 0
        assert B.sync() == 0
        # which envs are not finite: the oracle's sets
        assert sorted(stored.nonzero().flatten().tolist()) == sorted(lanes[want["x12_bad"]].tolist()), (poison, j)
        assert sorted((~torch.isfinite(A.bg)).nonzero().flatten().tolist()) == sorted(lanes[want["bg_bad"]].tolist()), (poison, j)
        # what such an env shows: done and the sensor's reading as the oracle has them; for a NaN BG that is done = 0 and
        # the sensor's lower end
        # the sample the launch ended on: with a one-minute sensor that is `cgm` itself (the held value is dead state
        # there, and the persistent single-minute kernel does not store it); otherwise the held value, last_cgm
        bad = L[torch.as_tensor(want["bg_bad"], device=A.device)]
        reading = A.cgm if st == 1 else A.last_cgm
        if len(bad):
            assert A.done[bad].cpu().tolist() == want["done"][want["bg_bad"]].tolist(), (poison, j)
            if want["last_cgm"] is not None:
                assert reading[bad].double().cpu().tolist() == want["last_cgm"][want["bg_bad"]].tolist(), (poison, j)
            nan = bad[torch.isnan(A.bg[bad])]
            assert bool((A.done[nan] == 0).all()) and bool((reading[nan] == vmin).all()), (poison, j)
        # isolation: every other env, bit for bit
        support.same_env_at(A, B, keys, clean, what=(poison, j))
        ea, eb = da.extras(), db.extras()
        support.same_env_at(ea, eb, tuple(ea), clean, what=(poison, j))
    assert steps == STATUS_POST


def _oracle_expect(sensor, exact, poison, n=STATUS_N, feed=3, meal_step=1):
    o = support.status_oracle(sensor, exact, poison, n, feed, meal_step)
    lanes = list(o["lanes"])

    def expect(steps):
        r = steps - 1
        return dict(x12_bad=o["x12_bad"][r, lanes], bg_bad=o["bg_bad"][r, lanes], done=o["done"][r, lanes],
                    last_cgm=o["last_cgm"][r, lanes], gave_up=bool(o["gave_up"][r]))
    return lanes, expect


def _per_lane_expect(exact, poison):
    """for the MLP paths, whose inputs the oracle does not restate: the oracle's answer for the status inputs, which is
    the same for every poisoned lane (asserted), applied to MLP_LANES"""
    o = support.status_oracle("Dexcom", exact, poison)
    lanes = list(o["lanes"])
    inp = support.status_inputs("Dexcom")

    def expect(steps):
        r = steps - 1
        out = {}
        for k in ("x12_bad", "bg_bad", "done"):
            v = o[k][r, lanes]
            assert (v == v[0]).all()
            out[k] = np.full(len(MLP_LANES), v[0])
        # the sensor's reading is stated where BG is not finite: it is one of the two clamp ends
        cg = o["last_cgm"][r, lanes]
        out["last_cgm"] = None
        if out["bg_bad"][0]:
            assert (cg == cg[0]).all() and cg[0] in (inp["vmin"], inp["vmax"])
            out["last_cgm"] = np.full(len(MLP_LANES), cg[0])
        out["gave_up"] = bool(o["gave_up"][r])
        return out
    return expect


STEP_PATHS = {                                  # name -> sensor, every feed-th env fed, in the first minute of which step, options
    "generic_navigator": ("Navigator", 3, 1, (("single_minute_kernel", 0),)),
    "generic_dexcom": ("Dexcom", 3, 1, ()),
    "single_minute": ("Navigator", 3, 1, ()),
    "single_minute_set_aside": ("Navigator", 3, 1, (("adaptive_gut", 3),)),
    "single_minute_in_place": ("Navigator", 3, 1, (("adaptive_gut", 2),)),
    "multi_minute_small_park": ("Dexcom", 3, 1, SMALL_PARK),
    "multi_minute_overflow": ("Dexcom", 1, STATUS_PRE, OVERFLOW),
}
ROLLOUT_FORMS = {"one_launch": (("rollout_launches", 0),), "launch_per_step": (("rollout_launches", 2), ("multi_minute_kernel", 2))}


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("path", list(STEP_PATHS))
def test_poisoned_state_through_the_step_kernels(path, dtype, poison):
    """the generic step kernel at one and at three minutes per step, the persistent single-minute kernel in its three forms,
    the persistent multi-minute kernel with few records and with more lanes of level 2 than records"""
    sensor, feed, meal_step, options = STEP_PATHS[path]
    inp = support.status_inputs(sensor, STATUS_N, feed, meal_step)
    lanes, expect = _oracle_expect(sensor, False, poison, STATUS_N, feed, meal_step)
    A, B = (support.status_env(sensor, STATUS_N, feed, options, _dtype(dtype), meal_step=meal_step) for _ in range(2))
    _poisoned_pair(A, B, _Step(A, inp), _Step(B, inp), lanes, poison, expect, False, support.STATE, inp["vmin"], inp["st"])


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("form", list(ROLLOUT_FORMS))
@pytest.mark.parametrize("ctrl", ["pid", "bb"])
def test_poisoned_state_through_the_rollouts(ctrl, form, dtype, poison):
    """rollout_pid and rollout_bb, all steps of a call in one launch and one launch of the multi-minute kernel per step:
    also the controller state, the accumulators and the trace rows of every other env"""
    inp = support.status_inputs("Dexcom")
    lanes, expect = _oracle_expect("Dexcom", False, poison)
    A, B = (support.status_env("Dexcom", options=ROLLOUT_FORMS[form], dtype=_dtype(dtype)) for _ in range(2))
    _poisoned_pair(A, B, _Rollout(A, inp, ctrl=ctrl), _Rollout(B, inp, ctrl=ctrl), lanes, poison, expect, False, support.STATE,
                   inp["vmin"], inp["st"])


@pytest.mark.parametrize("poison", list(POISONS))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("collect", [False, True], ids=["rollout_mlp", "collect_mlp_restart"])
def test_poisoned_state_through_the_mlp_paths(collect, dtype, poison):
    """rollout_mlp, and collect_mlp with on_done="restart": a poisoned env is never done, so never restarted"""
    pol = support.random_policy(widths=(8, 1), n_policies=2, seed=4)
    A, B = (support.gym_env(MLP_N, _dtype(dtype)) for _ in range(2))
    _poisoned_pair(A, B, _Mlp(A, pol, collect=collect), _Mlp(B, pol, collect=collect), MLP_LANES, poison,
                   _per_lane_expect(False, poison), False, support.STATE + GYM_KEYS, float(A.sensor_row[6]), 3)
    assert bool((A.episode[list(MLP_LANES)] == B.episode[list(MLP_LANES)]).all())


EXACT_PATHS = ("step", "rollout_pid_dopri5", "rollout_mlp_dopri5", "collect_mlp_dopri5")
# (the collector with x[12] = +Inf: the module docstring)
EXACT_CASES = [(p, q) for p in EXACT_PATHS for q in POISONS if (p, q) != ("collect_mlp_dopri5", "x12_inf")]


@pytest.mark.parametrize("path,poison", EXACT_CASES)
def test_poisoned_state_through_the_exact_mode(path, poison):
    """t1d_step_dopri5 and the exact-mode roll-outs: the solver gives up on the poisoned env (T1D_ST_SOLVER_FAILED in every
    launch), the env keeps its state, and T1D_ST_NONFINITE follows the stored x[12] as everywhere"""
    keys = support.STATE_EXACT + ("nfev",)
    if path in ("step", "rollout_pid_dopri5"):
        inp = support.status_inputs("Dexcom")
        lanes, expect = _oracle_expect("Dexcom", True, poison)
        A, B = (support.status_env("Dexcom", exact=True) for _ in range(2))
        mk = (lambda e: _Step(e, inp)) if path == "step" else (lambda e: _Rollout(e, inp, exact=True))
        _poisoned_pair(A, B, mk(A), mk(B), lanes, poison, expect, True, keys, inp["vmin"], inp["st"])
    else:
        pol = support.random_policy(widths=(8, 1), n_policies=2, seed=4)
        A, B = (support.gym_env(MLP_N, exact=True) for _ in range(2))
        collect = path == "collect_mlp_dopri5"
        _poisoned_pair(A, B, _Mlp(A, pol, exact=True, collect=collect), _Mlp(B, pol, exact=True, collect=collect), MLP_LANES, poison,
                       _per_lane_expect(True, poison), True, keys + GYM_KEYS, float(A.sensor_row[6]), 3)


# ------------------------------------------------------------------------------------------------ 1(b) NaN action
ACTION_PATHS = {"single_minute": ("Navigator", (), False), "generic_dexcom": ("Dexcom", (), False),
                "multi_minute": ("Dexcom", (("multi_minute_kernel", 2),), False), "exact": ("Dexcom", (), True)}
ACTION_CASES = [(p, d) for p in ACTION_PATHS for d in (("float64",) if p == "exact" else ("float64", "float32"))]


def _keys(exact):
    return support.STATE_EXACT + ("nfev",) if exact else support.STATE


@pytest.mark.parametrize("arm", ["basal", "bolus"])
@pytest.mark.parametrize("use_pump", [True, False], ids=["pump_on", "pump_off"])
@pytest.mark.parametrize("path,dtype", ACTION_CASES)
def test_nan_action_in_step(path, dtype, use_pump, arm):
    """step() with NaN in the basal (the bolus) of three lanes.  The reference's pump hands a NaN amount on (Python's
    min(v, hi), max(v, lo)): the recorded insulin of those envs is NaN -- not the pump's maximum -- and the launch raises
    T1D_ST_NONFINITE (exact mode: the solver gives up instead and the state stays as it was).  Every other env equals the
    clean twin.  With the pump on this fails where pump_quantise clamps with the mirrored selects."""
    torch = _torch()
    sensor, options, exact = ACTION_PATHS[path]
    inp = support.status_inputs(sensor)
    lanes = list(support.status_lanes(sensor))
    A, B = (support.status_env(sensor, options=options, dtype=_dtype(dtype), exact=exact, use_pump=use_pump) for _ in range(2))
    t = lambda v: torch.as_tensor(v, dtype=A.dtype, device=A.device)
    clean = torch.as_tensor(np.setdiff1d(np.arange(A.n), lanes), device=A.device)
    basal, bolus = grid_action(inp, 0), np.zeros(A.n)
    bad_basal, bad_bolus = basal.copy(), bolus.copy()
    (bad_basal if arm == "basal" else bad_bolus)[lanes] = np.nan
    A.step(t(bad_basal), t(bad_bolus)); B.step(t(basal), t(bolus))
    stored = ~torch.isfinite(A.x[12])
    st = A.sync(raise_on_status=False)
    assert bool(torch.isnan(A.insulin[lanes]).all()), A.insulin[lanes]
    if exact:
        assert st == SOLVER_FAILED and not bool(stored.any())
    else:
        assert st == NONFINITE and stored.nonzero().flatten().tolist() == sorted(lanes)
        reading = A.cgm if inp["st"] == 1 else A.last_cgm       # the sample the launch ended on (_poisoned_pair)
        assert bool((A.done[lanes] == 0).all()) and bool((reading[lanes] == inp["vmin"]).all())
    assert A.sync(raise_on_status=False) == 0 and B.sync() == 0
    support.same_env_at(A, B, _keys(exact), clean)
    # a clean action afterwards: the fixed-step env stays poisoned and says so again, the others stay the twin's
    A.step(t(grid_action(inp, 1)), t(bolus)); B.step(t(grid_action(inp, 1)), t(bolus))
    assert A.sync(raise_on_status=False) == (0 if exact else NONFINITE) and B.sync() == 0
    support.same_env_at(A, B, _keys(exact), clean)


@pytest.mark.parametrize("sign,limit", [(1.0, "max_basal"), (-1.0, "min_basal")], ids=["plus_inf", "minus_inf"])
@pytest.mark.parametrize("path,dtype", ACTION_CASES)
def test_infinite_action_in_step_is_the_pumps_limit(path, dtype, sign, limit):
    """+Inf / -Inf through the pump: no bit, and the env equals a twin given max_basal / min_basal, bit for bit -- the
    reference's min / max.  (Found here: the fp64 quantiser scaled back to U/min with a residual-corrected division,
    Inf - Inf = NaN, which the mirrored clamps then turned into max_basal for -Inf as well.)"""
    torch = _torch()
    sensor, options, exact = ACTION_PATHS[path]
    inp = support.status_inputs(sensor)
    lanes = list(support.status_lanes(sensor))
    A, B = (support.status_env(sensor, options=options, dtype=_dtype(dtype), exact=exact) for _ in range(2))
    row = dict(zip(("min_bolus", "max_bolus", "inc_bolus", "min_basal", "max_basal", "inc_basal"), A.pump_row))
    ua, ub = grid_action(inp, 0).copy(), grid_action(inp, 0).copy()
    ua[lanes] = sign * np.inf
    ub[lanes] = row[limit]
    t = lambda v: torch.as_tensor(v, dtype=A.dtype, device=A.device)
    for k in range(2):
        A.step(t(ua)); B.step(t(ub))
        assert A.sync() == 0 and B.sync() == 0
        support.same_env(A, B, _keys(exact))
    assert bool(torch.isfinite(A.x).all())


MLP_ACTION_PATHS = {"rollout_mlp": (False, False), "collect_mlp_restart": (False, True), "rollout_mlp_dopri5": (True, False),
                    "collect_mlp_dopri5_restart": (True, True)}
MLP_ACTION_CASES = [(p, d) for p, (ex, _) in MLP_ACTION_PATHS.items() for d in (("float64",) if ex else ("float64", "float32"))]


@pytest.mark.parametrize("use_pump", [True, False], ids=["pump_on", "pump_off"])
@pytest.mark.parametrize("path,dtype", MLP_ACTION_CASES)
def test_nan_weight_poisons_its_policys_envs_alone(path, dtype, use_pump):
    """two policies of 128 envs, one weight of policy 1 NaN: every env of policy 1 asks for a NaN basal in every step.  Its
    action_trace and its recorded insulin are NaN (not max_basal), the first launch raises T1D_ST_NONFINITE (exact mode:
    T1D_ST_SOLVER_FAILED, the state stays), and policy 0's envs equal the twin under the clean weights bit for bit."""
    torch = _torch()
    exact, collect = MLP_ACTION_PATHS[path]
    good = support.random_policy(widths=(8, 1), n_policies=2, seed=4)
    bad = support.random_policy(widths=(8, 1), n_policies=2, seed=4)
    bad.W[0][1, 0, 0] = float("nan")
    bad.invalidate()
    A, B = (support.gym_env(MLP_N, _dtype(dtype), exact=exact, use_pump=use_pump) for _ in range(2))
    da, db = _Mlp(A, bad, exact=exact, collect=collect), _Mlp(B, good, exact=exact, collect=collect)
    half = MLP_N // 2
    first = torch.arange(half, device=A.device)
    keys = _keys(exact) + GYM_KEYS
    row = 1
    for j, k in enumerate((1, 2)):
        da.run(k); db.run(k)
        stored = ~torch.isfinite(A.x[12])
        st = A.sync(raise_on_status=False)
        if exact:
            assert st == SOLVER_FAILED and not bool(stored.any()), (j, st)
        else:
            assert st == NONFINITE and stored.nonzero().flatten().tolist() == list(range(half, MLP_N)), (j, st)
            assert bool((A.done[half:] == 0).all())
        assert A.sync(raise_on_status=False) == 0 and B.sync() == 0
        assert bool(torch.isnan(A.insulin[half:]).all())
        for r in range(row, row + k):
            assert bool(torch.isnan(da.trace["action"][r, half:]).all()) and bool(torch.isnan(da.trace["insulin"][r, half:]).all())
            assert bool(torch.isfinite(da.trace["action"][r, :half]).all())
        row += k
        support.same_env_at(A, B, keys, first, what=j)
        ea, eb = da.extras(), db.extras()
        support.same_env_at(ea, eb, tuple(ea), first, what=j)


# ------------------------------------------------------------------------------------------------ 1(c) normals exhausted
NORMALS_PATHS = {"generic_inline_refill": ((("split_refill", 0),), False), "default": ((), False), "exact": ((), True)}
NORMALS_STEPS = 51                              # past minute 150


def _normals_pair(short, path):
    """A: the first `short` rows of B's 21, where B's rows from `short` on (a dropped pair as a whole) are zero"""
    options, exact = NORMALS_PATHS[path]
    rs = np.random.RandomState(31)
    zb = rs.randn(21, STATUS_N)
    zb[short - (short - 1) % 2:] = 0.0          # rows 1.. pair up as (1, 2), (3, 4), ...: from the first row of the pair cut into
    za = zb[:short].copy()
    A = support.status_env("Dexcom", options=options, exact=exact, z=za)
    B = support.status_env("Dexcom", options=options, exact=exact, z=zb)
    return A, B, _keys(exact)


@pytest.mark.parametrize("short", [11, 20], ids=["block_0_only", "last_pair_cut"])
@pytest.mark.parametrize("path", list(NORMALS_PATHS))
def test_normals_exhausted_is_raised_by_the_launch_that_opens_the_block(path, short):
    """Host normals, Dexcom: reset takes samples #0 and #1, step k (from 0) sample #k + 2, and a noise block holds 50
    samples, so block 1 -- rows 11 to 20 -- is built by step 48.  A has 11 rows (block 0 only), or 20 (the pair of rows 19
    and 20 is cut: dropped whole); B has 21 with zeros where A has nothing.  A raises T1D_ST_NORMALS_EXHAUSTED in that launch
    and in no other, B never, and A equals B bit for bit throughout: zeros were used."""
    torch = _torch()
    inp = support.status_inputs("Dexcom")
    A, B, keys = _normals_pair(short, path)
    assert A.sync() == 0 and B.sync() == 0
    support.same_env(A, B, keys)
    raised = []
    for k in range(NORMALS_STEPS):
        u = torch.as_tensor(grid_action(inp, k), dtype=A.dtype, device=A.device)
        A.step(u); B.step(u)
        sa = A.sync(raise_on_status=False)
        assert B.sync() == 0
        if sa:
            raised.append((k, sa))
        support.same_env(A, B, keys)
    assert int(A.t[0]) == 3 * NORMALS_STEPS > 150
    assert raised == [(48, EXHAUSTED)], raised


@pytest.mark.parametrize("path", ["default", "exact"])
def test_one_row_of_normals_is_exhausted_by_reset(path):
    """a one-row tensor: reset() itself builds block 0 from zeros and says so; equal to a reset with row 0 and ten zero rows"""
    torch = _torch()
    options, exact = NORMALS_PATHS[path]
    inp = support.status_inputs("Dexcom")
    zb = np.zeros((11, STATUS_N))
    zb[0] = np.random.RandomState(32).randn(STATUS_N)
    A = support.status_env("Dexcom", options=options, exact=exact, z=zb[:1].copy())
    B = support.status_env("Dexcom", options=options, exact=exact, z=zb)
    assert A.sync(raise_on_status=False) == EXHAUSTED and A.sync(raise_on_status=False) == 0 and B.sync() == 0
    support.same_env(A, B, _keys(exact) + ("cgm0",))
    for k in range(3):
        u = torch.as_tensor(grid_action(inp, k), dtype=A.dtype, device=A.device)
        A.step(u); B.step(u)
        assert A.sync() == 0 and B.sync() == 0
        support.same_env(A, B, _keys(exact))


# ------------------------------------------------------------------------------------------------ 1(d) bad index
def _model_rhs(e, g, pid, math, m):
    """t1d_model_rhs itself on the first m points of fixture G1: the Python wrapper refuses the indices this test is about"""
    from simglucose_amd import _lib
    torch = _torch()
    t = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt).to(e.device).contiguous()
    x, pidt = t(g["x"][:m].T), t(pid, torch.int32)
    args = [t(g[k][:m]) for k in ("cho", "insulin", "last_qsto", "last_foodtaken")]
    out = torch.empty(13, m, dtype=torch.float64, device=e.device)
    p = lambda v: C.c_void_p(v.data_ptr())
    with torch.cuda.device(e.device):
        _lib.check(e._L.t1d_model_rhs(e._ctx, _lib.T1D_F64, m, int(math), p(x), p(pidt), p(args[0]), p(args[1]), p(args[2]), p(args[3]),
                                      p(out), e._stream()))
    return out


@pytest.mark.parametrize("math", [0, 1])
def test_bad_patient_index_is_reported_and_row_0_used(golden, math):
    """t1d_model_rhs on 300 points with the patient index replaced, in a few places, by np (= 30), 255, -1 and INT32_MIN:
    T1D_ST_BAD_INDEX, those points equal the call with index 0, all others the clean call, bit for bit"""
    torch = _torch()
    g, m = golden("g1_rhs.npz"), 300
    e = support.plain_env(patient="adult#001", n_envs=1, sensor="Navigator")
    npat = len(e.names)
    assert npat == 30
    pid = np.asarray(g["patient_idx"][:m], dtype=np.int64)
    where = {3: npat, 63: 255, 64: -1, 150: -2 ** 31, 299: npat, 200: -1}
    bad, zero = pid.copy(), pid.copy()
    for i, v in where.items():
        bad[i], zero[i] = v, 0
    ref = _model_rhs(e, g, pid, math, m)
    assert e.sync() == 0
    ref0 = _model_rhs(e, g, zero, math, m)
    assert e.sync() == 0
    got = _model_rhs(e, g, bad, math, m)
    assert e.sync(raise_on_status=False) == BAD_INDEX and e.sync(raise_on_status=False) == 0
    idx = torch.as_tensor(sorted(where), device=e.device)
    rest = torch.as_tensor(np.setdiff1d(np.arange(m), sorted(where)), device=e.device)
    assert torch.equal(support.bits(got.index_select(1, idx)), support.bits(ref0.index_select(1, idx)))
    assert torch.equal(support.bits(got.index_select(1, rest)), support.bits(ref.index_select(1, rest)))
    assert not torch.equal(ref0.index_select(1, idx), ref.index_select(1, idx))      # row 0 is another patient's
    _model_rhs(e, g, bad, math, m)
    assert _raised_status(e) == BAD_INDEX
