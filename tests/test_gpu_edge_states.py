"""Model branch points through every stepping kernel.

The suite holds every kernel family to the oracle on ordinary trajectories and (test_gpu_status.py) on non-finite data.
Here the data are finite and sit where the model itself branches: x3, x4 and x12 below 0 (the reference holds them), an x3
that falls through 0 in the first or in the second minute of a step, x3 passing the renal threshold ke2 in both directions,
EGPt below 0, BG a little beyond 70 and 350 mg/dL.  These are the states that a kernel which keeps a lane in registers across
minutes, parks it in LDS "as at the start of the minute" or re-enters a solver can lose without any ordinary trajectory
noticing.

Inputs: support.status_inputs -- 150 envs, two full 64-env chunks and a partial one, all 30 patients -- stepped STATUS_PRE
times; then support.edge_states edits the state (the same function edits the oracle's: support.edge_oracle); then STATUS_POST
more steps.  Every kind of edit sits in lanes of all three chunks.  test_edge_states_host.py shows on the CPU that the oracle
reaches every branch, in minutes that the step-size rule puts at level 2, that no BG ends a step within 1e-6 mg/dL of a
`done` threshold (the closest is 0.028), and that the all-fed batch of the overflow case leaves more lanes at level 2 than
the workgroup has records.  The MLP paths take support.gym_env(256) under two policies, edited by the same function.

The drivers (_Step, _Rollout), the table of step paths and the roll-out forms are test_gpu_status.py's; the roll-outs'
step loops are test_gpu_sensor_grid.py's and test_gpu_dopri5_rollout.py's; the MLP paths' loop is support.loop_of_entry_points.

Tolerances, all the project's own: TOL_ORACLE (test_gpu_parity.py) on BG, CGM and last_cgm and, relative to max(1, |x|), on
the 13 states; 1e-6 on reward and risk; TOL_F32 (test_gpu_step_trim.py) for fp32 against fp64; TOL_KERNELS and TOL_KERNELS_X
(test_gpu_sensor_grid.py) kernel against kernel; the roll-outs against their loops as test_gpu_sensor_grid.py bounds them
(1e-9, the PID's integral 1e-6, prev_meal 1e-12; fp32: that file's kernel-against-kernel bounds TOL_KERNELS_F32 and
TOL_KERNELS_X_F32, the integral K st times the former, since it sums K readings times st); the exact mode as
test_gpu_dopri5.py holds a heterogeneous batch (95 % of the envs within 1e-8, none beyond 5e-4).  No lane is left out of
any comparison.  Every case prints its worst values; profiles/edge_states/README.md has them as measured on an MI355X."""
import functools

import numpy as np
import pytest

import support
from support import EDGE_CROSSING, EDGE_HELD, EDGE_LANES, EDGE_OUT, EDGE_SNAP, STATUS_N, STATUS_POST, STATUS_PRE, gpu_torch as _torch
from test_gpu_dopri5_rollout import STATE as EXACT_LOOP_STATE, _step_loop as _exact_step_loop
from test_gpu_parity import TOL_ORACLE, _env as _variant_env, _integ
from test_gpu_sensor_grid import (LOOP_KEYS, OVERFLOW_CAP, PID, TOL_KERNELS, TOL_KERNELS_F32, TOL_KERNELS_X, TOL_KERNELS_X_F32,
                                  _once, _step_by_step)
from test_gpu_status import GYM_KEYS, MLP_N, ROLLOUT_FORMS, STEP_PATHS, _Rollout, _Step, _dtype
from test_gpu_step_trim import TOL_F32

pytestmark = pytest.mark.gpu

HELD = {kind: word for kind, (word, _) in EDGE_HELD.items()}
K = STATUS_PRE + STATUS_POST
# name -> sensor, every feed-th env fed, in the first minute of which step, options, the generic kernel's variant or None
PATHS = {name: row + (None,) for name, row in STEP_PATHS.items()}
PATHS["generic_refill_inline"] = ("Dexcom", 3, 1, (("split_refill", 0),), None)
for _v in ("ref", "rk4", "split"):              # test_gpu_parity.VARIANTS that are not the default scheme or its inline refill
    PATHS["generic_dexcom_" + _v] = ("Dexcom", 3, 1, (), _v)
    PATHS["generic_navigator_" + _v] = ("Navigator", 3, 1, (("single_minute_kernel", 0),), _v)
# for the overflow case's kernel-against-kernel comparison: the generic kernel on the all-fed inputs
ALL_FED = ("Dexcom", 1, STATUS_PRE, (), None)


@pytest.fixture(scope="module")
def shared():
    """device runs that several cases compare with, each made by the first case that asks and kept on the host"""
    return {}


def _scheme(path):
    variant = (PATHS.get(path) or ALL_FED)[4]
    return "split_adaptive" if variant is None else _integ(variant)


def _device_run(path, dtype, inputs=support.status_inputs, write=lambda e, pid: support.edge_states(e.x, pid), keys=EDGE_OUT):
    """K steps of the status inputs' actions with the edge states written after STATUS_PRE of them -> EDGE_OUT after every
    step as fp64 arrays [K, n] (x: [K, 13, n]), raw_x / raw_edit = the states and the state as written in the env's own
    precision.  inputs, write(env, pid), keys: other inputs of the same shape, another edit, the attributes to record
    (test_gpu_gut_states.py)"""
    torch = _torch()
    sensor, feed, meal_step, options, variant = PATHS.get(path) or ALL_FED
    inp = inputs(sensor, STATUS_N, feed, meal_step)
    make = None if variant is None else functools.partial(_variant_env, variant)
    e = support.status_env(sensor, STATUS_N, feed, options, _dtype(dtype), meal_step=meal_step, make=make, inputs=inputs)
    d = _Step(e, inp)
    rows = {k: [] for k in keys}
    for k in range(K):
        if k == STATUS_PRE:
            assert write(e, inp["pid"]) is (EDGE_LANES if inputs is support.status_inputs else support.GUT_LANES)
            edit = e.x.clone()
        d.run(1)
        for key in keys:
            rows[key].append(getattr(e, key).clone())
    assert e.sync() == 0                                        # nothing non-finite, no normal missing, no stall
    assert int(e.t.min()) == int(e.t.max()) == K * inp["st"]
    out = {k: torch.stack(v).double().cpu().numpy() for k, v in rows.items()}
    out.update(raw_x=torch.stack(rows["x"]).cpu().numpy(), raw_edit=edit.cpu().numpy(), st=inp["st"])
    return out


def _run(shared, path, dtype="float64"):
    return _once(shared, (path, dtype), lambda: _device_run(path, dtype))


def _oracle(path):
    sensor, feed, meal_step, _, _ = PATHS.get(path) or ALL_FED
    return support.edge_oracle(sensor, _scheme(path), feed, meal_step)


def _words(a):
    return np.ascontiguousarray(a).view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _held_and_snapped(got, snapped, adaptive=True):
    """the exact part: a word below 0 stays what was written, bit for bit; in the schemes that snap, an x3 that a step took
    below 0 reads -1e-10 (in the env's precision) wherever `snapped` [K, n] says so, and then stays"""
    raw, edit = got["raw_x"], got["raw_edit"]
    for kind, word in HELD.items():
        L = list(EDGE_LANES[kind])
        assert np.array_equal(_words(edit[word, L]), _words(np.full(len(L), EDGE_HELD[kind][1], dtype=edit.dtype))), kind
        for k in range(STATUS_PRE, K):
            assert np.array_equal(_words(raw[k, word, L]), _words(edit[word, L])), (kind, k)
    if adaptive:
        L = support.edge_lanes(*EDGE_CROSSING)
        assert snapped[-1, L].all() and not snapped[:STATUS_PRE].any()
        assert np.array_equal(raw[:, 3][snapped], np.full(int(snapped.sum()), EDGE_SNAP, dtype=raw.dtype))


def _worst(got, ref, st):
    w = {k: float(np.abs(got[k] - ref[k]).max()) for k in ("cgm", "bg", "reward", "risk")}
    # with a one-minute sensor `cgm` is the sample itself; the held value is dead state there, and the persistent
    # single-minute kernel does not store it (test_gpu_status.py, _poisoned_pair)
    w["last_cgm"] = float(np.abs(got["last_cgm"] - ref["last_cgm"]).max()) if st != 1 else 0.0
    w["x"] = float((np.abs(got["x"] - ref["x"]) / np.maximum(1.0, np.abs(ref["x"]))).max())
    w["done"] = int((got["done"] != ref["done"]).sum())
    return w


def _show(group, label, w):
    print("\n[edge states] %s %s: %s" % (group, label, " ".join(("%s %d" if isinstance(v, int) else "%s %.2e") % (k, v) for k, v in w.items())))


# ------------------------------------------------------------------------------------------------ (a) against the oracle
@pytest.mark.parametrize("path", list(PATHS))
def test_step_kernels_follow_the_oracle_through_the_branch_points(shared, path):
    """every entry of test_gpu_status.STEP_PATHS, the generic kernel with the refill inline and the generic kernel's other
    schemes, fp64, each against the oracle's restatement of its scheme, after every step"""
    got, ref = _run(shared, path), _oracle(path)
    w = _worst(got, ref, got["st"])
    _show("(a) oracle", path, w)
    assert all(np.isfinite(got[k]).all() for k in EDGE_OUT)
    assert w["cgm"] < TOL_ORACLE and w["bg"] < TOL_ORACLE and w["last_cgm"] < TOL_ORACLE, w
    assert w["x"] < TOL_ORACLE, w
    assert w["reward"] < 1e-6 and w["risk"] < 1e-6, w
    assert w["done"] == 0 and got["done"][STATUS_PRE:].any()
    adaptive = _scheme(path) != "rk4"                           # classical RK4 steps through 0 and stays where it lands
    _held_and_snapped(got, ref["x"][:, 3] == EDGE_SNAP, adaptive)
    if path == "multi_minute_overflow":
        assert ref["level2"][STATUS_PRE] - OVERFLOW_CAP >= 64    # (test_edge_states_host.py: in its first minute alone)


# ------------------------------------------------------------------------------------------------ (b) fp32 against fp64
@pytest.mark.parametrize("path", list(PATHS))
def test_fp32_step_kernels_track_fp64_through_the_branch_points(shared, path):
    got, ref = _run(shared, path, "float32"), _run(shared, path)
    w = {k: float(np.abs(got[k] - ref[k]).max()) for k in ("bg", "cgm")}
    w["done"] = int((got["done"] != ref["done"]).sum())
    _show("(b) fp32", path, w)
    assert got["raw_x"].dtype == np.float32 and all(np.isfinite(got[k]).all() for k in EDGE_OUT)
    assert w["bg"] < TOL_F32 and w["cgm"] < TOL_F32, w
    assert w["done"] == 0
    _held_and_snapped(got, ref["raw_x"][:, 3] == EDGE_SNAP, _scheme(path) != "rk4")


# ------------------------------------------------------------------------------------------------ (c) kernel against kernel
PAIRS = [(a, b) for i, a in enumerate(("generic_navigator", "single_minute", "single_minute_set_aside", "single_minute_in_place"))
         for b in ("generic_navigator", "single_minute", "single_minute_set_aside", "single_minute_in_place")[i + 1:]] + \
        [("multi_minute_small_park", "generic_dexcom"), ("multi_minute_overflow", "generic_dexcom_all_fed")]


@pytest.mark.parametrize("a,b", PAIRS)
def test_step_kernels_agree_through_the_branch_points(shared, a, b):
    """the one-minute forms with each other, the multi-minute kernel (few records; more lanes at level 2 than records)
    with the generic kernel on the same inputs, fp64"""
    ra, rb = _run(shared, a), _run(shared, b)
    w = _worst(ra, rb, ra["st"])
    w["x_abs"] = float(np.abs(ra["x"] - rb["x"]).max())
    _show("(c) kernels", "%s / %s" % (a, b), w)
    for k in ("cgm", "bg", "reward", "risk", "last_cgm"):
        assert w[k] < TOL_KERNELS, (k, w)
    assert w["x_abs"] < TOL_KERNELS_X and w["done"] == 0, w


# ------------------------------------------------------------------------------------------------ (d) closed loops
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("form", list(ROLLOUT_FORMS))
@pytest.mark.parametrize("ctrl", ["pid", "bb"])
def test_rollouts_match_their_step_loops_through_the_branch_points(shared, ctrl, form, dtype):
    """rollout_pid / rollout_bb in calls of STATUS_PRE, 1 and STATUS_POST - 1 steps, all steps of a call in one launch or
    one launch of the multi-minute kernel per step, against the controller on the host around step()"""
    torch = _torch()
    inp = support.status_inputs("Dexcom")
    st = inp["st"]

    def loop():
        e = support.status_env("Dexcom", dtype=_dtype(dtype))
        out = _step_by_step(st, ctrl, e, K, lambda k: k == STATUS_PRE and support.edge_states(e.x, inp["pid"]))
        out["done"] = e.done.cpu()
        return out
    ref = _once(shared, ("loop", ctrl, dtype), loop)
    e = support.status_env("Dexcom", options=ROLLOUT_FORMS[form], dtype=_dtype(dtype))
    d = _Rollout(e, inp, ctrl=ctrl)
    d.run(STATUS_PRE)
    support.edge_states(e.x, inp["pid"])
    edit = e.x.clone()
    for k in d.calls:
        d.run(k)
    assert e.sync() == 0 and int(e.t.min()) == int(e.t.max()) == K * st
    worst = {k: float((getattr(e, k).double().cpu() - ref[k].double()).abs().max()) for k in LOOP_KEYS}
    ctl = {k: float((d.state[k].double().cpu() - ref[k].double()).abs().max()) for k in (("integ", "prev") if ctrl == "pid" else ("prev_meal",))}
    worst.update(ctl)
    worst["done"] = int((e.done.cpu() != ref["done"]).sum())
    _show("(d) roll-outs", "rollout_%s %s %s" % (ctrl, form, dtype), worst)
    tol, tol_x = (1e-9, 1e-9) if dtype == "float64" else (TOL_KERNELS_F32, TOL_KERNELS_X_F32)
    assert worst["t"] == 0
    for k in LOOP_KEYS:
        assert worst[k] < (tol_x if k == "x" else tol), (k, worst)
    if ctrl == "pid":
        assert ctl["integ"] < (1e-6 if dtype == "float64" else K * st * TOL_KERNELS_F32) and ctl["prev"] < tol, ctl
    else:
        assert ctl["prev_meal"] < (1e-12 if dtype == "float64" else tol), ctl
    assert worst["done"] == 0 and bool(e.done.any())
    for kind, word in HELD.items():                             # held through the roll-out's launches, to the bit
        L = list(EDGE_LANES[kind])
        assert torch.equal(support.bits(e.x[word, L]), support.bits(edit[word, L])), kind
    L = support.edge_lanes(*EDGE_CROSSING)
    assert bool((e.x[3, L] == torch.as_tensor(EDGE_SNAP, dtype=e.dtype)).all())


def _mlp_pair(collect, exact, write=lambda e: support.edge_states(e.x, e.patient_idx)):
    """A: rollout_mlp (collect: collect_mlp with on_done="restart"; exact: their _dopri5 twins) in launches of STATUS_PRE and
    STATUS_POST steps; B: support.loop_of_entry_points; the edge states written into both after the first launch (write(env):
    another edit, test_gpu_gut_states.py); equal bit for bit -> (A, B's episode counters before the second launch, A's state
    as edited)"""
    torch = _torch()
    pol = support.random_policy(widths=(8, 1), n_policies=2, seed=4)
    A, B = (support.gym_env(MLP_N, exact=exact) for _ in range(2))
    cols = support.MLP_TRACE + ("reward", "done")
    z = lambda: torch.zeros(MLP_N, dtype=A.dtype, device=A.device)
    sa, ta, terma, esa = support.stats(A), A.new_trace(K, columns=cols if collect else support.MLP_TRACE), z(), support.episode_stats(A)
    sb, tb, termb, esb = support.stats(B), B.new_trace(K, columns=cols), z(), support.episode_stats(B)
    fn = getattr(A, ("collect_mlp" if collect else "rollout_mlp") + ("_dopri5" if exact else ""))
    kw = dict(on_done="restart", days=support.DAYS, terminal_obs=terma, episode_stats=esa) if collect else {}
    sta = stb = None
    nfa, nfb = (torch.zeros(MLP_N, dtype=torch.int64, device=A.device) for _ in range(2))
    for steps in (STATUS_PRE, STATUS_POST):
        if steps == STATUS_POST:
            write(A); write(B)
            edit, before = A.x.clone(), B.episode.clone()
        sta = fn(steps, pol, policy_state=sta, stats=sa, trace=ta, **kw)
        nfa += A.nfev if exact else 0
        stb, low, high, nf = support.loop_of_entry_points(B, pol, steps, sb, tb, termb, esb, exact, st=stb, restart=collect)
        nfb += nf
    assert A.sync() == 0
    support.same_env(B, A, keys=(support.STATE_EXACT if exact else support.STATE) + GYM_KEYS)
    support.same_dicts(stb, sta, support.POLICY_STATE)
    support.same_dicts(sb, sa, support.STATS)
    support.same_dicts(tb, ta, cols if collect else support.MLP_TRACE)
    assert torch.equal(nfa, nfb)
    if collect:
        support.same_dicts(esb, esa, support.EPISODE_STATS)
        assert torch.equal(support.bits(termb), support.bits(terma))
    return A, before, edit, int(low), int(high)


def _mlp_case(collect, exact):
    torch = _torch()
    A, before, edit, low, high = _mlp_pair(collect, exact)
    restarted = (A.episode > before).cpu().numpy()
    print("\n[edge states] (%s) %s%s: bit for bit; restarted in the launch after the edit %s, endings of the reference loop < 70: %d, > 350: %d"
          % ("e" if exact else "d", "collect_mlp" if collect else "rollout_mlp", "_dopri5" if exact else "", np.nonzero(restarted)[0].tolist(), low, high))
    assert low > 0 and high > 0                                 # on the reference loop: `done` was raised at both ends
    if collect:
        # a done_high lane that also holds x4 < 0 was restarted inside the launch: its episode advanced and its state came
        # back from the held word to a fresh patient's
        both = [i for i in EDGE_LANES["done_high"] if i in EDGE_LANES["neg4"] and restarted[i]]
        assert both, restarted.nonzero()
        assert bool((edit[4, both] < 0).all()) and bool((A.x[[3, 4, 12]][:, both] > 0).all())
        assert restarted[list(EDGE_LANES["neg12"])].all()       # BG < 0: done in the first step after the edit
    else:
        assert not restarted.any()
        for kind, word in HELD.items():
            L = list(EDGE_LANES[kind])
            assert torch.equal(support.bits(A.x[word, L]), support.bits(edit[word, L])), kind


@pytest.mark.parametrize("collect", [False, True], ids=["rollout_mlp", "collect_mlp_restart"])
def test_mlp_paths_are_the_loop_of_entry_points_through_the_branch_points(collect):
    _mlp_case(collect, False)


# ------------------------------------------------------------------------------------------------ (e) exact mode
@pytest.mark.parametrize("sensor", ["Dexcom", "Navigator"])
def test_exact_step_follows_the_oracles_dopri5_through_the_branch_points(sensor):
    torch = _torch()
    inp = support.status_inputs(sensor)
    e = support.status_env(sensor, exact=True)
    d = _Step(e, inp)
    rows = {k: [] for k in ("bg", "cgm", "done", "x")}
    for k in range(K):
        if k == STATUS_PRE:
            support.edge_states(e.x, inp["pid"])
            edit = e.x.clone()
        d.run(1)
        for key in rows:
            rows[key].append(getattr(e, key).clone())
    assert e.sync() == 0                                        # no T1D_ST_SOLVER_FAILED, nothing non-finite
    got = {k: torch.stack(v).double().cpu().numpy() for k, v in rows.items()}
    ref = support.edge_oracle(sensor, "dopri")
    worst = np.maximum(np.abs(got["bg"] - ref["bg"]).max(0), np.abs(got["cgm"] - ref["cgm"]).max(0))
    near = worst <= 1e-8
    wx = float((np.abs(got["x"] - ref["x"]) / np.maximum(1.0, np.abs(ref["x"]))).max())
    print("\n[edge states] (e) exact %s: %d of %d envs within 1e-8 of the oracle, max %.3e, x(rel) %.2e, done flips %d"
          % (sensor, near.sum(), len(near), worst.max(), wx, (got["done"] != ref["done"]).sum()))
    assert np.array_equal(got["done"], ref["done"]) and got["done"][STATUS_PRE:].any()
    assert near.mean() >= 0.95 and worst.max() <= 5e-4, (near.mean(), worst.max())
    for kind, word in HELD.items():
        L = list(EDGE_LANES[kind])
        for k in range(STATUS_PRE, K):
            assert torch.equal(support.bits(rows["x"][k][word, L]), support.bits(edit[word, L])), (kind, k)
    L = support.edge_lanes(*EDGE_CROSSING)
    x3 = got["x"][:, 3, L]
    print("[edge states] (e) exact %s: x3 of the crossing lanes at the end %s" % (sensor, x3[-1]))
    assert ((x3[-1] > -1e-9) & (x3[-1] < 0)).all()
    for k in range(STATUS_PRE, K - 1):                          # once below 0 it does not move
        below = x3[k] < 0
        assert np.array_equal(x3[k + 1][below], x3[k][below]), k


def test_exact_pid_rollout_is_its_step_loop_through_the_branch_points():
    """rollout_pid_dopri5 in calls of STATUS_PRE, 1 and STATUS_POST - 1 steps against test_gpu_dopri5_rollout's loop of step()
    with the controller in torch, bit for bit"""
    torch = _torch()
    inp = support.status_inputs("Dexcom")
    a, b = (support.status_env("Dexcom", exact=True) for _ in range(2))
    d = _Rollout(b, inp, exact=True)
    state, rows = None, []
    for steps in (STATUS_PRE, STATUS_POST):
        if steps == STATUS_POST:
            support.edge_states(a.x, inp["pid"]); support.edge_states(b.x, inp["pid"])
            edit = b.x.clone()
        state, r, _ = _exact_step_loop(a, "pid", steps, PID[:3], PID[3], state)
        rows.append(r)
        for k in (steps,) if steps == STATUS_PRE else d.calls:
            d.run(k)
    assert a.sync() == 0 and b.sync() == 0
    support.same_env(a, b, EXACT_LOOP_STATE + ("done",), by="value")
    for k in ("integ", "prev"):
        assert torch.equal(state[k], d.state[k]), k
    for k in ("bg", "cgm", "cho", "insulin"):
        assert torch.equal(torch.cat([r[k] for r in rows]), d.trace[k][1:]), k
    print("\n[edge states] (e) rollout_pid_dopri5: bit for bit; done at the end in %d envs" % int(b.done.sum()))
    assert bool(b.done.any())
    for kind, word in HELD.items():
        L = list(EDGE_LANES[kind])
        assert torch.equal(support.bits(b.x[word, L]), support.bits(edit[word, L])), kind
    x3 = b.x[3, support.edge_lanes(*EDGE_CROSSING)]
    assert bool(((x3 > -1e-9) & (x3 < 0)).all())


@pytest.mark.parametrize("collect", [False, True], ids=["rollout_mlp_dopri5", "collect_mlp_dopri5_restart"])
def test_exact_mlp_paths_are_the_loop_of_entry_points_through_the_branch_points(collect):
    _mlp_case(collect, True)
