"""Gastric-emptying edge states through every stepping kernel, and the model's right-hand side over the gut domain.

test_gpu_edge_states.py takes every kernel family through the branch points of the glucose sub-system; here the gut
sub-system (x0, x1, x2, last_qsto, last_food, the dbar row) gets the same treatment.  It is where the kernels depart
furthest from the reference's arithmetic: rhs<1>, kgut_flux and the exact mode each restate the tanh pair of
t1dpatient.py:135-142 with their own guards and exponentials, and a wrong guard constant, a lost has_dbar select or an fp32
overflow of (Ea + 1)(Ec + 1) only shows where the arguments are large -- which no 70 g meal on an empty stomach reaches.

Inputs: support.gut_inputs -- the status inputs (150 envs, two full 64-env chunks and a partial one, all 30 patients) with
further meals after the edit -- stepped STATUS_PRE times; then support.gut_states edits x0, x1, last_qsto, last_food and the
dbar row (the same function edits the oracle's words); then STATUS_POST more steps.  Every kind (support.GUT_LANES) sits in
lanes of all three chunks.  test_gut_states_host.py shows on the CPU that the oracle reaches the arguments the kinds claim,
that the steep lanes are at level 2 in their minute, that no BG ends a step within 1e-6 mg/dL of a `done` threshold (no env
is ever `done`: the closest BG is 63 mg/dL away), and that the all-fed batch of the overflow case leaves more lanes at
level 2 than the workgroup has records.  The MLP paths take support.gym_env(256), edited by the same function.

The drivers, the table of step paths, the pairs and the roll-out forms are test_gpu_edge_states.py's, and so are the bounds:
TOL_ORACLE on BG, CGM and last_cgm and, relative to max(1, |x|), on the 13 states; 1e-6 on reward and risk; `done`
identical; TOL_F32 for fp32 against fp64; TOL_KERNELS and TOL_KERNELS_X kernel against kernel; the roll-outs against their
loops at 1e-9 (the PID's integral 1e-6, prev_meal 1e-12; fp32: TOL_KERNELS_F32, TOL_KERNELS_X_F32, the integral K st times
the former); the exact mode as test_gpu_dopri5.py holds a heterogeneous batch (95 % of the envs within 1e-8, none beyond
5e-4).  Added here: planned, last_qsto and last_food against the oracle's after every step and dbar against
last_qsto + 1000 last_food, each to 1e-12 relative to max(1, |value|).  No lane is left out of any comparison.  Every case
prints its worst values; profiles/edge_states/README.md has them as measured on an MI355X.

t1d_model_rhs, which fixture G1 checks on ordinary points in fp64 only, is taken over the gut domain in both math modes and
both precisions against a 40-digit restatement of the model (RHS_*, below)."""
import functools

import numpy as np
import pytest

import support
from support import EDGE_OUT, GUT_LANES, GUT_WORDS, STATUS_POST, STATUS_PRE, gpu_torch as _torch
from test_gpu_dopri5_rollout import STATE as EXACT_LOOP_STATE, _step_loop as _exact_step_loop
from test_gpu_edge_states import ALL_FED, K, PAIRS, PATHS, _device_run, _mlp_pair, _scheme, _show, _worst
from test_gpu_parity import TOL_ORACLE
from test_gpu_sensor_grid import (LOOP_KEYS, OVERFLOW_CAP, PID, TOL_KERNELS, TOL_KERNELS_F32, TOL_KERNELS_X, TOL_KERNELS_X_F32,
                                  _once, _step_by_step)
from test_gpu_status import ROLLOUT_FORMS, _Rollout, _Step, _dtype
from test_gpu_step_trim import TOL_F32

pytestmark = pytest.mark.gpu

KEYS = EDGE_OUT + GUT_WORDS + ("dbar",)
TOL_WORDS = 1e-12                               # the meal words and the dbar row, relative to max(1, |value|)


@pytest.fixture(scope="module")
def shared():
    """device runs that several cases compare with, each made by the first case that asks and kept on the host"""
    return {}


def _write(e, pid=None):
    return support.gut_states(e, e.patient_idx if pid is None else pid)


def _run(shared, path, dtype="float64"):
    return _once(shared, (path, dtype), lambda: _device_run(path, dtype, support.gut_inputs, _write, KEYS))


def _oracle(path):
    sensor, feed, meal_step, _, _ = PATHS.get(path) or ALL_FED
    return support.gut_oracle(sensor, _scheme(path), feed, meal_step)


def _rel(a, b):
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def _words(got, ref):
    """the meal bookkeeping against `ref`'s and the dbar row against the two words beside it"""
    w = {k: _rel(got[k], ref[k]) for k in GUT_WORDS}
    w["dbar"] = _rel(got["dbar"], got["last_qsto"] + 1000.0 * got["last_food"])
    return w


# ------------------------------------------------------------------------------------------------ (a) against the oracle
@pytest.mark.parametrize("path", list(PATHS))
def test_step_kernels_follow_the_oracle_through_the_gut_states(shared, path):
    """every entry of test_gpu_edge_states.PATHS, fp64, each against the oracle's restatement of its scheme, after every
    step; the meal words and the dbar row after every step as well"""
    got, ref = _run(shared, path), _oracle(path)
    w = _worst(got, ref, got["st"])
    w["x_gut"] = _rel(got["x"][:, :3], ref["x"][:, :3])          # (x is led by the glucose states: the gut's own three)
    w.update(_words(got, ref))
    _show("gut (a) oracle", path, w)
    assert all(np.isfinite(got[k]).all() for k in KEYS)
    assert w["cgm"] < TOL_ORACLE and w["bg"] < TOL_ORACLE and w["last_cgm"] < TOL_ORACLE, w
    assert w["x"] < TOL_ORACLE, w
    assert w["reward"] < 1e-6 and w["risk"] < 1e-6, w
    assert w["done"] == 0
    assert all(w[k] < TOL_WORDS for k in GUT_WORDS + ("dbar",)), w
    R = list(GUT_LANES["residue"])                               # what was written is what the env held: a denormal stays one
    assert (got["raw_edit"][0, R] == 1e-300).all() and (got["raw_edit"][1, R] == 5e-324).all()
    if path == "multi_minute_overflow":
        assert ref["level2"][STATUS_PRE] - OVERFLOW_CAP >= 64    # (test_gut_states_host.py: in its first minute alone)


# ------------------------------------------------------------------------------------------------ (b) fp32 against fp64
@pytest.mark.parametrize("path", list(PATHS))
def test_fp32_step_kernels_track_fp64_through_the_gut_states(shared, path):
    """in fp32 the residue lanes' x0 = 1e-300 and x1 = 5e-324 are written as 0 (asserted), every other word as its nearest
    float"""
    got, ref = _run(shared, path, "float32"), _run(shared, path)
    w = {k: float(np.abs(got[k] - ref[k]).max()) for k in ("bg", "cgm")}
    w["done"] = int((got["done"] != ref["done"]).sum())
    w.update(planned=_rel(got["planned"], ref["planned"]), dbar=_rel(got["dbar"], got["last_qsto"] + 1000.0 * got["last_food"]))
    _show("gut (b) fp32", path, w)
    assert got["raw_x"].dtype == np.float32 and all(np.isfinite(got[k]).all() for k in KEYS)
    assert (got["raw_edit"][:2, list(GUT_LANES["residue"])] == 0).all()
    assert w["bg"] < TOL_F32 and w["cgm"] < TOL_F32, w
    assert w["done"] == 0
    # the bookkeeping in fp32: the plan to a few ulp (sums of multiples of 5 g and of the meals), dbar to an ulp of fp32
    assert w["planned"] < 1e-6 and w["dbar"] < 2.0 ** -23, w


# ------------------------------------------------------------------------------------------------ (c) kernel against kernel
@pytest.mark.parametrize("a,b", PAIRS)
def test_step_kernels_agree_through_the_gut_states(shared, a, b):
    ra, rb = _run(shared, a), _run(shared, b)
    w = _worst(ra, rb, ra["st"])
    w["x_abs"] = float(np.abs(ra["x"] - rb["x"]).max())
    w.update(_words(ra, rb))
    _show("gut (c) kernels", "%s / %s" % (a, b), w)
    for k in ("cgm", "bg", "reward", "risk", "last_cgm"):
        assert w[k] < TOL_KERNELS, (k, w)
    assert w["x_abs"] < TOL_KERNELS_X and w["done"] == 0, w
    assert all(w[k] < TOL_WORDS for k in GUT_WORDS + ("dbar",)), w


# ------------------------------------------------------------------------------------------------ (d) closed loops
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("form", list(ROLLOUT_FORMS))
@pytest.mark.parametrize("ctrl", ["pid", "bb"])
def test_rollouts_match_their_step_loops_through_the_gut_states(shared, ctrl, form, dtype):
    """rollout_pid / rollout_bb in calls of STATUS_PRE, 1 and STATUS_POST - 1 steps, all steps of a call in one launch or
    one launch of the multi-minute kernel per step, against the controller on the host around step(): the meals after the
    edit arrive inside a launch that keeps the lane in registers -- the second meal of GUT_SECOND_LATE in its middle
    minute, the two of back_to_back across its boundary with the next"""
    torch = _torch()
    inp = support.gut_inputs("Dexcom")
    st = inp["st"]
    words = GUT_WORDS[1:] + ("dbar",)                            # (planned is one of LOOP_KEYS)

    def loop():
        e = support.status_env("Dexcom", dtype=_dtype(dtype), inputs=support.gut_inputs)
        out = _step_by_step(st, ctrl, e, K, lambda k: k == STATUS_PRE and _write(e, inp["pid"]))
        out.update({k: getattr(e, k).clone().cpu() for k in ("done",) + words})
        return out
    ref = _once(shared, ("loop", ctrl, dtype), loop)
    e = support.status_env("Dexcom", options=ROLLOUT_FORMS[form], dtype=_dtype(dtype), inputs=support.gut_inputs)
    d = _Rollout(e, inp, ctrl=ctrl)
    d.run(STATUS_PRE)
    _write(e, inp["pid"])
    for k in d.calls:
        d.run(k)
    assert e.sync() == 0 and int(e.t.min()) == int(e.t.max()) == K * st
    worst = {k: float((getattr(e, k).double().cpu() - ref[k].double()).abs().max()) for k in LOOP_KEYS}
    ctl = {k: float((d.state[k].double().cpu() - ref[k].double()).abs().max()) for k in (("integ", "prev") if ctrl == "pid" else ("prev_meal",))}
    worst.update(ctl)
    worst["done"] = int((e.done.cpu() != ref["done"]).sum())
    ww = {k: _rel(getattr(e, k).double().cpu().numpy(), ref[k].double().numpy()) for k in words}
    ww["dbar_row"] = _rel(e.dbar.double().cpu().numpy(), (e.last_qsto.double() + 1000.0 * e.last_food.double()).cpu().numpy())
    worst.update(ww)
    _show("gut (d) roll-outs", "rollout_%s %s %s" % (ctrl, form, dtype), worst)
    tol, tol_x = (1e-9, 1e-9) if dtype == "float64" else (TOL_KERNELS_F32, TOL_KERNELS_X_F32)
    assert worst["t"] == 0
    for k in LOOP_KEYS:
        assert worst[k] < (tol_x if k == "x" else tol), (k, worst)
    if ctrl == "pid":
        assert ctl["integ"] < (1e-6 if dtype == "float64" else K * st * TOL_KERNELS_F32) and ctl["prev"] < tol, ctl
    else:
        assert ctl["prev_meal"] < (1e-12 if dtype == "float64" else tol), ctl
    assert worst["done"] == 0
    # the meal words: last_food is the same sum of the same meals in both; last_qsto is x0 + x1 of a meal's first minute and
    # dbar holds it, so in fp32 they follow the states' bound; the row against its two words: one rounding
    tol_w = TOL_WORDS if dtype == "float64" else TOL_KERNELS_X_F32 / 30e3       # relative; the second meals take last_qsto > 30 g
    assert ww["last_food"] < TOL_WORDS and ww["last_qsto"] < tol_w and ww["dbar"] < tol_w, ww
    assert ww["dbar_row"] < (TOL_WORDS if dtype == "float64" else 2.0 ** -23), ww


# ------------------------------------------------------------------------------------------------ (e) exact mode
@pytest.mark.parametrize("sensor", ["Dexcom", "Navigator"])
def test_exact_step_follows_the_oracles_dopri5_through_the_gut_states(sensor):
    torch = _torch()
    inp = support.gut_inputs(sensor)
    e = support.status_env(sensor, exact=True, inputs=support.gut_inputs)
    d = _Step(e, inp)
    rows = {k: [] for k in ("bg", "cgm", "done", "x") + GUT_WORDS + ("dbar",)}
    for k in range(K):
        if k == STATUS_PRE:
            _write(e, inp["pid"])
        d.run(1)
        for key in rows:
            rows[key].append(getattr(e, key).clone())
    assert e.sync() == 0                                        # no T1D_ST_SOLVER_FAILED, nothing non-finite
    got = {k: torch.stack(v).double().cpu().numpy() for k, v in rows.items()}
    ref = support.gut_oracle(sensor, "dopri")
    worst = np.maximum(np.abs(got["bg"] - ref["bg"]).max(0), np.abs(got["cgm"] - ref["cgm"]).max(0))
    near = worst <= 1e-8
    wx = _rel(got["x"], ref["x"])
    ww = _words(got, ref)
    print("\n[gut states] (e) exact %s: %d of %d envs within 1e-8 of the oracle, max %.3e, x(rel) %.2e, done flips %d, words %s"
          % (sensor, near.sum(), len(near), worst.max(), wx, (got["done"] != ref["done"]).sum(), ww))
    assert all(np.isfinite(v).all() for v in got.values())
    assert np.array_equal(got["done"], ref["done"])
    assert near.mean() >= 0.95 and worst.max() <= 5e-4, (near.mean(), worst.max())
    assert all(v < TOL_WORDS for v in ww.values()), ww


def test_exact_pid_rollout_is_its_step_loop_through_the_gut_states():
    """rollout_pid_dopri5 in calls of STATUS_PRE, 1 and STATUS_POST - 1 steps against test_gpu_dopri5_rollout's loop of step()
    with the controller in torch, bit for bit"""
    torch = _torch()
    inp = support.gut_inputs("Dexcom")
    a, b = (support.status_env("Dexcom", exact=True, inputs=support.gut_inputs) for _ in range(2))
    d = _Rollout(b, inp, exact=True)
    state, rows = None, []
    for steps in (STATUS_PRE, STATUS_POST):
        if steps == STATUS_POST:
            _write(a, inp["pid"]); _write(b, inp["pid"])
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
    L = support.gut_lanes("second_meal", "tiny_meal", "huge_meal", "back_to_back", "meal_while_eating")
    eaten = d.trace["cho"][1 + STATUS_PRE:, L].sum(0)
    print("\n[gut states] (e) rollout_pid_dopri5: bit for bit; CHO per step summed over the steps after the edit, meal lanes %s" % eaten.tolist())
    assert bool((eaten > 0).all())


# ------------------------------------------------------------------------------------------------ (f) MLP paths
@pytest.mark.parametrize("collect", [False, True], ids=["rollout_mlp", "collect_mlp_restart"])
def test_mlp_paths_are_the_loop_of_entry_points_through_the_gut_states(collect):
    """rollout_mlp and collect_mlp(on_done="restart") against support.loop_of_entry_points, support.gym_env(256) edited by
    gut_states in both, bit for bit (the env's own meals; the kinds that arrive through the meal table are not in it)"""
    A, before, edit, low, high = _mlp_pair(collect, False, write=_write)
    L = support.gut_lanes(*support.GUT_EDITED)
    moved = int((A.x[:2, L] != edit[:2, L]).any(0).sum())
    print("\n[gut states] (f) %s: bit for bit; edited lanes whose x0 or x1 moved since %d of %d, endings < 70: %d, > 350: %d"
          % ("collect_mlp" if collect else "rollout_mlp", moved, len(L), low, high))
    assert bool((edit[0, list(GUT_LANES["no_dbar"])] == 3000.0).all()) and moved >= len(L) - len(GUT_LANES["deep_negative"])


# ------------------------------------------------------------------------------------------------ t1d_model_rhs over the gut domain
# Points: all 30 patients x Dbar in {0, 50 mg, 5 g, 70 g, 400 g} x qsto / Dbar on a grid from 0 to 30 that holds b and d
# exactly and one ulp to either side (Dbar = 0: a few absolute qsto) x x1 / qsto in {0, 0.3, 1}; the other ten states, CHO
# and insulin from rows of fixture G1.  Reference: t1dpatient.py:119-208 restated in mpmath at 40 digits, evaluated on the
# inputs as rounded to the call's precision, which returns beside each component S = the sum of the magnitudes of its terms:
# k[1] and k[2] cancel, so errors are taken relative to S, not to |k|.
# Bounds on |got - ref| / S.  fp64: the project's own for this entry point (test_gpu_configs.py), 1e-12 for math 0 and 1e-9
# for math 1.  fp32 has no project number: the plain float32 restatement of the model on the CPU, written as the reference
# writes it, sets the scale -- its worst error / S against mpmath on the same points is measured by the test (the reference
# alone; a trial on the kgut bracket gave 2.2e-7 relative to kmax, 3.9e-16 for float64) -- and math 0 gets 8 times that
# (ocml against libm, contraction), math 1 gets 32 times that (__expf loses about |argument| 2^-24 relative, which matters
# where |argument| <~ 10; the 1-ulp reciprocal; the 4 ulp of the bracket).  Both factors are margins, not measurements.
RHS_RATIOS = (0.0, 0.05, 0.5, 0.9, 1.0, 1.1, 2.0, 5.0, 12.0, 30.0)
RHS_DBAR = (0.0, 50.0, 5e3, 70e3, 400e3)         # mg
RHS_ABS_QSTO = (0.0, 1e-3, 40.0, 5e3, 3e5)       # mg, where Dbar = 0
RHS_SPLIT = (0.0, 0.3, 1.0)                      # x1 / qsto
RHS_TOL_F64 = {0: 1e-12, 1: 1e-9}
RHS_F32_FACTOR = {0: 8.0, 1: 32.0}
RHS_COLS = ("kabs", "kmax", "kmin", "b", "d", "BW", "f", "kp1", "kp2", "kp3", "Fsnc", "ke1", "ke2", "k1", "k2", "Vm0", "Vmx", "Km0",
            "m1", "m2", "m4", "m30", "ka1", "ka2", "kd", "Vi", "p2u", "Ib", "ki", "ksc")


@functools.lru_cache(maxsize=None)
def _rhs_points():
    """-> dict of fp64 arrays: pid [m], x [13, m], cho, insulin, last_qsto, last_food [m]"""
    from simglucose_amd import params
    g = np.load(support.os.path.join(support.GOLDEN, "g1_rhs.npz"))
    _, tab = params.patient_table()
    rows = []
    for pid in range(30):
        b, d = float(tab[pid, params.P_COL["b"]]), float(tab[pid, params.P_COL["d"]])
        for dbar in RHS_DBAR:
            if dbar == 0.0:
                qs = RHS_ABS_QSTO
            else:                                # b Dbar and d Dbar as the model forms them, and their neighbours
                at = [f * dbar for f in (b, d)]
                qs = [r * dbar for r in RHS_RATIOS] + at + [np.nextafter(q, s) for q in at for s in (0.0, np.inf)]
            for q in qs:
                for f1 in RHS_SPLIT:
                    x1 = f1 * q
                    rows.append((pid, q - x1, x1, dbar))
    m = len(rows)
    rs = np.random.RandomState(5)
    pick = rs.randint(0, len(g["x"]), m)
    x = g["x"][pick].T.copy()
    pid, x[0], x[1], dbar = (np.array(c) for c in zip(*rows))
    # Dbar through both words: last_qsto alone, last_food alone, and both (a quarter in last_qsto)
    way = np.arange(m) % 3
    lq = np.where(way == 0, dbar, np.where(way == 1, 0.0, 0.25 * dbar))
    lf = (dbar - lq) / 1000.0
    return dict(pid=pid.astype(np.int64), x=x, cho=g["cho"][pick], insulin=g["insulin"][pick], last_qsto=lq, last_food=lf)


def _rhs_model(p, x, cho, ins, lq, lf, F):
    """t1dpatient.py:119-208 on one point in the arithmetic F (F.num: a number of it; F.tanh) -> (dx/dt [13], S [13]) with
    S = the sum of the magnitudes of the terms of each component"""
    n, k, S = F.num, [None] * 13, [None] * 13

    def total(i, *terms):
        v, s = n(0), n(0)
        for t in terms:
            v = v + t; s = s + abs(t)
        k[i], S[i] = v, s
    d = cho * n(1000)                                            # :121
    insulin = ins * n(6000) / p["BW"]                            # :122
    qsto = x[0] + x[1]                                           # :126
    dbar = lq + lf * n(1000)                                     # :130
    total(0, -p["kmax"] * x[0], d)                               # :133
    if dbar > 0:                                                 # :135-140
        aa = n(5) / n(2) / (n(1) - p["b"]) / dbar
        cc = n(5) / n(2) / p["d"] / dbar
        kgut = p["kmin"] + (p["kmax"] - p["kmin"]) / n(2) * (F.tanh(aa * (qsto - p["b"] * dbar)) - F.tanh(cc * (qsto - p["d"] * dbar)) + n(2))
    else:
        kgut = p["kmax"]                                         # :142
    total(1, p["kmax"] * x[0], -x[1] * kgut)                     # :145
    total(2, kgut * x[1], -p["kabs"] * x[2])                     # :148
    rat = p["f"] * p["kabs"] * x[2] / p["BW"]                    # :151
    egp = p["kp1"] - p["kp2"] * x[3] - p["kp3"] * x[8]           # :153
    et = p["ke1"] * (x[3] - p["ke2"]) if x[3] > p["ke2"] else n(0)   # :158-161
    total(3, egp if egp > 0 else n(0), rat, -p["Fsnc"], -et, -p["k1"] * x[3], p["k2"] * x[4])       # :165
    vmt = p["Vm0"] + p["Vmx"] * x[6]                             # :169
    total(4, -(vmt * x[4] / (p["Km0"] + x[4])), p["k1"] * x[3], -p["k2"] * x[4])                    # :171-172
    total(5, -(p["m2"] + p["m4"]) * x[5], p["m1"] * x[9], p["ka1"] * x[10], p["ka2"] * x[11])       # :176
    it = x[5] / p["Vi"]                                          # :178
    total(6, -p["p2u"] * x[6], p["p2u"] * (it - p["Ib"]))        # :182
    total(7, -p["ki"] * x[7], p["ki"] * it)                      # :185
    total(8, -p["ki"] * x[8], p["ki"] * x[7])                    # :187
    total(9, -(p["m1"] + p["m30"]) * x[9], p["m2"] * x[5])       # :190
    total(10, insulin, -(p["ka1"] + p["kd"]) * x[10])            # :194
    total(11, p["kd"] * x[10], -p["ka2"] * x[11])                # :197
    total(12, -p["ksc"] * x[12], p["ksc"] * x[3])                # :201
    for i in (3, 4, 5, 9, 10, 11, 12):                           # :167, 173, 179, 191, 195, 198, 202
        if not x[i] >= 0:
            k[i] = n(0)
    return k, S


class _Mp:
    import mpmath as mp
    num = staticmethod(lambda v: _Mp.mp.mpf(v))
    tanh = staticmethod(lambda v: _Mp.mp.tanh(v))


class _Np:
    """numpy scalars of one type: every operation rounds to it"""
    def __init__(self, ft):
        self.num, self.tanh = ft, np.tanh


@functools.lru_cache(maxsize=None)
def _rhs_reference(dtype):
    """the 40-digit model on the points as rounded to `dtype` -> (ref [13, m], S [13, m]) as fp64, and the worst error / S
    of the plain restatement in that precision"""
    from simglucose_amd import params
    _Mp.mp.mp.dps = 40
    ft = {"float64": np.float64, "float32": np.float32}[dtype]
    P, _, tab = _rhs_points(), *params.patient_table()
    m = len(P["pid"])
    ref, S, plain = np.zeros((13, m)), np.zeros((13, m)), 0.0
    # the device holds the table in the call's precision: the reference takes the parameters as rounded to it
    par = [{c: ft(tab[r, params.P_COL[c]]) for c in RHS_COLS} for r in range(30)]
    par_mp = [{c: _Mp.num(float(v)) for c, v in row.items()} for row in par]
    lib = _Np(ft)
    with np.errstate(all="ignore"):
        for j in range(m):
            pid = int(P["pid"][j])
            args = [ft(P[key][j]) for key in ("cho", "insulin", "last_qsto", "last_food")]
            x = [ft(v) for v in P["x"][:, j]]
            k, s = _rhs_model(par_mp[pid], [_Mp.num(float(v)) for v in x], *[_Mp.num(float(v)) for v in args], _Mp)
            kp, _ = _rhs_model(par[pid], x, *args, lib)
            for i in range(13):
                ref[i, j], S[i, j] = float(k[i]), float(s[i])
                if s[i] > 0:
                    plain = max(plain, float(abs(_Mp.num(float(kp[i])) - k[i]) / s[i]))
    return ref, S, plain


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_rhs_over_the_gut_domain(shared, dtype):
    """t1d_model_rhs in both math modes, one launch each, against the 40-digit model, relative to S"""
    torch = _torch()
    P = _rhs_points()
    ref, S, plain = _rhs_reference(dtype)
    e = support.plain_env(patient="adult#001", n_envs=1, sensor="Navigator", dtype=_dtype(dtype))
    got, worst = {}, {}
    for math in (0, 1):
        out = e.model_rhs(P["x"], P["pid"], P["cho"], P["insulin"], P["last_qsto"], P["last_food"], math=math)
        got[math] = out.double().cpu().numpy()
        assert np.isfinite(got[math]).all(), math
        err = np.abs(got[math] - ref) / np.where(S > 0, S, 1.0)
        worst[math] = err.max(1)
    assert e.sync() == 0
    tol = dict(RHS_TOL_F64) if dtype == "float64" else {mth: RHS_F32_FACTOR[mth] * plain for mth in (0, 1)}
    between = np.abs(got[0] - got[1]) / np.where(S > 0, S, 1.0)
    print("\n[gut states] rhs %s over %d points: plain %s restatement %.2e of S; math 0 %.2e (bound %.2e), math 1 %.2e (bound %.2e), "
          "math 0 against 1 %.2e; per component, math 1: %s" % (dtype, ref.shape[1], dtype, plain, worst[0].max(), tol[0], worst[1].max(), tol[1],
                                                               between.max(), " ".join("%.1e" % v for v in worst[1])))
    for math in (0, 1):
        assert worst[math].max() < tol[math], (math, worst[math])
    assert between.max() < tol[0] + tol[1]
    assert (got[0][:, S.sum(0) == 0] == 0).all() and (got[1][:, S.sum(0) == 0] == 0).all()
