"""The oracle's side of test_gpu_gut_states.py, checked without a GPU: the gut words that support.gut_states writes after
the STATUS_PRE steps of support.gut_inputs, and the meals that arrive after them, really take the reference where they claim
-- exponent arguments of the gastric-emptying term (t1dpatient.py:135-142) beyond the kernels' guards at 40 and 350 and below
-80, Dbar = 0 with grams in the stomach, both transitions met exactly, slopes of order 1 per mg, a meal on a stomach in
transit, a meal of 50 mg and one of 400 g -- in lanes of all three chunks, so that the device comparison cannot pass on
nothing.  The arguments are the doubled ones, 2 aa (qsto - b Dbar) and 2 cc (qsto - d Dbar): what the kernels' exponentials
take.  The patients' minutes are looked at under a one-minute sensor, as support.status_lanes does: the patient does not
depend on the sensor.

Measured (printed by the tests): the edit puts 49, 34 and 21 of Navigator's 150 envs at level 2 in the three minutes after
it and 26, 17 and 19 of Dexcom's; the overfull lanes hold A2 from 260 to 12 388 and C2 from 800 to 1 074 in the minutes
after it; the all-fed batch has 136 of 150 envs at level 2 in its first minute; no BG of any run is closer than 63 mg/dL to
70 or 350 (no env is `done`)."""
import types

import numpy as np
import pytest

import support
from support import GUT_EDITED, GUT_LANES, STATUS_N, STATUS_POST, STATUS_PRE

SENSORS = ("Navigator", "Dexcom")
# every oracle run that test_gpu_gut_states.py compares a device run with: sensor, integrator, feed, meal_step
RUNS = [(s, i, 3, 1) for s in SENSORS for i in ("split_adaptive", "dopri", "rk4", "split")] + [("Dexcom", "split_adaptive", 1, STATUS_PRE)]
# kind -> the minute after the edit (1 = the first) in which the step-size rule has to put its lanes at level 2.  tiny_dbar
# is not among them and cannot be: the rule (o_tier_level) asks for an argument that moves by more than kMove = 4 in the
# minute, that is qsto by more than 1.6 (1 - b) Dbar >= 0.9 mg, and 25 mg in x1 empty at kgut x1 < 1.8 mg a minute only where
# kgut is near kmax, which it is not at qsto = 0.8 Dbar.  The tiny_meal lanes are the ones that hold Dbar = 50 mg at level 2.
LEVEL2_MINUTE = {"tiny_meal": 1, "at_transition_b": 1, "at_transition_d": 1}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _d_of(pid):
    from simglucose_amd import params
    return params.patient_table()[1][pid, params.P_COL["d"]]


def _target(lib, n=STATUS_N, dtype=None, dbar=True):
    """what gut_states edits: the four rows of an oracle (numpy, no dbar) or of a device env (torch)"""
    rs = np.random.RandomState(1)
    rows = dict(x=rs.uniform(1.0, 200.0, size=(13, n)), last_qsto=rs.uniform(0.0, 9.0, n), last_food=rs.uniform(0.0, 9.0, n))
    if dbar:
        rows["dbar"] = np.zeros(n)
    return types.SimpleNamespace(**{k: v if lib is np else lib.as_tensor(v).to(dtype) for k, v in rows.items()})


def test_every_kind_is_in_all_three_chunks():
    assert STATUS_N == 150
    seen = set()
    for kind, lanes in GUT_LANES.items():
        assert len(set(lanes)) == len(lanes) >= 3 and max(lanes) < STATUS_N, kind
        assert {min(i // 64, 2) for i in lanes} == {0, 1, 2}, kind
        assert not seen & set(lanes), kind                       # the kinds are disjoint
        seen |= set(lanes)
    fed = support.status_inputs()["fed"]
    eating = ("at_transition_b", "at_transition_d", "meal_while_eating")         # fed lanes: eating at the edit
    assert not fed[support.gut_lanes(*[k for k in GUT_LANES if k not in eating])].any() and fed[support.gut_lanes(*eating)].all()
    pid = support.status_inputs()["pid"]
    assert 4 in pid[list(GUT_LANES["overfull"])] and 4 in pid[list(GUT_LANES["deep_negative"])]   # the largest b, 0.988
    assert set(support.GUT_DEEP_ZERO) < set(GUT_LANES["deep_negative"]) and set(support.GUT_SECOND_LATE) < set(GUT_LANES["second_meal"])


@pytest.mark.parametrize("sensor,feed,meal_step", [("Navigator", 3, 1), ("Dexcom", 3, 1), ("Dexcom", 1, STATUS_PRE)])
def test_the_meal_table_is_the_dense_cho(sensor, feed, meal_step):
    """the table the device reads and the grams per minute the oracle takes are the same meals; per env the table ascends,
    one entry per minute; the status inputs' 70 g stay where they were"""
    from simglucose_amd import _lib
    inp, base = support.gut_inputs(sensor, STATUS_N, feed, meal_step), support.status_inputs(sensor, STATUS_N, feed, meal_step)
    st, t0 = inp["st"], STATUS_PRE * inp["st"]
    cho = np.zeros_like(inp["cho"])
    for i in range(STATUS_N):
        used = inp["mt"][:, i] != _lib.MEAL_UNUSED
        assert used[:used.sum()].all() and (np.diff(inp["mt"][used, i]) > 0).all(), i
        cho[inp["mt"][used, i], i] = inp["ma"][used, i]
    assert np.array_equal(cho, inp["cho"])
    extra = inp["cho"] - base["cho"]
    assert (extra[:t0] == 0).all() and (extra >= 0).all()
    assert sorted(np.nonzero(extra.any(0))[0].tolist()) == sorted(support.gut_meals(st))
    assert np.array_equal(inp["z"], base["z"]) and np.array_equal(inp["basal"], base["basal"])
    L = list(GUT_LANES["back_to_back"])                         # the last minute of a step and the first of the next
    assert (extra[t0 + st - 1, L] == 4.0).all() and (extra[t0 + st, L] == 3.0).all()
    if st == 3:                                                  # the middle minute of the first step after the edit
        assert (extra[t0 + 1, list(support.GUT_SECOND_LATE)] == 30.0).all()


def test_the_edit_is_the_same_through_numpy_and_torch():
    """gut_states on torch rows (as the device env's are edited) writes the words it writes into the oracle's arrays; the
    dbar row it forms from them with one rounding is the plain fp64 expression last_qsto + 1000 * last_food in every
    lane; in fp32 it is the fused form of the fp32 words, and the residue lanes' 1e-300 and 5e-324 both round to 0"""
    import torch
    pid = support.status_inputs()["pid"]
    a, b, f = _target(np, dbar=False), _target(torch, dtype=torch.float64), _target(torch, dtype=torch.float32)
    assert support.gut_states(a, pid) is support.gut_states(b, pid) is support.gut_states(f, pid) is GUT_LANES
    for k in ("x", "last_qsto", "last_food"):
        assert np.array_equal(_bits(getattr(a, k)), _bits(getattr(b, k).numpy())), k
    L = support.gut_lanes(*GUT_EDITED)
    assert np.array_equal(_bits(b.dbar.numpy()[L]), _bits((a.last_qsto + 1000.0 * a.last_food)[L]))
    assert (b.dbar.numpy()[np.setdiff1d(np.arange(STATUS_N), L)] == 0).all()      # no other lane is touched
    fused = np.array([support.fma_word(float(f.last_food[i]), 1000.0, float(f.last_qsto[i])) for i in L])
    assert np.array_equal(f.dbar.numpy()[L], fused.astype(np.float32))
    R = list(GUT_LANES["residue"])
    assert (a.x[0, R] == 1e-300).all() and (a.x[1, R] == 5e-324).all() and (f.x[:2, R] == 0).all()
    assert support.gut_lanes("no_dbar", "residue") == sorted(GUT_LANES["no_dbar"] + GUT_LANES["residue"])


@pytest.mark.parametrize("sensor", SENSORS)
def test_the_oracle_reaches_the_arguments(sensor):
    inp = support.gut_inputs(sensor)
    pid, st, t0 = inp["pid"], inp["st"], STATUS_PRE * inp["st"]
    m = support.gut_oracle(sensor, minutes=True)                  # minute by minute; row t0 + j: minute j + 1 after the edit
    o = support.gut_oracle(sensor)
    for run in (m, o, support.gut_oracle(sensor, "dopri")):
        assert all(np.isfinite(run[k]).all() for k in support.EDGE_OUT + support.GUT_WORDS)
    assert np.array_equal(_bits(m["x"][st - 1::st]), _bits(o["x"]))          # the minutes are the steps' minutes
    a2, c2, dbar, qsto = support.gut_arguments(m, pid)
    after = slice(t0, None)
    print("\n[gut states] %s: envs at level 2 in the minutes after the edit %s, lane-minutes per step %s"
          % (sensor, m["level2"][t0:t0 + 3], o["level2"]))

    L = list(GUT_LANES["overfull"])
    print("[gut states] %s overfull: A2 %.0f to %.0f, C2 %.0f to %.0f" % (sensor, a2[after, L].min(), a2[after, L].max(), c2[after, L].min(), c2[after, L].max()))
    assert (a2[after, L] > 40).all() and (c2[after, L] > 40).all()
    for chunk in range(3):                                       # beyond the fp64 guard in every chunk, both arguments at once
        C = [i for i in L if min(i // 64, 2) == chunk]
        assert ((a2[after, C] > 350) & (c2[after, C] > 350)).all(0).any(), chunk
    assert (a2[after, 32] < 350).all()                           # ... and one lane with one argument on either side of it

    L = list(GUT_LANES["deep_negative"])
    print("[gut states] %s deep_negative: A2 %.1f to %.1f" % (sensor, a2[after, L].min(), a2[after, L].max()))
    assert (a2[after, L] < -80).all() and (a2[after, [i for i in L if pid[i] == 4]] < -400).all()
    assert (qsto[after, list(support.GUT_DEEP_ZERO)] == 0).all()
    rest = [i for i in L if i not in support.GUT_DEEP_ZERO]
    assert (m["x"][after, 1, rest] > 0.2).all()                  # something for kgut to multiply, through every minute

    L = list(GUT_LANES["no_dbar"])
    assert (dbar[after, L] == 0).all() and (qsto[after, L] > 1000).all()

    L = list(GUT_LANES["at_transition_b"])                      # exactly at the transition, and gone from it a minute later
    assert (a2[t0, L] == 0).all() and (np.abs(a2[t0 + 1, L]) > 1).all() and (dbar[t0, L] == 6e3).all()
    L = list(GUT_LANES["at_transition_d"])
    assert (c2[t0, L] == 0).all() and (np.abs(c2[t0 + 1, L]) > 1).all() and (dbar[t0, L] == 6e3).all()

    L = list(GUT_LANES["tiny_dbar"])                            # slopes d(argument)/d(qsto) of 0.1 to 1.4 per mg
    assert (dbar[after, L] == 50).all() and (qsto[t0, L] == 40).all() and (c2[t0, L] / (40 - _d_of(pid[L]) * 50) > 0.1).all()

    L = list(GUT_LANES["huge_in_transit"])
    assert (dbar[after, L] == 4e5).all() and (qsto[t0, L] == 3.7e5).all()

    L = list(GUT_LANES["residue"])
    assert (dbar[after, L] == 7e4).all() and (qsto[after, L] > 0).all() and (qsto[after, L] <= 1e-300).all()

    # a meal on a stomach in transit: from its minute on, Dbar is more than 1000 x the 30 g -- last_qsto was taken
    for i in GUT_LANES["second_meal"]:
        tm = t0 + (i in support.GUT_SECOND_LATE)
        assert (dbar[t0:tm, i] == 7e4).all() and (dbar[tm:, i] > 30e3).all() and (m["last_qsto"][tm:, i] > 30e3).all(), i
        assert m["last_qsto"][tm, i] == qsto[tm, i] and m["last_food"][tm, i] == 5.0
    L = list(GUT_LANES["tiny_meal"])
    assert (dbar[after, L] == support.fma_word(0.05, 1000.0, 0.0)).all() and (m["planned"][after, L] == 0).all()
    L = list(GUT_LANES["huge_meal"])
    assert (m["planned"][t0, L] == 395.0).all() and (m["planned"][-1, L] == 400.0 - 5.0 * STATUS_POST * st).all()
    # two meals in consecutive minutes are one meal: last_qsto is taken once, last_food adds up
    L = list(GUT_LANES["back_to_back"])
    assert (dbar[t0 + st - 1, L] == 4e3).all() and (dbar[t0 + st, L] == 7e3).all() and (m["last_qsto"][after, L] == 0).all()
    assert (dbar[t0 + st + 1:, L] == 7e3).all()
    # 30 g more while the 70 g are being eaten: no new last_qsto, the plan grows
    L = list(GUT_LANES["meal_while_eating"])
    assert (m["last_qsto"][after, L] == m["last_qsto"][t0 - 1, L]).all()
    assert (m["planned"][t0 + 1, L] - m["planned"][t0, L] == 25.0).all() and (np.diff(m["last_food"][:, L], axis=0)[st:] == 5.0).all()


@pytest.mark.parametrize("sensor", SENSORS)
def test_the_steep_lanes_are_at_level_2_in_their_minute(sensor):
    """one single-env oracle per lane, as support.status_lanes finds its level-2 lane: the level count of the minute named
    in LEVEL2_MINUTE, the first after the edit (for tiny_meal: the minute of its meal)"""
    from oracle import t1d_oracle as O
    inp = support.gut_inputs(sensor)
    st, t0 = inp["st"], STATUS_PRE * inp["st"]

    def level2_in(lane, minute):
        orc = O.OracleEnv(inp["pid"][lane:lane + 1], sensor="Navigator", normals=inp["z"][:, lane:lane + 1], integrator="split_adaptive", n_sub=4)
        orc.reset()
        for k in range(t0 + minute):
            if k == t0:
                T = _target(np, dbar=False)
                for key in ("x", "last_qsto", "last_food"):
                    getattr(T, key)[..., lane] = getattr(orc, key)[..., 0]
                support.gut_states(T, inp["pid"])
                for key in ("x", "last_qsto", "last_food"):
                    getattr(orc, key)[..., 0] = getattr(T, key)[..., lane]
            before = int(orc.level_count[2])
            orc.step(support.grid_action(inp, k // st)[lane:lane + 1], None, inp["cho"][k:k + 1, lane:lane + 1])
        return int(orc.level_count[2]) > before
    at = {kind: [level2_in(i, minute) for i in GUT_LANES[kind]] for kind, minute in LEVEL2_MINUTE.items()}
    print("\n[gut states] %s: at level 2 in the named minute %s" % (sensor, at))
    assert all(all(v) for v in at.values())


@pytest.mark.parametrize("sensor,integrator,feed,meal_step", RUNS)
def test_no_bg_ends_a_step_at_a_done_threshold(sensor, integrator, feed, meal_step):
    """`done` is BG < 70 or BG > 350: a device that is TOL_ORACLE away may differ in `done` only where BG is that close to a
    threshold.  No run has such a step, so a `done` flip on the device is never legitimate."""
    o = support.gut_oracle(sensor, integrator, feed, meal_step)
    assert all(np.isfinite(o[k]).all() for k in support.EDGE_OUT + support.GUT_WORDS)
    margin = min(np.abs(o["bg"] - 70.0).min(), np.abs(o["bg"] - 350.0).min())
    print("\n[gut states] %s %s feed %d: closest BG to 70 / 350: %.4f mg/dL" % (sensor, integrator, feed, margin))
    assert margin > 1e-6


@pytest.mark.parametrize("sensor", SENSORS)
def test_the_exact_oracle_moves_under_one_ulp_within_the_batch_rule(sensor):
    """How far the exact-mode reference is from itself on these inputs: every word of the edited state moved by one ulp up
    or down.  The device is held to the rule of test_gpu_dopri5.py's heterogeneous batch -- 95 % of the envs within 1e-8
    mg/dL, none beyond 5e-4 -- and the oracle alone stays inside it."""
    base = support.gut_oracle(sensor, "dopri")
    rs = np.random.RandomState(2)
    worst = np.zeros(STATUS_N)
    for _ in range(2):
        def nudge(x):
            x *= 1.0 + 2.3e-16 * rs.choice([-1.0, 1.0], size=x.shape)
        o = support.gut_oracle_run(sensor, "dopri", after_edit=nudge)
        worst = np.maximum(worst, np.maximum(np.abs(o["bg"] - base["bg"]).max(0), np.abs(o["cgm"] - base["cgm"]).max(0)))
        assert np.array_equal(o["done"], base["done"])
    print("\n[gut states] %s dopri under one ulp: %d of %d envs beyond 1e-8, max %.2e mg/dL" % (sensor, (worst > 1e-8).sum(), STATUS_N, worst.max()))
    assert (worst <= 1e-8).mean() >= 0.95 and worst.max() <= 5e-4


def test_the_all_fed_batch_overflows_the_records():
    """the inputs of STEP_PATHS["multi_minute_overflow"]: every env fed in the first minute after the edit, which there
    starts a meal in every lane (last_qsto = the edited stomach, last_food = 5 g).  In that minute more lanes are at level 2
    than the OVERFLOW_CAP = 64 records of the one workgroup, by more than a wave."""
    inp = support.gut_inputs("Dexcom", STATUS_N, 1, STATUS_PRE)
    t0 = STATUS_PRE * inp["st"]
    m = support.gut_oracle("Dexcom", "split_adaptive", 1, STATUS_PRE, minutes=True)
    print("\n[gut states] all fed: envs at level 2 per minute %s" % (m["level2"],))
    assert m["level2"][t0] - 64 >= 64 and m["level2"][:t0].sum() == 0
    assert (m["last_food"][t0] == 5.0).all() and np.array_equal(m["last_qsto"][t0], m["x_edit"][0] + m["x_edit"][1])


@pytest.mark.parametrize("sensor", SENSORS)
def test_a_lost_gut_word_is_far_beyond_the_tolerance(sensor):
    """what the comparison with the oracle can see: a reference that has lost a lane's meal words on the way through a
    record or a register -- Dbar = 0 where it was set, or the 70 g that the no_dbar lanes never ate -- leaves the stated one
    by far more than TOL_ORACLE = 1e-8 in the gut states of that lane after the first step"""
    base = support.gut_oracle(sensor)
    kinds = ("no_dbar", "deep_negative", "at_transition_b", "at_transition_d", "tiny_dbar", "huge_in_transit")

    class Lose:
        """gut_states, then the loss"""
        def __call__(self, orc, pid):
            support.gut_states(orc, pid)
            for kind in kinds:
                L = list(GUT_LANES[kind])
                orc.last_food[L] = 70.0 if kind == "no_dbar" else 0.0
                orc.last_qsto[L] = 0.0
            return GUT_LANES
    o = support.edge_oracle_run(sensor, inputs=support.gut_inputs, edit=Lose())
    rel = np.abs(o["x"] - base["x"]) / np.maximum(1.0, np.abs(base["x"]))
    moved = {kind: float(rel[STATUS_PRE][:3][:, [i for i in GUT_LANES[kind] if i not in support.GUT_DEEP_ZERO]].max(0).min()) for kind in kinds}
    print("\n[gut states] %s: meal words lost, smallest relative move of a lane's gut states after one step %s" % (sensor, moved))
    assert min(moved.values()) > 1e-5


def test_the_rhs_points_cover_the_gut_domain():
    """the points test_gpu_gut_states.py hands to t1d_model_rhs: a few thousand, all patients, both Dbar branches, arguments
    beyond every guard, both transitions exactly and one ulp to either side"""
    from simglucose_amd import params
    from test_gpu_gut_states import RHS_DBAR, _rhs_points
    P = _rhs_points()
    _, tab = params.patient_table()
    m = len(P["pid"])
    assert 3000 <= m <= 9000 and set(P["pid"]) == set(range(30))
    b, d = tab[P["pid"], params.P_COL["b"]], tab[P["pid"], params.P_COL["d"]]
    dbar, q = P["last_qsto"] + 1000.0 * P["last_food"], P["x"][0] + P["x"][1]
    safe = np.where(dbar > 0, dbar, 1.0)
    a2, c2 = 5.0 / (1.0 - b) / safe * (q - b * safe), 5.0 / d / safe * (q - d * safe)
    live = dbar > 0
    assert ((dbar == 0) & (q > 0)).sum() >= 30 * 4 * 2 and sorted(set(np.round(dbar, 6))) == sorted(RHS_DBAR)
    assert (a2[live] > 350).any() and (c2[live] > 350).any() and (a2[live] < -80).any() and (a2[live] < -400).any()
    for arg in (a2, c2):
        assert ((arg == 0) & live).sum() >= 30 and ((np.abs(arg) < 1e-12) & (arg > 0) & live).any() and ((np.abs(arg) < 1e-12) & (arg < 0) & live).any()
