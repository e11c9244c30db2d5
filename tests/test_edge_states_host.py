"""The oracle's side of test_gpu_edge_states.py, checked without a GPU: the states that support.edge_states writes after
the STATUS_PRE steps of the status inputs really take the reference through the branches of the model -- a held x3, x4 and
x12, an x3 that falls through 0 in a stated minute, the renal threshold ke2 passed in both directions, a clamped EGPt, `done`
raised a little beyond 70 and 350 mg/dL -- in lanes of all three chunks and in minutes that the step-size rule puts at level
2, so that the device comparison cannot pass on nothing.  The patients' minutes are looked at under a one-minute sensor, as
support.status_lanes does: the patient does not depend on the sensor.

Measured (printed by the tests): Navigator's inputs put 45, 33 and 20 of the 150 envs at level 2 in the three minutes after
the edit, Dexcom's 26, 18 and 15; x3 of the crossing lanes ends at -1e-10 exactly in the fixed-step scheme and between
-1.1e-11 and -4.4e-10 under DOPRI5; no BG of any run is closer than 0.028 mg/dL to 70 or 350."""
import numpy as np
import pytest

import support
from support import EDGE_CROSSING, EDGE_HELD, EDGE_LANES, EDGE_SNAP, STATUS_N, STATUS_POST, STATUS_PRE

SENSORS = ("Navigator", "Dexcom")
HELD = {kind: word for kind, (word, _) in EDGE_HELD.items()}
# every oracle run that test_gpu_edge_states.py compares a device run with: sensor, integrator, feed, meal_step
RUNS = [(s, i, 3, 1) for s in SENSORS for i in ("split_adaptive", "dopri", "rk4", "split")] + [("Dexcom", "split_adaptive", 1, STATUS_PRE)]


def _table(name):
    from simglucose_amd import params
    _, tab = params.patient_table()
    return tab[support.status_inputs()["pid"], params.P_COL[name]]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def test_every_kind_is_in_all_three_chunks():
    assert STATUS_N == 150
    for kind, lanes in EDGE_LANES.items():
        assert len(set(lanes)) == len(lanes) >= 3 and max(lanes) < STATUS_N, kind
        assert {min(i // 64, 2) for i in lanes} == {0, 1, 2}, kind
    # a lane may carry two kinds only where they write different words (17: x4 and x12; 40, 100: x4 and x3 / x12)
    words = {"held3": {3}, "cross_m1": {3, 4, 8}, "cross_m2": {3, 4, 8}, "neg4": {4}, "neg12": {12}, "ke2_down": {3},
             "ke2_up": {3, 4}, "egp_neg": {8}, "done_high": {3, 12}, "done_low": {3, 12}}
    for a in EDGE_LANES:
        for b in EDGE_LANES:
            if a < b and words[a] & words[b]:
                assert not set(EDGE_LANES[a]) & set(EDGE_LANES[b]), (a, b)


def test_the_edit_is_the_same_through_numpy_and_torch():
    """edge_states on a torch tensor (as the device env's x is edited) writes the words it writes into the oracle's array"""
    import torch
    pid = support.status_inputs()["pid"]
    a = np.random.RandomState(1).uniform(1.0, 200.0, size=(13, STATUS_N))
    b = torch.as_tensor(a.copy())
    assert support.edge_states(a, pid) is support.edge_states(b, pid) is EDGE_LANES
    assert np.array_equal(_bits(a), _bits(b.numpy()))
    assert support.edge_lanes("held3", "neg4") == sorted(set(EDGE_LANES["held3"] + EDGE_LANES["neg4"]))


@pytest.mark.parametrize("sensor", SENSORS)
def test_the_oracle_reaches_the_branches(sensor):
    inp = support.status_inputs(sensor)
    st, t0 = inp["st"], STATUS_PRE * inp["st"]
    m = support.edge_oracle_run(sensor, minutes=True)             # minute by minute; row t0 + j: after minute j + 1 of the edit
    o = support.edge_oracle(sensor)
    assert np.isfinite(m["x"]).all() and np.isfinite(o["x"]).all() and np.isfinite(o["bg"]).all() and np.isfinite(o["cgm"]).all()
    assert np.array_equal(_bits(m["x"][st - 1::st]), _bits(o["x"]))          # the minutes are the steps' minutes
    print("\n[edge states] %s: envs at level 2 in the minutes after the edit %s, lane-minutes per step %s"
          % (sensor, m["level2"][t0:t0 + 3], o["level2"]))
    assert (m["level2"][t0:t0 + 3] > 0).all()
    x3 = lambda row, lanes: (m["x_edit"] if row < 0 else m["x"][t0 + row])[3, list(lanes)]
    # a crossing lane is at x3 >= 0 until its minute, at -1e-10 exactly after it, and stays
    for kind, minute in EDGE_CROSSING.items():
        lanes = EDGE_LANES[kind]
        for j in range(-1, minute - 1):
            assert (x3(j, lanes) > 0).all(), (kind, j)
        for j in range(minute - 1, STATUS_POST * st):
            assert (x3(j, lanes) == EDGE_SNAP).all(), (kind, j)
    # the renal threshold in both directions, in the first minute
    ke2 = _table("ke2")
    dn, up = list(EDGE_LANES["ke2_down"]), list(EDGE_LANES["ke2_up"])
    assert (m["x_edit"][3, dn] > ke2[dn]).all() and (m["x"][t0, 3, dn] < ke2[dn]).all()
    assert (m["x_edit"][3, up] < ke2[up]).all() and (m["x"][t0, 3, up] > ke2[up]).all()
    # EGPt (t1d_oracle.c:53) below 0 where x8 = 500 was written
    for kind in ("egp_neg", "cross_m1", "cross_m2"):
        L = list(EDGE_LANES[kind])
        egp = _table("kp1")[L] - _table("kp2")[L] * m["x_edit"][3, L] - _table("kp3")[L] * m["x_edit"][8, L]
        assert (egp < 0).all(), (kind, egp)
    # what the reference holds, it holds to the bit
    for kind, word in HELD.items():
        L = list(EDGE_LANES[kind])
        assert (m["x_edit"][word, L] < 0).all()
        assert np.array_equal(_bits(o["x"][STATUS_PRE:, word, L]), _bits(np.broadcast_to(m["x_edit"][word, L], (STATUS_POST, len(L))))), kind
    # done: raised by a lane of each done kind after the edit, and by the lanes whose x12 < 0
    done = o["done"][STATUS_PRE:]
    for kind in ("done_high", "done_low"):
        L = list(EDGE_LANES[kind])
        print("[edge states] %s %s: BG after the edit %s" % (sensor, kind, o["bg"][STATUS_PRE:, L].round(3).tolist()))
        assert done[:, L].any(), kind
    assert (o["bg"][STATUS_PRE:, list(EDGE_LANES["done_high"])] > 300).all() and (o["bg"][STATUS_PRE:, list(EDGE_LANES["done_low"])] < 80).all()
    assert done[:, list(EDGE_LANES["neg12"])].all() and not o["done"][:STATUS_PRE].any()


@pytest.mark.parametrize("sensor", SENSORS)
def test_a_crossing_lane_and_a_threshold_lane_are_at_level_2_in_their_minute(sensor):
    """one single-env oracle per lane, as support.status_lanes finds its level-2 lane: the level count of the minute in
    which the lane crosses"""
    inp = support.status_inputs(sensor)
    st, t0 = inp["st"], STATUS_PRE * inp["st"]
    from oracle import t1d_oracle as O

    def level2_in(lane, minute):
        orc = O.OracleEnv(inp["pid"][lane:lane + 1], sensor="Navigator", normals=inp["z"][:, lane:lane + 1], integrator="split_adaptive", n_sub=4)
        orc.reset()
        for k in range(t0 + minute):
            if k == t0:
                X = np.zeros((13, STATUS_N))
                X[:, lane] = orc.x[:, 0]
                support.edge_states(X, inp["pid"])
                orc.x[:, 0] = X[:, lane]
            before = int(orc.level_count[2])
            orc.step(support.grid_action(inp, k // st)[lane:lane + 1], None, inp["cho"][k:k + 1, lane:lane + 1])
        return int(orc.level_count[2]) > before
    crossing = {i: level2_in(i, EDGE_CROSSING[kind]) for kind in EDGE_CROSSING for i in EDGE_LANES[kind]}
    ke2 = {i: level2_in(i, 1) for kind in ("ke2_down", "ke2_up") for i in EDGE_LANES[kind]}
    print("\n[edge states] %s: at level 2 in the crossing minute: x3 = 0 %s, ke2 %s" % (sensor, crossing, ke2))
    assert any(crossing.values()) and any(ke2.values())


@pytest.mark.parametrize("sensor,integrator,feed,meal_step", RUNS)
def test_no_bg_ends_a_step_at_a_done_threshold(sensor, integrator, feed, meal_step):
    """`done` is BG < 70 or BG > 350 (t1d_oracle.c:619): a device that is TOL_ORACLE away may differ in `done` only where BG is
    that close to a threshold.  No run has such a step, so a `done` flip on the device is never legitimate."""
    bg = support.edge_oracle(sensor, integrator, feed, meal_step)["bg"]
    margin = min(np.abs(bg - 70.0).min(), np.abs(bg - 350.0).min())
    print("\n[edge states] %s %s feed %d: closest BG to 70 / 350: %.4f mg/dL" % (sensor, integrator, feed, margin))
    assert margin > 1e-6


@pytest.mark.parametrize("sensor", SENSORS)
def test_the_exact_oracle_completes_and_holds(sensor):
    """DOPRI5 on the same inputs: no solver gives up (edge_oracle raises if one does), held words stay to the bit, and an x3
    that crossed 0 sits within 1e-9 below it and does not move again"""
    o = support.edge_oracle(sensor, "dopri")
    assert np.isfinite(o["x"]).all() and np.isfinite(o["bg"]).all()
    for kind, word in HELD.items():
        L = list(EDGE_LANES[kind])
        assert np.array_equal(_bits(o["x"][STATUS_PRE:, word, L]), _bits(np.broadcast_to(o["x_edit"][word, L], (STATUS_POST, len(L))))), kind
    L = support.edge_lanes(*EDGE_CROSSING)
    x3 = o["x"][:, 3, L]
    print("\n[edge states] %s dopri: x3 of the crossing lanes at the end %s" % (sensor, x3[-1]))
    assert ((x3[-1] > -1e-9) & (x3[-1] < 0)).all()
    for k in range(STATUS_PRE, STATUS_PRE + STATUS_POST - 1):   # once below 0 it is held
        below = x3[k] < 0
        assert np.array_equal(_bits(x3[k + 1][below]), _bits(x3[k][below]))
    assert (x3[STATUS_PRE + 1] < 0).all()                        # both kinds have crossed after two steps, whatever the sensor


@pytest.mark.parametrize("sensor", SENSORS)
def test_the_exact_oracle_moves_under_one_ulp_within_the_batch_rule(sensor):
    """How far the exact-mode reference is from itself on these inputs (as test_sensor_grid_host.py measures it on the
    grid's): every word of the edited state moved by one ulp up or down.  The device is held to the rule of
    test_gpu_dopri5.py's heterogeneous batch -- 95 % of the envs within 1e-8 mg/dL, none beyond 5e-4 -- and the oracle
    alone stays inside it."""
    base = support.edge_oracle(sensor, "dopri")
    rs = np.random.RandomState(2)
    worst = np.zeros(STATUS_N)
    for _ in range(2):
        def nudge(x):
            x *= 1.0 + 2.3e-16 * rs.choice([-1.0, 1.0], size=x.shape)
        o = support.edge_oracle_run(sensor, "dopri", after_edit=nudge)
        worst = np.maximum(worst, np.maximum(np.abs(o["bg"] - base["bg"]).max(0), np.abs(o["cgm"] - base["cgm"]).max(0)))
        assert np.array_equal(o["done"], base["done"])
    print("\n[edge states] %s dopri under one ulp: %d of %d envs beyond 1e-8, max %.2e mg/dL" % (sensor, (worst > 1e-8).sum(), STATUS_N, worst.max()))
    assert (worst <= 1e-8).mean() >= 0.95 and worst.max() <= 5e-4


@pytest.mark.parametrize("sensor", SENSORS)
def test_a_lost_held_word_is_far_beyond_the_tolerance(sensor):
    """what the comparison with the oracle can see: a reference whose held x3, x4 or x12 is raised to 0 (a lane's state
    "tidied" on its way through a record or a register) leaves the stated one by far more than TOL_ORACLE = 1e-8 in the
    states of those lanes after the first step -- besides the word itself, which the device test holds to the bit"""
    base = support.edge_oracle(sensor)

    def lose(x):
        for kind, word in HELD.items():
            x[word, list(EDGE_LANES[kind])] = 0.0
    o = support.edge_oracle_run(sensor, after_edit=lose)
    rel = np.abs(o["x"] - base["x"]) / np.maximum(1.0, np.abs(base["x"]))
    moved = {kind: float(rel[STATUS_PRE][:, list(EDGE_LANES[kind])].max(0).min()) for kind in HELD}
    print("\n[edge states] %s: held word lost, smallest relative move of a lane's state after one step %s" % (sensor, moved))
    assert min(moved.values()) > 1e-5
    others = np.setdiff1d(np.arange(STATUS_N), support.edge_lanes(*HELD))
    assert np.array_equal(_bits(o["x"][:, :, others]), _bits(base["x"][:, :, others]))


def test_the_all_fed_batch_overflows_the_records():
    """the inputs of STEP_PATHS["multi_minute_overflow"]: every env fed in the first minute after the edit.  In that minute
    every lane whose x3 is not held is at level 2 -- more than the OVERFLOW_CAP = 64 records of the one workgroup."""
    n, meal_step = STATUS_N, STATUS_PRE
    inp = support.status_inputs("Dexcom", n, 1, meal_step)
    t0 = STATUS_PRE * inp["st"]
    m = support.edge_oracle_run("Dexcom", "split_adaptive", 1, meal_step, minutes=True)
    held = int((m["x_edit"][3] < 0).sum())
    print("\n[edge states] all fed: envs at level 2 per minute %s, held at the edit %d" % (m["level2"], held))
    assert held == len(EDGE_LANES["held3"])
    assert n - held <= m["level2"][t0] <= n and m["level2"][t0] - 64 >= 64      # more than a wave's worth goes through the redo map
    assert m["level2"][:t0].sum() == 0


@pytest.mark.parametrize("sensor", SENSORS)
def test_a_lone_x12_does_not_raise_done(sensor):
    """why done_high and done_low write x3 as well: with x12 = 351 Vg (69.5 Vg) alone, BG has left the threshold by the end of
    the first minute and `done` is never raised"""
    vg = _table("Vg")
    hi, lo = list(EDGE_LANES["done_high"]), list(EDGE_LANES["done_low"])

    def lone(x):
        x[3, hi + lo] = x3_before[hi + lo]
        x[12, hi] = 351.0 * vg[hi]; x[12, lo] = 69.5 * vg[lo]
    # x3 as it was before the edit: the state after STATUS_PRE steps of the poison-free status oracle run
    inp = support.status_inputs(sensor)
    orc = support.status_oracle_env(inp, "split_adaptive")
    orc.reset()
    for k in range(STATUS_PRE):
        orc.step(support.grid_action(inp, k), None, inp["cho"][k * inp["st"]:(k + 1) * inp["st"]])
    x3_before = orc.x[3].copy()
    o = support.edge_oracle_run(sensor, after_edit=lone)
    print("\n[edge states] %s lone x12: BG after the edit, high %s low %s" % (sensor, o["bg"][STATUS_PRE:, hi].round(2).tolist(),
                                                                         o["bg"][STATUS_PRE:, lo].round(2).tolist()))
    assert not o["done"][STATUS_PRE:, hi + lo].any()
