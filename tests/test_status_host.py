"""Non-finite data on the host side: the pump's clamps on NaN and +-Inf, a NaN action through the oracle, and the poisoned
oracle runs whose sets test_gpu_status.py holds the device to.  No GPU.

The reference clamps with Python's min(v, hi) and max(v, lo) (actuator/pump.py:28-29, 37-38): both hand their first operand
on unless the second compares beyond it, so a NaN amount stays NaN, +Inf becomes max and -Inf min.  InsulinPump is the
project's restatement of that expression; the oracle's pump and the kernels' pump_quantise must agree with it word for word,
NaN included."""
import numpy as np
import pytest

import support
from oracle import t1d_oracle as O

NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("name", ["Insulet", "Cozmo"])
def test_oracle_pump_is_the_host_pump_on_non_finite_amounts_and_ties(golden, name):
    from simglucose_amd.actuator.pump import InsulinPump
    host = InsulinPump.withName(name)
    pr = O.pump_row(name)
    amounts = np.concatenate([[NAN, INF, -INF], golden("g3_pump.npz")["amount"]])
    with np.errstate(invalid="ignore"):
        ref_basal = np.array([host.basal(a) for a in amounts], dtype=np.float64)
        ref_bolus = np.array([host.bolus(a) for a in amounts], dtype=np.float64)
    got_basal = np.array([O.pump(a, pr[5], pr[3], pr[4]) for a in amounts])
    got_bolus = np.array([O.pump(a, pr[2], pr[0], pr[1]) for a in amounts])
    # the reference's answers on the three non-finite amounts, stated: NaN, max, min
    assert np.isnan(ref_basal[0]) and ref_basal[1] == pr[4] and ref_basal[2] == pr[3]
    assert np.isnan(ref_bolus[0]) and ref_bolus[1] == pr[1] and ref_bolus[2] == pr[0]
    assert np.array_equal(got_basal, ref_basal, equal_nan=True), (got_basal[:3], ref_basal[:3])
    assert np.array_equal(got_bolus, ref_bolus, equal_nan=True), (got_bolus[:3], ref_bolus[:3])


@pytest.mark.parametrize("arm", ["basal", "bolus"])
@pytest.mark.parametrize("sensor", ["Navigator", "Dexcom"])
def test_nan_action_through_the_oracle_poisons_that_env_alone(sensor, arm):
    """one step with a NaN basal (bolus) in three envs: those end the step with a non-finite x[12], BG and recorded insulin;
    every other env equals the clean run bit for bit"""
    inp = support.status_inputs(sensor)
    lanes = list(support.status_lanes(sensor))
    clean, dirty = (support.status_oracle_env(inp, "split_adaptive") for _ in range(2))
    clean.reset(); dirty.reset()
    basal = support.grid_action(inp, 0)
    bolus = np.zeros(inp["n"])
    bad_basal, bad_bolus = basal.copy(), bolus.copy()
    (bad_basal if arm == "basal" else bad_bolus)[lanes] = NAN
    rc = clean.step(basal, bolus, inp["cho"][:inp["st"]])
    rd = dirty.step(bad_basal, bad_bolus, inp["cho"][:inp["st"]])
    others = np.setdiff1d(np.arange(inp["n"]), lanes)
    assert np.isnan(dirty.x[12, lanes]).all() and np.isnan(rd["bg"][lanes]).all() and np.isnan(rd["insulin"][lanes]).all()
    assert np.isfinite(dirty.x[:, others]).all()
    assert np.array_equal(dirty.x[:, others].view(np.int64), clean.x[:, others].view(np.int64))
    for k in ("cgm", "bg", "reward", "risk", "insulin", "done"):
        assert np.array_equal(rd[k][others], rc[k][others]), k
    # the sample taken at the end of the step reads the sensor's lower end (`cgm` is the mean over the step's minutes)
    assert (rd["done"][lanes] == 0).all() and (dirty.last_cgm[lanes] == inp["vmin"]).all()


@pytest.mark.parametrize("sign,row", [(1.0, 4), (-1.0, 3)], ids=["plus_inf_is_max_basal", "minus_inf_is_min_basal"])
def test_infinite_action_through_the_oracle_is_the_pumps_limit(sign, row):
    inp = support.status_inputs("Dexcom")
    lanes = list(support.status_lanes("Dexcom"))
    a, b = (support.status_oracle_env(inp, "split_adaptive") for _ in range(2))
    a.reset(); b.reset()
    ua, ub = support.grid_action(inp, 0).copy(), support.grid_action(inp, 0).copy()
    ua[lanes] = sign * INF
    ub[lanes] = O.pump_row("Insulet")[row]
    ra, rb = a.step(ua, None, inp["cho"][:inp["st"]]), b.step(ub, None, inp["cho"][:inp["st"]])
    assert np.array_equal(a.x.view(np.int64), b.x.view(np.int64)) and np.isfinite(a.x).all()
    assert np.array_equal(ra["insulin"], rb["insulin"]) and np.array_equal(ra["bg"], rb["bg"])


@pytest.mark.parametrize("exact", [False, True], ids=["split_adaptive", "dopri"])
@pytest.mark.parametrize("sensor", ["Navigator", "Dexcom"])
def test_poisoned_oracle_runs_end_and_stay_inside_their_lanes(sensor, exact):
    """The oracle runs test_gpu_status.py compares with: they finish, nothing outside the three lanes is touched, and what
    they say about the lanes is what the schemes' definitions say.  Fixed-step scheme: whichever word is poisoned, x[12] is
    non-finite after the first step and stays so; done stays 0 and the sensor reads its lower end.  DOPRI5: the solver gives
    up on such an env at once and the env keeps its last accepted state, so a poisoned x[0] or x[5] never reaches x[12],
    and x[12] = +Inf stays +Inf: BG above 350, done, the sensor's upper end."""
    inp = support.status_inputs(sensor)
    clean = support.status_oracle(sensor, exact)
    assert not clean["x12_bad"].any() and not clean["gave_up"].any() and np.isfinite(clean["x"]).all()
    lanes = list(clean["lanes"])
    assert lanes[0] < 64 and 64 <= lanes[2] < 128 <= lanes[1] and len(set(lanes)) == 3
    others = np.setdiff1d(np.arange(inp["n"]), lanes)
    for poison in support.POISONS:
        o = support.status_oracle(sensor, exact, poison)
        assert o["lanes"] == clean["lanes"]
        assert not o["x12_bad"][:, others].any() and not o["bg_bad"][:, others].any()
        assert np.array_equal(o["x"][:, others].view(np.int64), clean["x"][:, others].view(np.int64)), poison
        assert np.array_equal(o["bg"][:, others], clean["bg"][:, others]), poison
        assert np.array_equal(o["x12_bad"], o["bg_bad"]), poison
        reaches = poison.startswith("x12") or not exact
        assert (o["x12_bad"][:, lanes] == reaches).all(), poison
        assert (o["gave_up"] == exact).all(), poison
        if exact and poison == "x12_inf":
            assert (o["done"][:, lanes] == 1).all() and (o["last_cgm"][:, lanes] == inp["vmax"]).all()
        elif reaches:
            assert (o["done"][:, lanes] == 0).all() and (o["last_cgm"][:, lanes] == inp["vmin"]).all(), poison


def test_poisoned_lanes_of_the_all_fed_batch():
    """the inputs of the multi-minute kernel's overflow case: every env fed at the first minute of the first step after the
    poison, so that step has more lanes of level 2 (all 150) than the workgroup has records (64)"""
    n, meal_step = support.STATUS_N, support.STATUS_PRE
    lanes = support.status_lanes("Dexcom", n, 1, meal_step)
    o = support.status_oracle("Dexcom", False, "x5_nan", n, 1, meal_step)
    assert o["lanes"] == lanes and (o["x12_bad"].sum(1) == 3).all()
    # envs with a minute of level 2, per step: one single-env oracle per patient (every env is fed, so the patient decides)
    inp = support.status_inputs("Dexcom", n, 1, meal_step)
    st = inp["st"]
    per_patient = np.zeros((30, inp["K"]), dtype=bool)
    for i in range(30):
        orc = support.status_oracle_env(inp, "split_adaptive", slice(i, i + 1))
        orc.reset()
        for k in range(inp["K"]):
            before = int(orc.level_count[2])
            orc.step(support.grid_action(inp, k)[i:i + 1], None, inp["cho"][k * st:(k + 1) * st, i:i + 1])
            per_patient[i, k] = int(orc.level_count[2]) > before
    count = per_patient[inp["pid"]].sum(0)
    print("envs with a minute of level 2, per step:", count)
    assert count[support.STATUS_PRE] - 64 >= 64 and per_patient[inp["pid"][lanes[2]], support.STATUS_PRE]      # more than a wave's worth is left over
