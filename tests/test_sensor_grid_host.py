"""The oracle's side of test_gpu_sensor_grid.py, checked without a GPU: its spline block operator against SciPy's own
interp1d(kind="cubic") at sample times the stock sensors do not have, and the oracle run that the device is compared with
-- finite at every sample time, and with minutes at level 2 of the step-size rule, so that the comparison covers the
refined sub-steps too."""
import numpy as np
import pytest

import support


@pytest.mark.parametrize("st", support.GRID_STS_HOST)
def test_spline_block_operator_is_scipys_cubic_interpolant(st):
    """noise_gen.py:38-47 as the reference writes it: interp1d through the 11 points of a block at 15-minute spacing,
    evaluated on the sensor grid, first sample dropped.  Reference against reference: measured <= 8.9e-16 on unit-normal
    points; the bound leaves a factor of about 100 for other BLAS builds."""
    from scipy.interpolate import interp1d
    from oracle import t1d_oracle as O
    W = O.spline_block_operator(st)
    t15 = np.arange(0, 151, 15, dtype=np.float64)
    nsample = int(np.floor(150 / st)) + 1
    t = np.arange(0, nsample) * float(st)                       # noise_gen.py:41-44
    assert W.shape == (150 // st, 11) and t[-1] <= 150.0
    rs = np.random.RandomState(100 + st)
    worst = 0.0
    for _ in range(20):
        y = rs.randn(11)
        worst = max(worst, np.abs(W @ y - interp1d(t15, y, kind="cubic")(t)[1:]).max())
    print("st = %3d: max |W y - interp1d| = %.2e" % (st, worst))
    assert worst < 1e-13, worst


@pytest.mark.parametrize("st", support.GRID_STS_HOST)
def test_oracle_run_of_the_grid_is_finite_and_reaches_level_2(st):
    """what test_gpu_sensor_grid.py compares the device with: no normal is missing, every output is finite, the clock ends
    at K st, and the step-size rule put minutes at level 2"""
    inp = support.grid_inputs(st)
    S, K = inp["S"], inp["K"]
    assert 2 + K > 2 * S                                         # a third noise block is opened
    assert inp["z"].shape[0] >= 1 + 10 * (1 + (K + 1) // S)      # ten rows for every block up to the last sample's
    r = support.grid_oracle(st)
    for key in support.GRID_OUT + ("x", "last_cgm"):
        assert np.isfinite(r[key]).all(), key
    assert (r["t"] == K * st).all()
    assert r["level_count"][2] > 0, r["level_count"]
    d = support.grid_oracle(st, "dopri")
    assert np.isfinite(d["bg"]).all() and np.isfinite(d["cgm"]).all() and np.isfinite(d["x"]).all()


@pytest.mark.parametrize("st", (4, 20, 150))
def test_overflow_inputs_put_more_lanes_at_level_2_than_a_workgroup_has_records(st):
    """the inputs of test_multi_minute_overflow_path_follows_the_oracle: 315 envs in one workgroup, every env fed, 64 records.
    A lane leaves at most one record per launch, so the step with the meal must hold more than 64 + 64 envs at level 2."""
    lanes = support.grid_level2_lanes(st, 315, feed=1)
    assert lanes[0] == 0 and lanes[1] == 315 and lanes.max() - 64 >= 64, lanes
    # the grid's own inputs cannot get there: 50 fed envs of 150
    assert support.grid_level2_lanes(st, support.GRID_N, feed=3).max() == 50


def test_oracle_dopri5_moves_under_one_ulp_of_the_initial_state():
    """How far the exact-mode reference is from itself: the oracle's DOPRI5 run of the grid at st = 7 with every initial
    state word moved by one ulp up or down.  Most envs stay within 1e-8 mg/dL; a few take an accept/reject decision the
    other way and move by up to 5.4e-5 (measured: 7 envs of 150 beyond 1e-8 over these three draws, 5.7e-5 over six; the
    largest on the envs of patient 24) -- which
    is why the device test holds the exact mode to test_gpu_dopri5.py's batch bound (5e-4) and not to 1e-5."""
    from oracle import t1d_oracle as O
    st = 7
    inp = support.grid_inputs(st)
    _, tab = O.patient_table()
    x0 = tab[inp["pid"], :13].T.copy()

    def bg_trace(x):
        orc = O.OracleEnv(inp["pid"], normals=inp["z"], integrator="dopri", sensor_row_override=inp["row"])
        orc.reset(x0=x)
        return np.stack([orc.step(support.grid_action(inp, k), None, inp["cho"][k * st:(k + 1) * st])["bg"] for k in range(inp["K"])])
    base = bg_trace(x0)
    assert np.array_equal(base, support.grid_oracle(st, "dopri")["bg"][1:])
    rs = np.random.RandomState(1)
    worst = np.zeros(inp["n"])
    for _ in range(3):
        worst = np.maximum(worst, np.abs(bg_trace(x0 * (1.0 + 2.3e-16 * rs.choice([-1.0, 1.0], size=x0.shape))) - base).max(0))
    print("oracle DOPRI5 at st = 7 under one ulp: %d of %d envs beyond 1e-8, max %.2e mg/dL" % ((worst > 1e-8).sum(), len(worst), worst.max()))
    assert worst.max() <= 5e-4


@pytest.mark.parametrize("st", (3, 7))
def test_uneven_cuts_hold_a_launch_with_two_samples_one_opening_a_block(st):
    """the launch lengths of the device test: the same K st minutes, and a launch that takes two or more samples of which
    one opens a noise block strictly inside it"""
    K, S = support.grid_inputs(st)["K"], 150 // st
    cuts = support.uneven_cuts(st, K * st)
    assert sum(cuts) == K * st and min(cuts) >= 1
    assert any(m == 1 for m in cuts) and any(m < st for m in cuts) and any(m > st for m in cuts)
    found, t0 = False, 0
    for m in cuts:
        samples = [t1 for t1 in range(t0 + 1, t0 + m + 1) if t1 % st == 0]
        opens = [t1 for t1 in samples if (1 + t1 // st) % S == 0 and t0 + 1 <= t1 < t0 + m]
        found = found or (len(samples) >= 2 and bool(opens))
        t0 += m
    assert found
    # a launch of 2 st minutes that spans two whole steps: at st = 7 the one that starts at minute 231.  At st = 3 the pattern
    # is 27 minutes long, a multiple of st, and its 2 st launch starts at minute 7 of every period: none lies on a step boundary
    pair = support.whole_pair_launch(st, cuts)
    if st == 7:
        assert pair is not None and sum(cuts[:pair[0]]) == 231 and pair[1] == 33
    else:
        assert pair is None
