"""The exact mode on the GPU: t1d_step_dopri5 (scipy's dopri5 as the reference drives it) against the reference's golden
vectors and the oracle's restatement of the same driver (oracle/t1d_oracle.c, t1d_o_dopri5_minute), from one env to
262 144, through every layer of the Python surface."""
import functools
import os
from datetime import datetime, timedelta

import numpy as np
import pytest

import support
from support import GOLDEN, basal_of as _basal, golden_hist as _hist

pytestmark = pytest.mark.gpu
_mk = functools.partial(support.plain_env, integrator="dopri5")
INSULET_EXACT = np.array([0.0, 1e9, 1e-9, 0.0, 1e9, 1e-9])      # a pump that (almost) passes the action through


@pytest.mark.parametrize("sensor", ["Dexcom", "Navigator", "GuardianRT"])
@pytest.mark.parametrize("pname", ["adult#001", "child#003"])
def test_g5_env_steps_match_reference_and_oracle(golden, sensor, pname):
    """G5 (T1DSimEnv.step of the reference, every output) on three replicas of one env, host normals."""
    import torch
    from oracle import t1d_oracle as O
    g = golden("g5_env.npz")
    tag = "%s_%s" % (sensor, pname.replace("#", ""))
    names, _ = O.patient_table()
    st = int(O.sensor_row(sensor)[5])
    nstep = len(g["basal_" + tag])
    cho = O.custom_scenario_cho(g["scen_hours"], g["scen_grams"], nstep * st)
    R = 3
    z = np.repeat(g["randn_" + tag][:, None], R, axis=1)
    ip = names.index(pname)
    env = _mk(patient=[ip] * R, sensor=sensor, noise="host", normals=z)
    orc = O.OracleEnv([ip], sensor=sensor, normals=g["randn_" + tag][:, None], integrator="dopri")
    env.reset(); orc.reset()
    worst = {"bg": 0.0, "orc": 0.0, "rr": 0.0, "state": 0.0}
    for k in range(nstep):
        c = np.repeat(cho[k * st:(k + 1) * st, None], R, axis=1)
        obs, rew, done, info = env.step(g["basal_" + tag][k], g["bolus_" + tag][k], cho=c)
        r = orc.step(g["basal_" + tag][k], g["bolus_" + tag][k], cho[k * st:(k + 1) * st, None])
        bg, cg = info["bg"].cpu().numpy(), obs.cpu().numpy()
        x = env.x.cpu().numpy()
        for a in (bg, cg, rew.cpu().numpy(), x):
            assert np.array_equal(a[..., 0:1].repeat(R, axis=-1), a), k          # replicas bitwise equal
        worst["bg"] = max(worst["bg"], abs(bg[0] - g["bg_" + tag][k]), abs(cg[0] - g["cgm_" + tag][k]))
        worst["rr"] = max(worst["rr"], abs(rew[0].item() - g["reward_" + tag][k]), abs(info["risk"][0].item() - g["risk_" + tag][k]))
        worst["state"] = max(worst["state"], np.abs(x[:, 0] - g["state_" + tag][k]).max())
        worst["orc"] = max(worst["orc"], abs(bg[0] - r["bg"][0]), abs(cg[0] - r["cgm"][0]))
        assert bool(done[0]) == bool(g["done_" + tag][k]), k
    assert env.sync() == 0
    # bars the oracle's own dopri path meets against the reference (tests/test_oracle_golden.py)
    assert worst["bg"] < 1e-8 and worst["rr"] < 1e-7 and worst["state"] < 1e-6, worst
    assert worst["orc"] < 1e-8, worst
    hc = env.h_carry.cpu().numpy()
    assert np.abs(hc - orc.h_carry[0]).max() <= 1e-9 * abs(orc.h_carry[0]), (hc, orc.h_carry)


def test_g2_all_30_patients_24h_nfev_and_traces(golden):
    """G2, 30 patients x 24 h open loop in one batch (the pump passes the action through, as in
    test_gpu_parity.py::test_all_30_patients_24h_vs_scipy_and_oracle): against the reference's SciPy traces, against the
    oracle's dopri per patient, and the solver's control flow (RHS evaluations per minute) against the oracle's."""
    import torch
    from oracle import t1d_oracle as O
    g = golden("g2_openloop.npz")
    names, tab = O.patient_table()
    n = 30
    env = _mk(patient=np.arange(n), sensor="Navigator", pump_row=INSULET_EXACT)
    env.reset()
    cho = np.zeros(1440)
    for m, gr in zip(g["meal_minute"], g["meal_grams"]):
        cho[int(m)] = gr
    orc = [O.PatientOracle(tab[ip]) for ip in range(n)]
    vg = tab[:, O.IDX["Vg"]]
    worst_s = np.zeros(n); worst_o = np.zeros(n)
    same_nfev = 0
    for t in range(1440):
        a = torch.as_tensor(g["basal"] * g["action_mult"][t], dtype=torch.float64, device=env.device)
        c = torch.full((1, n), float(cho[t]), dtype=torch.float64, device=env.device)
        _, _, _, info = env.step(a, cho=c)
        nf = env.nfev.cpu().numpy()
        for ip in range(n):
            q = O.pump(g["basal"][ip] * g["action_mult"][t], 1e-9, 0.0, 1e9)
            orc[ip].step(cho[t], q, integrator="dopri")
            same_nfev += int(nf[ip] == orc[ip].nfcn)
        bg = info["bg"].cpu().numpy()
        worst_s = np.maximum(worst_s, np.abs(bg - g["gsub_default"][:, t + 1]))
        worst_o = np.maximum(worst_o, np.abs(bg - np.array([orc[ip].x[12] / vg[ip] for ip in range(n)])))
    assert env.sync() == 0
    print("nfev equal to the oracle's in %d of %d patient-minutes; max vs SciPy %.3e, vs oracle %.3e, %d patients within 1e-8"
          % (same_nfev, n * 1440, worst_s.max(), worst_o.max(), (worst_o <= 1e-8).sum()))
    # Measured (MI355X): the RHS counts agree in 43 190 of the 43 200 patient-minutes and 28 patients stay within 1e-8 of
    # the oracle.  The solver is chaotic at the ulp level: the device's tanh and pow (ocml) are not glibc's, and where such
    # a difference decides an accept/reject at the tolerance boundary the trace moves by up to the solver's tolerance
    # (rtol 1e-6 of BG) -- one patient ends 9.8e-5 from the oracle and 9.3e-5 from SciPy (the oracle's own bar against
    # SciPy, 2e-5, is one such flip smaller).  Bounds: the measured values with a margin of two.
    assert same_nfev >= 0.99 * n * 1440, same_nfev
    assert worst_s.max() <= 2e-4, worst_s.max()
    assert (worst_o <= 1e-8).sum() >= 28 and worst_o.max() <= 2e-4, worst_o


def test_1024_replicas_of_one_patient_are_bitwise_equal(golden):
    """config-2 shape: 1 024 replicas of adult#001 under the G2 inputs of that patient."""
    import torch
    from oracle import t1d_oracle as O
    g = golden("g2_openloop.npz")
    names, _ = O.patient_table()
    ip = names.index("adult#001")
    n = 1024
    env = _mk(patient=[ip] * n, sensor="Navigator", pump_row=INSULET_EXACT, extra_outputs=False)
    env.reset()
    cho = np.zeros(1440)
    for m, gr in zip(g["meal_minute"], g["meal_grams"]):
        cho[int(m)] = gr
    worst = 0.0
    for t in range(1440):
        env.step(float(g["basal"][ip] * g["action_mult"][t]), cho=torch.full((1, n), float(cho[t]), dtype=torch.float64, device=env.device))
        if t % 30 == 29 or t == 1439:
            bg = env.bg.cpu().numpy()
            assert np.array_equal(bg, np.full(n, bg[0])), t
            worst = max(worst, abs(bg[0] - g["gsub_default"][ip, t + 1]))
    assert env.sync() == 0
    assert bool((env.x == env.x[:, :1]).all()) and bool((env.h_carry == env.h_carry[0]).all())
    assert worst <= 2e-5, worst


def test_reference_regression_test_on_the_gpu_surface():
    """The reference's tests/test_sim_engine.py (adolescent#001, Dexcom seed 1, Insulet, RandomScenario seed 1,
    BBController, 2 days == sim_results.csv) with the reference's own assertion, assert_frame_equal(rtol=1e-5)."""
    import pandas as pd
    from simglucose_amd.simulation.env import T1DSimEnv
    from simglucose_amd.controller.basal_bolus_ctrller import BBController
    from simglucose_amd.sensor.cgm import CGMSensor
    from simglucose_amd.actuator.pump import InsulinPump
    from simglucose_amd.patient.t1dpatient import T1DPatient
    from simglucose_amd.simulation.scenario_gen import RandomScenario
    from simglucose_amd.simulation.sim_engine import SimObj, sim
    start_time = datetime(2018, 1, 1, 0, 0, 0)
    env = T1DSimEnv(T1DPatient.withName("adolescent#001"), CGMSensor.withName("Dexcom", seed=1),
                    InsulinPump.withName("Insulet"), RandomScenario(start_time=start_time, seed=1), integrator="dopri5")
    results = sim(SimObj(env, BBController(), timedelta(days=2), animate=False, path=None))
    exp, times = _hist("upstream_sim_results.csv")
    assert len(results) == 961 and list(results.columns) == ["BG", "CGM", "CHO", "insulin", "LBGI", "HBGI", "Risk"]
    for col in exp:
        got = results[col].to_numpy()
        assert np.array_equal(np.isnan(got), np.isnan(exp[col])), col
        ok = ~np.isnan(exp[col])
        tol = {"CHO": 1e-12, "insulin": 1e-9}.get(col, 1e-6)
        assert np.abs(got[ok] - exp[col][ok]).max() <= tol, (col, np.abs(got[ok] - exp[col][ok]).max())
    ref = pd.read_csv(os.path.join(GOLDEN, "upstream_sim_results.csv"), index_col=0, parse_dates=True)
    got = results.copy()
    got.index = ref.index
    pd.testing.assert_frame_equal(got, ref, rtol=1e-5, check_dtype=False, check_freq=False, check_names=False)


def test_standalone_patient_matches_oracle():
    from simglucose_amd.patient.t1dpatient import T1DPatient, Action
    from oracle import t1d_oracle as O
    p = T1DPatient.withName("child#005", integrator="dopri5")
    names, tab = O.patient_table()
    orc = O.PatientOracle(tab[names.index("child#005")])
    basal = float(p._params.u2ss * p._params.BW / 6000)
    for t in range(90):
        cho = 50.0 if t == 10 else 0.0
        ins = basal * (3.0 if 10 <= t < 13 else 1.0)
        p.step(Action(CHO=cho, insulin=ins))
        orc.step(cho, ins, integrator="dopri")
    assert p.t == 90
    assert np.abs(p.state - orc.x).max() < 1e-8, np.abs(p.state - orc.x).max()


def test_partial_reset_zeroes_h_carry_and_matches_fresh_and_continuing_oracles():
    """Dexcom steps (3 minutes per launch, so the predicted step crosses minutes inside a launch); half the envs reset at
    step 40 start over with a probed initial step, the others carry theirs on."""
    import torch
    from oracle import t1d_oracle as O
    n = 64
    pid = (np.arange(n) * 7) % 30
    z = np.random.RandomState(5).randn(64, n)
    env = _mk(patient=pid, sensor="Dexcom", noise="host", normals=z)
    orc = O.OracleEnv(pid, sensor="Dexcom", normals=z, integrator="dopri")
    basal = _basal(pid)
    env.reset(); orc.reset()

    def drive(k, envs):
        c = np.zeros((3, n))
        if k % 25 == 3:
            c[0, :] = 40.0
        bol = np.where(np.arange(n) % 5 == 0, 0.5, 0.0) if k % 25 == 4 else np.zeros(n)
        a = basal * (0.6 + 0.2 * (k % 4))
        env.step(a, bol, cho=c)
        return [o.step(a[sel], bol[sel], c[:, sel]) for o, sel in envs]

    allsel = np.arange(n)
    for k in range(40):
        drive(k, [(orc, allsel)])
    assert bool((env.h_carry != 0).all())
    mask = np.arange(n) % 2 == 1
    keep_i, reset_i = np.where(~mask)[0], np.where(mask)[0]
    env.reset(mask=torch.as_tensor(mask.astype(np.uint8)))
    assert bool((env.h_carry[torch.as_tensor(reset_i, device=env.device)] == 0).all())
    assert bool((env.h_carry[torch.as_tensor(keep_i, device=env.device)] != 0).all())
    fresh = O.OracleEnv(pid[reset_i], sensor="Dexcom", normals=z[:, reset_i], integrator="dopri")
    fresh.reset()
    kept = O.OracleEnv(pid[keep_i], sensor="Dexcom", normals=z[:, keep_i], integrator="dopri")
    kept.reset()
    for k in range(40):                                       # the kept envs' oracle replays their history first
        c = np.zeros((3, len(keep_i)))
        if k % 25 == 3:
            c[0, :] = 40.0
        bol = np.where(keep_i % 5 == 0, 0.5, 0.0) if k % 25 == 4 else np.zeros(len(keep_i))
        kept.step(basal[keep_i] * (0.6 + 0.2 * (k % 4)), bol, c)
    worst = np.zeros(n)
    for k in range(40, 80):
        rk, rf = drive(k, [(kept, keep_i), (fresh, reset_i)])
        bg, cg = env.bg.cpu().numpy(), env.cgm.cpu().numpy()
        worst[keep_i] = np.maximum(worst[keep_i], np.maximum(np.abs(bg[keep_i] - rk["bg"]), np.abs(cg[keep_i] - rk["cgm"])))
        worst[reset_i] = np.maximum(worst[reset_i], np.maximum(np.abs(bg[reset_i] - rf["bg"]), np.abs(cg[reset_i] - rf["cgm"])))
    assert env.sync() == 0
    print("partial reset: %d of %d envs within 1e-8 of the oracle, max %.3e" % ((worst <= 1e-8).sum(), n, worst.max()))
    # measured: max 3.2e-7 (an ulp-level accept/reject flip, see the G2 test); most envs follow the oracle to ~1e-12
    assert (worst <= 1e-8).mean() >= 0.9 and worst.max() <= 1e-5, ((worst <= 1e-8).mean(), worst.max())


@pytest.mark.parametrize("sensor,hours", [("Navigator", 6), ("Dexcom", 6)])
def test_large_batch_sampled_envs_match_oracle(sensor, hours):
    """262 144 envs with random meal tables, Philox noise and a random basal pool; 300 envs sampled across the batch
    replayed on the oracle's dopri with the very normals, meals and actions the kernel used."""
    import torch
    from simglucose_amd import scenario_batch as sb
    from oracle import t1d_oracle as O
    n = 1 << 18
    pid = np.arange(n) % 30
    e = _mk(patient=pid, sensor=sensor, noise="philox", seed=91, extra_outputs=False)
    st = int(e.sample_time)
    K = hours * 60 // st
    mt, ma = sb.random_meal_tables(n, days=1, start_minute_of_day=6 * 60, seed=8, device=e.device)
    e.set_meals(mt, ma)
    rs = np.random.RandomState(3)
    sample = np.unique(np.concatenate([np.arange(0, 130), np.arange(n - 130, n), rs.randint(0, n, 60)]))[:300]
    sidx = torch.as_tensor(sample, device=e.device)
    z = e.philox_normals(1 + 10 * (2 + K * st // 150), draw0=0, episode=1)[:, sidx].cpu().numpy()
    t_s, a_s = mt[:, sample].cpu().numpy().astype(np.int64), ma[:, sample].cpu().numpy()
    cho = np.zeros((K * st, len(sample)))
    for j in range(len(sample)):
        for tt, aa in zip(t_s[:, j], a_s[:, j]):
            if tt < K * st:
                cho[tt, j] = aa
    b0 = torch.as_tensor(_basal(pid), device=e.device)
    g = torch.Generator(device=e.device); g.manual_seed(5)
    pool = [(b0 * 2.0 * torch.rand(n, generator=g, device=e.device, dtype=torch.float64)).contiguous() for _ in range(8)]
    pool_s = [p[sidx].cpu().numpy() for p in pool]
    orc = O.OracleEnv(pid[sample], sensor=sensor, normals=z, integrator="dopri")
    e.reset(); orc.reset()
    worst = np.zeros(len(sample))
    for k in range(K):
        e.step(pool[k % 8])
        r = orc.step(pool_s[k % 8], None, cho[k * st:(k + 1) * st])
        if k % 8 == 7 or k == K - 1:
            worst = np.maximum(worst, np.abs(e.bg[sidx].cpu().numpy() - r["bg"]))
            worst = np.maximum(worst, np.abs(e.cgm[sidx].cpu().numpy() - r["cgm"]))
    print("%s: %.1f %% of sampled traces within 1e-8 of the oracle, max %.3e" % (sensor, 100 * (worst <= 1e-8).mean(), worst.max()))
    # measured: 96.3 % (Navigator) / 96.7 % (Dexcom) of the sampled traces within 1e-8, max 1.2e-4 / 1.5e-5 -- ulp-level
    # accept/reject flips as in the G2 test, each up to the solver's tolerance; the north star's bar against SciPy is 1e-3
    assert (worst <= 1e-8).mean() >= 0.95 and worst.max() <= 5e-4, ((worst <= 1e-8).mean(), worst.max())
    assert e.sync() == 0 and int(e.t.min()) == K * st == int(e.t.max())


def test_solver_budget_is_reported_not_faulted():
    """A patient row with kabs scaled by 1e6 (stiff: DOPRI5 would need far more than its 500 steps in a minute) next to
    normal envs: the oracle gives up on it, the kernel raises T1D_ST_SOLVER_FAILED and the other envs are unaffected."""
    import torch
    from simglucose_amd import _lib
    from oracle import t1d_oracle as O
    names, tab = O.patient_table()
    rows = tab[[names.index("adult#001"), names.index("adult#001")]].copy()
    rows[1, O.IDX["kabs"]] *= 1e6
    stiff = O.PatientOracle(rows[1])
    with pytest.raises(RuntimeError):
        stiff.step(50.0, 0.01, integrator="dopri")
    n = 128
    pid = (np.arange(n) % 16 == 5).astype(np.int64)          # a few stiff envs among normal ones
    z = np.random.RandomState(9).randn(40, n)
    env = _mk(patient=pid, patient_table=rows, sensor="Navigator", noise="host", normals=z)
    env.reset()
    normal = np.where(pid == 0)[0]
    orc = O.OracleEnv(np.zeros(len(normal), np.int32), sensor="Navigator", normals=z[:, normal], integrator="dopri",
                      ptab_override=rows)
    orc.reset()
    basal = float(_basal(np.array([names.index("adult#001")]))[0])
    worst = 0.0
    for k in range(30):
        c = np.full((1, n), 50.0 if k == 2 else 0.0)
        env.step(basal, cho=c)
        r = orc.step(np.full(len(normal), basal), None, c[:, normal])
        worst = max(worst, np.abs(env.bg.cpu().numpy()[normal] - r["bg"]).max())
    st = env.sync(raise_on_status=False)
    assert st & _lib.T1D_ST_SOLVER_FAILED, st
    assert worst <= 1e-8, worst
    assert bool(torch.isfinite(env.x).all())
    for k in range(2):
        env.step(basal)
    with pytest.raises(_lib.T1DError):
        env.sync()


def test_checkpoint_round_trip_and_rollouts_refused():
    import torch
    from simglucose_amd import _lib
    n = 96
    pid = np.arange(n) % 30
    z = np.random.RandomState(4).randn(40, n)
    basal = _basal(pid)

    def run(env, ks):
        for k in ks:
            c = np.zeros((3, n))
            if k == 4:
                c[0] = 60.0
            env.step(basal * (0.5 + 0.25 * (k % 3)), cho=c)

    a = _mk(patient=pid, sensor="Dexcom", noise="host", normals=z)
    a.reset()
    run(a, range(30))
    b = _mk(patient=pid, sensor="Dexcom", noise="host", normals=z)
    b.reset()
    run(b, range(15))
    sd = b.state_dict()
    assert "h_carry" in sd
    c = _mk(patient=pid, sensor="Dexcom", noise="host", normals=z)
    c.load_state_dict(sd)
    run(c, range(15, 30))
    for k in ("x", "h_carry", "cgm", "bg", "reward"):
        assert torch.equal(getattr(a, k), getattr(c, k)), k
    sd.pop("h_carry")
    with pytest.raises(_lib.T1DError):
        c.load_state_dict(sd)
    with pytest.raises(_lib.T1DError, match="DOPRI5"):
        c.rollout_pid(2, 1e-4, 1e-7, 1e-2)
    with pytest.raises(_lib.T1DError, match="DOPRI5"):
        c.rollout_bb(2)
    assert a.sync() == 0 and c.sync() == 0
