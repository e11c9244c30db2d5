"""Closed-loop roll-outs in the exact mode on the GPU (rollout_pid_dopri5 / rollout_bb_dopri5: dopri5_rollout_kernel, every
lane at its own pace inside a launch): bit for bit the step() loop with the controller evaluated operation by operation,
independent of the other envs of the batch, and the reference's own closed-loop files.  Inputs and envs come from
support.py; comparisons are by value (torch.equal): a NaN anywhere fails them.  _step_loop and _rollout stay here: they
evaluate a PID or basal-bolus controller in torch, those of test_gpu_policy_dopri5.py a network through policy_action."""
import functools
import os
from datetime import datetime

import numpy as np
import pytest

import support
from support import GOLDEN, ST, dense_cho as _dense_cho, exact_inputs as _inputs

pytestmark = pytest.mark.gpu
_mk = functools.partial(support.plain_env, integrator="dopri5")
_env = functools.partial(support.host_noise_env, start=None)         # no start_minute: these controllers take no time of day
STATE = ("x", "t", "cgm", "bg", "reward", "last_cgm", "prev_risk", "planned", "h_carry")
MILD = (1.5e-4, 4e-7, 5e-4)


def _step_loop(e, kind, K, gains=MILD, target=140.0, state=None):
    """A: one launch per step, the controller in torch fp64 between the launches, in the order rollout_body writes it
    (torch does not fuse: every product is rounded before it is added).  state: the controller state an earlier call
    returned, to go on from it.  -> controller state, trace rows, summed nfev"""
    import torch
    n, dv = e.n, e.device
    zero = torch.zeros(n, dtype=torch.float64, device=dv)
    rows = {k: [] for k in ("bg", "cgm", "cho", "insulin")}
    nf = torch.zeros(n, dtype=torch.int64, device=dv)
    obs = e.cgm.clone()
    if kind == "bb":
        c = e.bb_constants()
        meal = zero.clone() if state is None else state["prev_meal"].clone()
    else:
        P, I, D = gains
        integ, prev = (zero.clone(), zero.clone()) if state is None else (state["integ"].clone(), state["prev"].clone())
    for k in range(K):
        if kind == "bb":
            corr = torch.where(obs > 150.0, (obs - target) / c["cf"], zero)
            bolus = torch.where(meal > 0, ((meal * float(ST)) / c["cr"] + corr) / float(ST), zero)
            e.step(c["basal"], bolus)
            meal = e.meal.clone()
        else:
            u = P * (obs - target) + I * integ + D * (obs - prev) / float(ST)
            prev = obs.clone()
            integ = integ + (obs - target) * float(ST)
            e.step(u, zero)
        obs = e.cgm.clone()
        nf += e.nfev
        for key, t in (("bg", e.bg), ("cgm", e.cgm), ("cho", e.meal), ("insulin", e.insulin)):
            rows[key].append(t.clone())
    state = {"prev_meal": meal} if kind == "bb" else {"integ": integ, "prev": prev}
    return state, {k: torch.stack(v) for k, v in rows.items()}, nf


def _rollout(e, kind, chunks, gains=MILD, stats=None, **kw):
    """B: the roll-out in calls of the given lengths -> controller state, trace, summed nfev"""
    import torch
    tr = e.new_trace(sum(chunks))
    state = None
    nf = torch.zeros(e.n, dtype=torch.int64, device=e.device)
    for ch in chunks:
        if kind == "bb":
            state = e.rollout_bb_dopri5(ch, bb_state=state, stats=stats, trace=tr, **kw)
        else:
            state = e.rollout_pid_dopri5(ch, *gains, pid_state=state, stats=stats, trace=tr, **kw)
        nf += e.nfev
    return state, tr, nf


@pytest.mark.parametrize("kind", ["bb", "pid"])
def test_rollout_equals_step_loop_bit_for_bit(kind):
    """Independence from the neighbours: in A the 64 envs of a wave are in the same minute in every launch, in B each lane is
    wherever its own step sizes have taken it.  Every word must still be equal."""
    import torch
    n, K = 192, 160
    inp = _inputs(n, K)
    ea, eb, ec = _env(*inp), _env(*inp), _env(*inp)
    sa, rows, nfa = _step_loop(ea, kind, K)
    sb_, tr, nfb = _rollout(eb, kind, (1, 9, 70, 80))
    support.same_env(ea, eb, STATE, by="value")
    for k in sa:
        assert torch.equal(sa[k], sb_[k]), k
    for k in rows:
        assert torch.equal(rows[k], tr[k][1:]), k
    assert torch.equal(nfa, nfb)
    assert ea.sync() == 0 and eb.sync() == 0
    assert int(eb.t.min()) == K * ST == int(eb.t.max())
    assert bool((rows["cho"] > 0).any()) and bool((rows["insulin"] > 0).any())
    # one call, uncut (160 steps = 480 minutes in one launch) against launches of 30 minutes
    sc, trc, nfc = _rollout(ec, kind, (K,), max_minutes_per_launch=10 ** 6)
    ed = _env(*inp)
    sd, trd, nfd = _rollout(ed, kind, (K,), max_minutes_per_launch=30)
    support.same_env(ec, ed, STATE, by="value"); support.same_env(ec, eb, STATE, by="value")
    for k in sc:
        assert torch.equal(sc[k], sd[k]) and torch.equal(sc[k], sb_[k]), k
    for k in ("bg", "cgm", "cho", "insulin"):
        assert torch.equal(trc[k][1:], trd[k][1:]) and torch.equal(trc[k][1:], tr[k][1:]), k       # row 0: what reset() recorded
    assert torch.equal(nfc, nfd) and torch.equal(nfc, nfb)
    assert ec.sync() == 0 and ed.sync() == 0


@pytest.mark.parametrize("kind", ["bb", "pid"])
def test_the_same_env_in_different_company(kind):
    import torch
    n, K = 128, 120
    pid, z, mt, ma = _inputs(n, K, seed=11)
    E = 77                                         # the env under test: column 77 of the inputs (patient 17)
    traces = []
    for cols in (np.full(64, E), np.r_[E, np.arange(1, n)], np.r_[np.arange(0, 37), E, np.arange(38, n)], np.array([E])):
        e = _env(pid, z, mt, ma, cols=cols)
        _, tr, _ = _rollout(e, kind, (K,))
        lane = int(np.where(cols == E)[0][0])
        assert lane in (0, 37)
        traces.append({k: tr[k][1:, lane].clone() for k in ("bg", "cgm", "cho", "insulin")})
        if len(cols) == 64:                        # the replicas among themselves
            assert bool((tr["bg"][1:] == tr["bg"][1:, :1]).all()) and bool((e.x == e.x[:, :1]).all())
        assert e.sync() == 0
    for t in traces[1:]:
        for k in t:
            assert torch.equal(t[k], traces[0][k]), k


def _ref_csv(name):
    import pandas as pd
    return pd.read_csv(os.path.join(GOLDEN, name), index_col=0, parse_dates=True)


@pytest.mark.parametrize("case", ["g6", "g10", "upstream"])
def test_reference_closed_loop_files(golden, case):
    """The reference's recorded closed loops through the roll-out and the device-resident history, at the bars the oracle's
    own DOPRI5 meets against the same files on the CPU (tests/test_oracle_golden.py)."""
    from simglucose_amd import scenario_batch as sb
    from simglucose_amd.analysis import report
    from oracle import t1d_oracle as O
    name, fname, sensor_seed, scen_seed, K = {"g6": ("adult#001", "g6_config1_adult001_bb.csv", 1, 1, 480),
                                              "g10": ("adult#001", "g10_pid_adult001.csv", 5, 9, 480),
                                              "upstream": ("adolescent#001", "upstream_sim_results.csv", 1, 1, 960)}[case]
    ref = _ref_csv(fname)
    assert len(ref) == K + 1
    z = golden("g10_pid_actions.npz")["randn"] if case == "g10" else np.random.RandomState(sensor_seed).randn(1 + 10 * (2 + K * ST // 150))
    cho = O.random_scenario_cho(scen_seed, 0, K * ST)
    lst = [(int(m), float(cho[m])) for m in np.nonzero(cho)[0]]
    n = 3
    e = _mk(patient=name, n_envs=n, sensor="Dexcom", noise="host", normals=np.repeat(np.asarray(z)[:, None], n, 1))
    mt, ma = sb.tables_from_minute_lists([lst] * n, device=e.device)
    e.set_meals(mt, ma)
    e.reset()
    tr = e.new_trace(K)
    if case == "g10":
        e.rollout_pid_dopri5(K, 0.001, 0.00001, 0.001, 140.0, trace=tr)
    else:
        e.rollout_bb_dopri5(K, trace=tr)
    assert e.sync() == 0
    df = report.history_frame(tr, 1, datetime(2018, 1, 1, 0, 0, 0), ST)
    assert list(df.columns) == list(ref.columns) and len(df) == len(ref)
    worst = {}
    for col in ref.columns:
        got, exp = df[col].to_numpy(), ref[col].to_numpy()
        assert np.array_equal(np.isnan(got), np.isnan(exp)), col
        worst[col] = float(np.nanmax(np.abs(got - exp)))
    print(case, worst)
    for col in ref.columns:
        assert worst[col] <= {"CHO": 1e-12, "insulin": 1e-9}.get(col, 1e-6), (col, worst)


@pytest.mark.parametrize("n,n_sample,edge", [(1 << 18, 300, 130), (1 << 20, 200, 70)])
def test_large_batch_sampled_envs_match_oracle(n, n_sample, edge):
    """Dexcom, Philox noise, random meal tables from 06:00, the mild PID gains, 160 steps (8 h, two launches of 240 minutes);
    envs sampled across the batch (first and last workgroups, every patient) replayed on the oracle's dopri with the
    kernel's own normals and meals and the controller in numpy.  Bars as for the step kernel on such a replay
    (tests/test_gpu_dopri5.py): at least 95 % of the sampled traces within 1e-8, all within 5e-4 mg/dL -- the device's tanh
    and pow are not glibc's, and where that decides an accept/reject the trace moves by up to the solver's tolerance."""
    import torch
    from simglucose_amd import scenario_batch as sb
    from oracle import t1d_oracle as O
    K = 160
    pid = np.arange(n) % 30
    e = _mk(patient=pid, sensor="Dexcom", noise="philox", seed=56, extra_outputs=False)
    mt, ma = sb.random_meal_tables(n, days=1, start_minute_of_day=6 * 60, seed=22, device=e.device)
    e.set_meals(mt, ma)
    rs = np.random.RandomState(3)
    sample = np.unique(np.concatenate([np.arange(0, edge), np.arange(n - edge, n), rs.randint(0, n, 60)]))[:n_sample]
    assert len(set(pid[sample])) == 30
    sidx = torch.as_tensor(sample, device=e.device)
    z = e.philox_normals(1 + 10 * (2 + K * ST // 150), draw0=0, episode=1)[:, sidx].cpu().numpy()
    cho = _dense_cho(mt, ma, sample, K * ST)
    orc = O.OracleEnv(pid[sample], sensor="Dexcom", normals=z, integrator="dopri")
    e.reset()
    r = orc.reset()
    P, I, D = MILD
    target = 140.0
    tr = e.new_trace(K, columns=("bg", "cgm"))
    e.rollout_pid_dopri5(K, P, I, D, target, trace=tr)
    assert e.sync() == 0
    assert int(e.t.min()) == K * ST == int(e.t.max())
    obs = r["cgm"].copy(); integ = np.zeros(len(sample)); prev = np.zeros(len(sample))
    worst = np.zeros(len(sample))
    bg_d, cgm_d = tr["bg"][1:, sidx].cpu().numpy(), tr["cgm"][1:, sidx].cpu().numpy()
    for k in range(K):
        u = P * (obs - target) + I * integ + D * (obs - prev) / ST              # pid_ctrller.py:17-36
        prev = obs.copy(); integ = integ + (obs - target) * ST
        o = orc.step(u, None, cho[k * ST:(k + 1) * ST])
        obs = o["cgm"]
        worst = np.maximum(worst, np.maximum(np.abs(bg_d[k] - o["bg"]), np.abs(cgm_d[k] - o["cgm"])))
    print("%d envs: %.1f %% of %d sampled traces within 1e-8 of the oracle, max %.3e; RHS per env-minute %.2f"
          % (n, 100 * (worst <= 1e-8).mean(), len(sample), worst.max(), float(e.nfev.double().mean()) / (K * ST)))
    assert (worst <= 1e-8).mean() >= 0.95 and worst.max() <= 5e-4, ((worst <= 1e-8).mean(), worst.max())
    assert bool(torch.isfinite(e.bg).all())


def test_solver_failure_inside_a_rollout():
    """The stiff-patient construction of test_gpu_dopri5.py (kabs x 1e6: DOPRI5 would need far more than its 500 steps in a
    minute) inside a roll-out: the status bit, a finite state, and the normal envs as if the stiff ones were not there."""
    import torch
    from simglucose_amd import _lib
    from oracle import t1d_oracle as O
    names, tab = O.patient_table()
    rows = tab[[names.index("adult#001"), names.index("adult#001")]].copy()
    rows[1, O.IDX["kabs"]] *= 1e6
    n, K = 128, 10
    pid = (np.arange(n) % 16 == 5).astype(np.int64)
    normal = np.where(pid == 0)[0]
    rs = np.random.RandomState(9)
    z = rs.randn(21, n)
    mt = np.stack([np.full(n, 4), np.full(n, 17)]).astype(np.int64)
    ma = rs.uniform(30.0, 60.0, size=(2, n))
    out = []
    for cols in (np.arange(n), normal):
        e = _mk(patient=pid[cols], patient_table=rows, sensor="Dexcom", noise="host", normals=z[:, cols])
        e.set_meals(torch.as_tensor(mt[:, cols]), torch.as_tensor(ma[:, cols]))
        e.reset()
        tr = e.new_trace(K)
        e.rollout_bb_dopri5(K, trace=tr)
        st = e.sync(raise_on_status=False)
        out.append((e, tr, st))
    (ea, tra, sta), (eb, trb, stb) = out
    assert sta & _lib.T1D_ST_SOLVER_FAILED and not (sta & _lib.T1D_ST_NONFINITE), sta
    assert stb == 0
    assert bool(torch.isfinite(ea.x).all()) and int(ea.t.min()) == K * ST == int(ea.t.max())
    nidx = torch.as_tensor(normal, device=ea.device)
    for k in ("bg", "cgm", "cho", "insulin"):
        assert torch.equal(tra[k][1:, nidx], trb[k][1:]), k
    for k in STATE:
        assert torch.equal(getattr(ea, k)[..., nidx], getattr(eb, k)), k


def test_statistics_and_partial_reset():
    import torch
    from simglucose_amd.analysis.risk import risk_index
    n, K = 96, 60
    inp = _inputs(n, 2 * K, seed=21)
    e, cont, fresh = _env(*inp), _env(*inp), _env(*inp)
    dv = e.device
    stats = {"sum_risk": torch.zeros(n, dtype=torch.float64, device=dv),
             "min_bg": torch.full((n,), 1e9, dtype=torch.float64, device=dv),
             "max_bg": torch.zeros(n, dtype=torch.float64, device=dv),
             "n_low": torch.zeros(n, dtype=torch.int32, device=dv), "n_high": torch.zeros(n, dtype=torch.int32, device=dv)}
    gains = (1e-3, 1e-5, 1e-3)                                  # the reference's: strong enough for lows and highs
    state, tr, _ = _rollout(e, "pid", (7, K - 7), gains=gains, stats=stats)
    bg = tr["bg"][1:]
    assert torch.equal(stats["min_bg"], bg.min(0).values) and torch.equal(stats["max_bg"], bg.max(0).values)
    assert torch.equal(stats["n_low"].long(), (bg < 70).sum(0)) and torch.equal(stats["n_high"].long(), (bg > 180).sum(0))
    assert int(stats["n_high"].sum()) > 0
    # the risk index of every step's BG, recomputed on the host (risk.py:5-17): log and pow of the host's libm against the
    # device's, a few ulp of a sum of K terms of order 1..100 -> 1e-9 absolute is ~1e4 ulp of headroom and far below any
    # wrong term (one missed step changes the sum by its whole risk, > 1e-3)
    want = np.array([sum(risk_index([v], 1)[2] for v in col) for col in bg.cpu().numpy().T])
    assert np.abs(stats["sum_risk"].cpu().numpy() - want).max() <= 1e-9 * max(1.0, want.max()), np.abs(stats["sum_risk"].cpu().numpy() - want).max()
    # partial reset: the reset envs start over like a fresh env (probed first step), the others continue
    state_c, _, _ = _rollout(cont, "pid", (K,), gains=gains)
    mask = torch.as_tensor((np.arange(n) % 3 == 1).astype(np.uint8))
    mb = mask.bool().to(dv)
    e.reset(mask=mask)
    assert bool((e.h_carry[mb] == 0).all()) and bool((e.h_carry[~mb] != 0).all())
    for k in ("integ", "prev"):
        assert torch.equal(state[k], state_c[k]), k
        state[k][mb] = 0.0
    _, tr2, _ = _rollout_with_state(e, K, gains, state)
    _, trc, _ = _rollout_with_state(cont, K, gains, state_c)
    _, trf, _ = _rollout(fresh, "pid", (K,), gains=gains)
    for k in ("bg", "cgm", "cho", "insulin"):
        assert torch.equal(tr2[k][1:, mb], trf[k][1:, mb]), k
        assert torch.equal(tr2[k][1:, ~mb], trc[k][1:, ~mb]), k
    for k in STATE:
        assert torch.equal(getattr(e, k)[..., mb], getattr(fresh, k)[..., mb]), k
        assert torch.equal(getattr(e, k)[..., ~mb], getattr(cont, k)[..., ~mb]), k
    assert e.sync() == 0 and cont.sync() == 0 and fresh.sync() == 0


def _rollout_with_state(e, K, gains, state):
    import torch
    tr = {"row": 1}
    for k in ("bg", "cgm", "cho", "insulin"):
        tr[k] = torch.full((K + 1, e.n), float("nan"), dtype=torch.float64, device=e.device)
    st = e.rollout_pid_dopri5(K, *gains, pid_state=state, trace=tr)
    return st, tr, None


def test_surface_errors():
    """the new methods take exact-mode envs only; the old ones keep refusing them"""
    from simglucose_amd import _lib
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    fixed = BatchedT1DSimEnv(patient="adult#001", n_envs=4, sensor="Dexcom")
    fixed.reset()
    with pytest.raises(_lib.T1DError, match="dopri5"):
        fixed.rollout_pid_dopri5(2, *MILD)
    with pytest.raises(_lib.T1DError, match="dopri5"):
        fixed.rollout_bb_dopri5(2)
    exact = _mk(patient="adult#001", n_envs=4, sensor="Dexcom")
    exact.reset()
    with pytest.raises(_lib.T1DError, match="DOPRI5"):
        exact.rollout_pid(2, *MILD)
    with pytest.raises(ValueError):
        exact.rollout_pid_dopri5(0, *MILD)
    exact.rollout_pid_dopri5(2, *MILD)
    assert exact.sync() == 0 and int(exact.t[0]) == 6
