"""The controllers' collectors in the exact mode on the GPU (BatchedT1DSimEnv.collect_pid_dopri5 / collect_bb_dopri5 ->
t1d_collect_pid_dopri5 / t1d_collect_bb_dopri5, dopri5_ctrl_collect_kernel of csrc/t1d_dopri5.hpp): pinned bit for bit to
rollout_pid_dopri5 / rollout_bb_dopri5 (no episode ends) and to the loop of entry points the header names (episodes that end,
lanes of a wave in different steps and episodes); the action restated in torch; batches that are no multiple of 64, shards and
cuts; a solver that gives up; the shortest and the longest window.  fp64, Dexcom; every comparison is bit for bit.  The runs come
from support_ctrl_exact.py, each made once and shared."""
import numpy as np
import pytest

from support import (DAYS, EPISODE_STATS, POLICY_STATE, ST, STATE_EXACT, STATS, bits as _bits, gpu_torch as _torch,
                     gym_env as _mk_gym, same_dicts as _same_dicts, same_env as _same_env, stats as _stats)
from support_ctrl import COLS, CTRL_STATE, PID, ctrl_state, feature_policy
from support_ctrl_exact import call as _call, collector_run, loop_run

pytestmark = pytest.mark.gpu
ENV_KEYS = STATE_EXACT + ("meal_time", "meal_amt", "start_minute", "episode", "cgm0")
LOOP_COLS = tuple(c for c in COLS if c != "action")
KINDS = ["pid", "bb"]


def _same_run(ref, got, kind, sl=slice(None), cols=LOOP_COLS):
    """everything a run leaves: `got` (its envs are the envs `sl` of `ref`) against `ref`, bit for bit"""
    torch = _torch()
    _same_env(ref["e"], got["e"], ENV_KEYS, sl)
    _same_dicts(ref["cs"], got["cs"], CTRL_STATE[kind], sl)
    _same_dicts(ref["ps"], got["ps"], POLICY_STATE, sl)
    _same_dicts(ref["acc"], got["acc"], STATS, sl)
    _same_dicts(ref["es"], got["es"], EPISODE_STATS, sl)
    assert torch.equal(_bits(ref["term"][sl]), _bits(got["term"]))
    _same_dicts(ref["tr"], got["tr"], cols, sl)
    assert torch.equal(ref["nfev"][sl], got["nfev"])


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", KINDS)
def test_without_episode_ends_it_is_the_exact_rollout_bit_for_bit(kind):
    torch = _torch()
    n, K = 192, 60
    pol = feature_policy()
    a, c = _mk_gym(n, exact=True), _mk_gym(n, exact=True)
    sa, ta = _stats(a), a.new_trace(K)
    ca = ctrl_state(a, kind, "stock")
    nfa = torch.zeros(n, dtype=torch.int64, device=a.device)
    for k in (20, 40):
        _call(a, kind, "stock", False, k, pol, ca, None, stats=sa, trace=ta)
        nfa += a.nfev
    assert a.sync() == 0
    got = collector_run(kind, "stock", (20, 40), n=n, on_done="continue")
    b, tb = got["e"], got["tr"]
    _same_env(a, b, STATE_EXACT)
    _same_dicts(ca, got["cs"], CTRL_STATE[kind])
    _same_dicts(sa, got["acc"], STATS)
    _same_dicts(ta, tb, ("bg", "cgm", "cho", "insulin"))
    assert torch.equal(nfa, got["nfev"]) and int(nfa.min()) > 0
    assert float(tb["insulin"][1:].max()) > 0 and float(tb["cgm"].std()) > 0 and bool(torch.isfinite(tb["action"][1:]).all())
    # the reward and done of every step: what the env holds after each of K one-step roll-outs
    cc = ctrl_state(c, kind, "stock")
    for s in range(1, K + 1):
        _call(c, kind, "stock", False, 1, pol, cc, None)
        assert torch.equal(_bits(tb["reward"][s]), _bits(c.reward)), s
        assert torch.equal(tb["done"][s], c.done), s
    assert c.sync() == 0
    _same_env(a, c, STATE_EXACT)
    assert float(tb["reward"][1:].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("workload", ["hot", "high"])
@pytest.mark.parametrize("kind", KINDS)
def test_restart_is_the_loop_of_entry_points_bit_for_bit(kind, workload):
    """400 Dexcom steps in calls of 150 and 250, each cut into launches of 240 minutes, against the loop: under constants that
    end episodes low (basal-bolus: envs 128 .. 255 at 0.05 U/min beside 128 stock envs; PID: the "hot" gains) and under no
    insulin at all (episodes end high).  The entry points record no action: that column is checked in the test below."""
    ref = loop_run(kind, workload, 400)
    got = collector_run(kind, workload, (150, 250))
    r = ref["restarts"]
    print("\n[%s %s] envs restarted %d of %d, max restarts per env %d, endings < 70: %d, > 350: %d"
          % (kind, workload, (r > 0).sum(), len(r), r.max(), ref["low"], ref["high"]))
    # asserted on the reference loop, so that the comparison cannot pass on nothing
    if workload == "hot":
        assert (r > 0).sum() >= 13
        assert r.max() >= 2
    else:
        assert ref["high"] >= 1
    _same_run(ref, got, kind)


# ---------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("kind", KINDS)
def test_action_and_features_are_what_the_contract_says(kind):
    """On the hot run of the test above.  Action: the controller restated in torch fp64 elementwise operations, one rounding
    each as in dopri5_controller (no fused multiply-add on either side), on the observation and the controller state that
    every step of the loop found: bit for bit.  Features: row s is policy_features before step s of the loop (compared in the
    test above); a restarted env's next row shows its new first observation in every CGM entry."""
    torch = _torch()
    ref, got = loop_run(kind, "hot", 400), collector_run(kind, "hot", (150, 250))
    K, H = 400, 4
    tr, feat, done = got["tr"], got["tr"]["features"], ref["tr"]["done"]
    assert torch.equal(_bits(feat[1:]), _bits(ref["tr"]["features"][1:]))
    e, bf = ref["e"], ref["before"]
    cs0 = ctrl_state(e, kind, "hot")
    obs = bf["obs"][1:]
    st = torch.full_like(obs, float(ST))        # a tensor: torch divides by a Python number as a product with its reciprocal
    if kind == "bb":
        meal = bf["prev_meal"][1:]
        corr = torch.where(obs > 150.0, (obs - 140.0) / cs0["cf"], torch.zeros_like(obs))
        bolus = torch.where(meal > 0.0, ((meal * st) / cs0["cr"] + corr) / st, torch.zeros_like(obs))
        want = cs0["basal"] + bolus
        assert float((want - cs0["basal"]).max()) > 0                       # boluses were given
    else:
        P, I, D, target = PID["hot"]
        integ, prev = bf["integ"][1:], bf["prev"][1:]
        want = P * (obs - target) + I * integ + D * (obs - prev) / st
        assert float(integ.abs().max()) > 0 and float(prev.abs().max()) > 0
    assert torch.equal(_bits(tr["action"][1:]), _bits(want))
    assert float(tr["action"][1:].std()) > 0
    # a restarted env's next feature row: every CGM entry its new first observation, no insulin, no meal
    pol = feature_policy(H)
    rows = done[1:K].bool()                                                  # steps 1 .. K - 1: the next row is in the trace
    assert int(rows.sum()) > 0
    nxt = feat[2:K + 1]
    first = ((ref["first"][1:K] - pol.cgm_mean) * pol.cgm_scale).unsqueeze(1).expand(-1, H, -1)
    mask = rows.unsqueeze(1).expand(-1, H, -1)
    assert torch.equal(_bits(nxt[:, :H][mask]), _bits(first[mask]))
    assert bool((nxt[:, H:2 * H + 1][rows.unsqueeze(1).expand(-1, H + 1, -1)] == 0).all())


# ---------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("kind", KINDS)
def test_any_n_and_shards(kind):
    """70 envs -- a full wave and a partial one, which the network's kernels refuse -- give what envs 0 .. 69 of a batch of 128
    give; a shard of 128 envs at env_offset 128 is the upper half of the batch of 256."""
    big = collector_run(kind, "hot", (80, 120), n=128, hot_from=32)
    small = collector_run(kind, "hot", (200,), n=70, hot_from=32)
    assert int(small["tr"]["done"][1:].sum()) > 0
    _same_run(big, small, kind, slice(0, 70), cols=COLS)
    whole = collector_run(kind, "hot", (150, 250))
    shard = collector_run(kind, "hot", (400,), n=128, env_offset=128)
    assert int(shard["tr"]["done"][1:].sum()) > 0
    _same_run(whole, shard, kind, slice(128, 256), cols=COLS)


# ---------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("kind", KINDS)
def test_the_cut_into_launches_changes_nothing(kind):
    a = collector_run(kind, "hot", (150, 250))
    b = collector_run(kind, "hot", (150, 250), max_minutes_per_launch=30)
    _same_run(a, b, kind, cols=COLS)


# ---------------------------------------------------------------------------------------------------------- 6
def _stiff_rows():
    from oracle import t1d_oracle as O
    names, tab = O.patient_table()
    rows = tab[[names.index("adult#001"), names.index("adult#001")]].copy()
    rows[1, O.IDX["kabs"]] *= 1e6
    return rows


def test_solver_failure_inside_a_collection():
    """kabs x 1e6 for one env in three (test_gpu_collect_dopri5.py::test_solver_failure_inside_a_collection): the status bit, a
    finite state, and the normal envs as if the stiff ones were not there."""
    torch = _torch()
    from simglucose_amd import _lib
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    n, K = 192, 10
    pid = (np.arange(n) % 3 == 1).astype(np.int64)
    normal = np.where(pid == 0)[0]                                  # 128 envs, spread over all three waves
    rs = np.random.RandomState(9)
    z = rs.randn(21, n)
    mt = np.stack([np.full(n, 4), np.full(n, 17)]).astype(np.int64)
    ma = rs.uniform(30.0, 60.0, size=(2, n))
    pol = feature_policy()
    out = []
    for sel in (np.arange(n), normal):
        e = BatchedT1DSimEnv(patient=pid[sel], patient_table=_stiff_rows(), sensor="Dexcom", noise="host", normals=z[:, sel],
                             integrator="dopri5")
        e.set_meals(torch.as_tensor(mt[:, sel]), torch.as_tensor(ma[:, sel]))
        e.reset()
        tr = e.new_trace(K, columns=COLS, history=pol.history)
        e.collect_bb_dopri5(K, features=pol, trace=tr)
        out.append((e, tr, e.sync(raise_on_status=False)))
    (ea, tra, sta), (eb, trb, stb) = out
    assert sta & _lib.T1D_ST_SOLVER_FAILED and not (sta & _lib.T1D_ST_NONFINITE), sta
    assert stb == 0
    assert bool(torch.isfinite(ea.x).all()) and int(ea.t.min()) == K * ST == int(ea.t.max())
    nidx = torch.as_tensor(normal, device=ea.device)
    for k in COLS:
        assert torch.equal(_bits(tra[k][1:][..., nidx]), _bits(trb[k][1:])), k
    for k in ("x", "t", "cgm", "bg", "reward", "last_cgm", "prev_risk", "planned", "h_carry"):
        assert torch.equal(getattr(ea, k)[..., nidx], getattr(eb, k)), k
    assert bool((trb["cho"][1:] > 0).any()) and float(trb["action"][1:].max()) > float(trb["action"][1:].min())


def test_after_a_solver_failure_the_next_episode_integrates_again():
    """The stiff envs start low (subcutaneous glucose at 60 mg/dL) with a full stomach, which feeds the gut: their solver gives
    up in the first minute, the state stays, the first step ends the episode below 70 and the env restarts with an empty
    stomach, where the stiff rate has nothing to act on -- the new episode integrates until its first meal."""
    torch = _torch()
    from oracle import t1d_oracle as O
    from simglucose_amd import _lib
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    n, K = 128, 6
    rows = _stiff_rows()
    pid = (np.arange(n) % 3 == 1).astype(np.int64)
    e = BatchedT1DSimEnv(patient=pid, patient_table=rows, sensor="Dexcom", noise="philox", random_init_bg=True, seed=3,
                         integrator="dopri5")
    e.restart_done(mask=torch.ones(n, dtype=torch.uint8, device=e.device), days=DAYS, reset_outputs=True)
    stiff = torch.as_tensor(pid == 1, device=e.device)
    e.x[0, stiff] = 20000.0; e.x[1, stiff] = 20000.0                 # Qsto1, Qsto2 in mg
    e.x[12, stiff] = 60.0 * float(rows[1, O.IDX["Vg"]])               # Gsub: BG = 60 mg/dL
    pol = feature_policy()
    tr = e.new_trace(K, columns=COLS, history=pol.history)
    es = {k: torch.zeros(n, dtype=torch.int32 if "length" in k else e.dtype, device=e.device) for k in EPISODE_STATS}
    e.collect_bb_dopri5(K, features=pol, trace=tr, on_done="restart", days=DAYS, episode_stats=es)
    status = e.sync(raise_on_status=False)
    assert status & _lib.T1D_ST_SOLVER_FAILED and not (status & _lib.T1D_ST_NONFINITE), status
    assert bool(tr["done"][1][stiff].all()) and bool((tr["bg"][1][stiff] < 70).all())
    assert bool((e.episode[stiff] >= 2).all()) and bool((es["last_length"][stiff] >= 1).all())
    assert bool(torch.isfinite(e.x).all()) and bool(torch.isfinite(tr["bg"][1:]).all())
    # the new episode moves: a frozen state would repeat one BG word in every row
    once = stiff & (e.episode == 2) & (tr["cho"][2:].sum(dim=0) == 0)
    assert int(once.sum()) >= int(stiff.sum()) // 2
    moved = (tr["bg"][2:K + 1][:, once] != tr["bg"][2][once]).any(dim=0)
    assert bool(moved.all())
    assert bool((e.t[once] == (K - 1) * ST).all()) and bool((e.h_carry[once] > 0).all())
    assert bool((~tr["done"][1][~stiff].bool()).all())


# ---------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("history", [1, 12])
def test_the_shortest_and_the_longest_window(history):
    """H = 1 and H = 12 (a wave's piece of LDS is largest there, and the workgroup may shrink): 40 steps against the loop, every
    env at 0.05 U/min"""
    ref = loop_run("bb", "hot", 40, n=128, history=history, hot_from=0)
    got = collector_run("bb", "hot", (15, 25), n=128, history=history, hot_from=0)
    print("\n[H = %d] envs restarted %d of 128, endings %d" % (history, (ref["restarts"] > 0).sum(), ref["low"] + ref["high"]))
    assert (ref["restarts"] > 0).sum() >= 1
    _same_run(ref, got, "bb")
    assert bool(_torch().isfinite(got["tr"]["features"][1:]).all())
