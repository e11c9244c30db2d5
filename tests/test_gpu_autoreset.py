"""GPU tests of the device-side episode restart (t1d_restart_done, BatchedT1DSimEnv.restart_done,
BatchedGymT1DSimEnv(auto_reset="device")).  The reference throughout is what existed before it: t1d_random_meals, t1d_reset
and the Python start-hour formula, composed on the host."""
import numpy as np
import pytest

from support import DAYS

pytestmark = pytest.mark.gpu

OUT8 = ("reward", "done", "bg", "lbgi", "hbgi", "risk", "meal", "insulin")


def _names(n):
    return ["child#001", "adult#001"] * (n // 2)


def _mk(n, dtype, seed=3, env_offset=0, names=None, integrator=None):
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    return BatchedT1DSimEnv(patient=names or _names(n), sensor="Dexcom", pump="Insulet", dtype=dtype, n_sub=4, seed=seed,
                            env_offset=env_offset, noise="philox", random_init_bg=True, integrator=integrator)


def _host_restart(e, mask, keep_outputs):
    """the composition of the existing entry points: for the envs of `mask`, the start hour by the Python formula, the meal
    table column from t1d_random_meals (one call per distinct episode index, columns copied in place), then reset(mask)."""
    import torch
    from simglucose_amd import scenario_batch
    from simglucose_amd.envs.batched_gym_env import start_hours
    mask = mask.bool()
    gid = torch.arange(e.n, dtype=torch.int64, device=e.device) + e.env_offset
    idx = e.episode.long()                                           # the episode index: the counter before the reset
    hours = start_hours(e.seed, idx, gid)
    for k in torch.unique(idx[mask]).tolist():
        mt, ma = scenario_batch.random_meal_tables(e.n, days=DAYS, start_minute_of_day=hours * 60, seed=e.seed * 7919 + k,
                                                   device=e.device, dtype=e.dtype, env_offset=e.env_offset)
        sel = (mask & (idx == k)).unsqueeze(0)
        e.meal_time.copy_(torch.where(sel, mt, e.meal_time))
        e.meal_amt.copy_(torch.where(sel, ma, e.meal_amt))
    saved = {k: getattr(e, k).clone() for k in OUT8}
    e.reset(mask=mask)
    if keep_outputs:
        for k in OUT8:
            getattr(e, k).copy_(saved[k])
    return hours


def _run_pair(n, dtype, basal, steps, integrator=None):
    """batch A restarts on the device, batch B through the host composition; equal bit for bit after every step.
    -> what happened in B: restarts per env, low endings, high endings"""
    import torch
    A, B = _mk(n, dtype, integrator=integrator), _mk(n, dtype, integrator=integrator)
    rows = 6 * (DAYS + 1)
    B.set_meals(torch.full((rows, n), 0x7FFFFFFF, dtype=torch.int32, device=B.device), torch.zeros(rows, n, dtype=dtype, device=B.device))
    ones = torch.ones(n, dtype=torch.uint8, device=A.device)
    term = torch.zeros(n, dtype=dtype, device=A.device)
    A.restart_done(mask=ones, days=DAYS, reset_outputs=True)
    hours = _host_restart(B, ones, keep_outputs=False)
    assert torch.equal(A.start_minute.long(), hours * 60)

    def same(step):
        keys = ("state", "istate", "ar_e", "meal_time", "meal_amt", "cgm", "cgm0", "reward", "done") + \
            (("h_carry",) if integrator else ())
        for k in keys:
            assert torch.equal(getattr(A, k), getattr(B, k)), (k, step)
    same(-1)
    a = torch.full((n,), basal, dtype=dtype, device=A.device)
    low = high = 0
    for s in range(steps):
        A.step(a); B.step(a)
        done = B.done.bool()
        b_term = B.cgm.clone()
        low += int((done & (B.bg < 70)).sum()); high += int((done & (B.bg > 350)).sum())
        A.restart_done(days=DAYS, terminal_obs=term)
        if bool(done.any()):
            _host_restart(B, done, keep_outputs=True)
        same(s)
        assert torch.equal(term[done], b_term[done]), s
    assert A.sync() == 0 and B.sync() == 0
    return (B.episode - 1).cpu().numpy(), low, high


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_restart_equals_host_composition_bit_for_bit(dtype_name):
    """The hypo workload of test_batched_gym_env_device_mode_and_auto_reset (4 096 envs, child#001 / adult#001, basal
    0.05 U/min, Dexcom) over 400 steps, and a run without insulin for the high side."""
    import torch
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    n = 4096
    restarts_lo, low_lo, high_lo = _run_pair(n, dtype, 0.05, 400)
    restarts_hi, low_hi, high_hi = _run_pair(n, dtype, 0.0, 400)
    print("restarted envs: %d / %d of %d, max restarts per env %d / %d, endings < 70: %d / %d, > 350: %d / %d"
          % ((restarts_lo > 0).sum(), (restarts_hi > 0).sum(), n, restarts_lo.max(), restarts_hi.max(), low_lo, low_hi, high_lo, high_hi))
    # so that the comparison cannot pass on nothing (asserted on the reference composition, batch B)
    assert ((restarts_lo > 0) | (restarts_hi > 0)).sum() >= 0.05 * n
    assert max(restarts_lo.max(), restarts_hi.max()) >= 2
    assert low_lo + low_hi > 0 and high_lo + high_hi > 0


def test_restart_equals_host_composition_with_dopri5():
    import torch
    restarts, low, high = _run_pair(256, torch.float64, 0.05, 400, integrator="dopri5")
    print("dopri5: restarted envs %d of 256, max restarts per env %d" % ((restarts > 0).sum(), restarts.max()))
    assert (restarts > 0).sum() >= 0.05 * 256 and low > 0


def test_restarts_do_not_depend_on_neighbours_or_sharding():
    """two shards = the slices of the whole batch through every restart; and an env's later episodes are the same when
    other envs of the batch finish at other times (their basal differs)"""
    import torch
    n, h = 4096, 2048
    names = _names(n)
    W = _mk(n, torch.float64)
    S = [_mk(h, torch.float64, env_offset=0, names=names[:h]), _mk(h, torch.float64, env_offset=h, names=names[h:])]
    V = _mk(n, torch.float64)                       # every other PAIR of envs gets another basal: other neighbours finish
    ones = torch.ones(n, dtype=torch.uint8, device=W.device)
    a = torch.full((n,), 0.05, dtype=torch.float64, device=W.device)
    pair = (torch.arange(n, device=W.device) // 2) % 2 == 0
    av = torch.where(pair, a, torch.full_like(a, 0.02))
    for e in [W, V] + S:
        e.restart_done(mask=ones[:e.n], days=DAYS, reset_outputs=True)
    keys = ("state", "istate", "ar_e", "meal_time", "meal_amt", "cgm", "cgm0", "start_minute")
    for s in range(400):
        W.step(a); V.step(av)
        for k, e in enumerate(S):
            e.step(a[k * h:(k + 1) * h])
        for e in [W, V] + S:
            e.restart_done(days=DAYS)
        if s % 10 == 9 or s == 0:
            for key in keys:
                w = getattr(W, key)
                assert torch.equal(w[..., :h], getattr(S[0], key)) and torch.equal(w[..., h:], getattr(S[1], key)), (key, s)
                assert torch.equal(w[..., pair], getattr(V, key)[..., pair]), (key, s)
    assert int(W.episode[h:].max()) >= 3 and int(W.episode[:h].max()) >= 3     # second episodes happened in both shards
    assert int(W.episode[pair].max()) >= 3
    assert not torch.equal(W.episode[~pair], V.episode[~pair])                   # the neighbours did finish differently
    for e in [W, V] + S:
        assert e.sync() == 0


def test_device_mode_full_reset_is_episode_zero_of_the_present_wrapper():
    import torch
    from simglucose_amd.envs import BatchedGymT1DSimEnv
    n = 4096
    for dtype in (torch.float64, torch.float32):
        new = BatchedGymT1DSimEnv(n, patient_name=_names(n), seed=3, auto_reset="device", dtype=dtype, env_offset=640)
        old = BatchedGymT1DSimEnv(n, patient_name=_names(n), seed=3, auto_reset=True, dtype=dtype, env_offset=640)
        o_new, o_old = new.reset(), old.reset()
        assert torch.equal(o_new, o_old)
        for k in ("state", "istate", "ar_e", "meal_time", "meal_amt", "cgm0", "bg", "reward", "done"):
            assert torch.equal(getattr(new.env, k), getattr(old.env, k)), k
        assert torch.equal(new.start_hour, old.start_hour) and torch.equal(new.time(), old.time())
        assert int(new.start_hour.min()) == 0 and int(new.start_hour.max()) == 23
        assert new.env.sync() == 0


def test_statistics_of_restarted_episodes():
    """start hours, initial glucose and meal tables of the episodes the device starts, over a 65 536-env run"""
    import torch
    from simglucose_amd import params
    from simglucose_amd.envs import BatchedGymT1DSimEnv
    from oracle import t1d_oracle as O
    n = 65536
    env = BatchedGymT1DSimEnv(n, patient_name=_names(n), seed=5, auto_reset="device", horizon_days=DAYS)
    env.reset()
    names, tab = params.patient_table()
    vg = torch.as_tensor(tab[env.env.patient_idx, 19], device=env.env.device)          # T1D_P_VG
    a = torch.full((n,), 0.05, dtype=torch.float64, device=env.env.device)
    bg_at_restart = torch.full((n,), float("nan"), dtype=torch.float64, device=env.env.device)
    for _ in range(300):
        obs, rew, done, info = env.step(a)
        bg_at_restart = torch.where(done, env.env.x[12] / vg, bg_at_restart)
    restarted = (env.env.episode > 1)
    assert torch.equal(restarted, ~torch.isnan(bg_at_restart))
    m = int(restarted.sum())
    adult = restarted.clone(); adult[0::2] = False
    print("restarted %d of %d envs, %d of them adult#001" % (m, n, int(adult.sum())))
    assert m >= 2000 and int(adult.sum()) >= 500                      # enough for the bounds below to mean something
    hours = env.start_hour[restarted]
    assert int(torch.bincount(hours, minlength=24).min()) > 0 and int(hours.min()) == 0 and int(hours.max()) == 23
    assert torch.equal(env.env.start_minute[restarted].long(), hours * 60)
    sd = float(bg_at_restart[adult].std())
    print("adult#001 BG at restart: mean %.2f sd %.3f" % (float(bg_at_restart[adult].mean()), sd))
    assert 2.3 < sd < 3.1                            # random_init_bg: sd = sqrt(0.1 x0_13) / Vg = 2.69 mg/dL around 138.56
    assert abs(float(bg_at_restart[adult].mean()) - 138.56) < 5 * 2.69 / np.sqrt(int(adult.sum())) + 0.01
    # meal tables of the restarted envs: structure as t1d_random_meals leaves it, meals per day as the reference generator
    t = env.env.meal_time[:, restarted].cpu().numpy().astype(np.int64)
    amt = env.env.meal_amt[:, restarted].cpu().numpy()
    st = env.env.start_minute[restarted].cpu().numpy().astype(np.int64)
    used = t != 0x7FFFFFFF
    assert t.shape[0] == 6 * (DAYS + 1)
    assert np.all(np.diff(t, axis=0)[used[1:]] > 0) and np.all(used[:-1] | ~used[1:])
    assert t[used].min() >= 0 and t[used].max() < DAYS * 1440
    tod = (t + st[None, :]) % 1440
    assert tod[used].min() >= 5 * 60 and tod[used].max() <= 23 * 60
    assert np.all(amt[~used] == 0) and np.all(amt[used] >= 0) and np.all(amt[used] == np.round(amt[used]))
    rs = np.random.RandomState(123)
    ref_days = 6000
    ref = sum(len(O.random_scenario_draw(rs)[0]) for _ in range(ref_days))
    # 3.75 meals a day is an upper bound of the variance of a day's count; both samples contribute
    assert abs(used.sum() / (m * DAYS) - ref / ref_days) < 5 * np.sqrt(3.75 / ref_days + 3.75 / (m * DAYS))
    assert env.env.sync() == 0


def test_gym_contract_of_device_mode():
    import torch
    from simglucose_amd.envs import BatchedGymT1DSimEnv
    n = 4096
    env = BatchedGymT1DSimEnv(n, patient_name=_names(n), seed=3, auto_reset="device")
    obs = env.reset()
    dev = env.env.device
    a = torch.full((n,), 0.05, dtype=torch.float64, device=dev)
    ret = torch.zeros(n, dtype=torch.float64, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    last_ret = torch.zeros_like(ret); last_len = torch.zeros_like(length)
    episode0 = env.env.episode.clone()
    n_done = 0
    for s in range(300):
        obs, rew, done, info = env.step(a)
        assert done.dtype == torch.bool
        ret = ret + rew; length = length + 1
        bg = info["bg"]
        assert torch.equal(done, (bg < 70) | (bg > 350))              # done and reward are the terminal step's
        assert torch.equal(rew, env.env.reward) and bool(torch.isfinite(rew).all())
        last_ret = torch.where(done, ret, last_ret); last_len = torch.where(done, length, last_len)
        ret = torch.where(done, torch.zeros_like(ret), ret); length = torch.where(done, torch.zeros_like(length), length)
        # the clock: a restarted env is at t = 0, the others where their episode's steps took them
        assert torch.equal(env.env.t.long(), length * 3)
        assert torch.equal(info["episode"]["l"].long(), last_len)     # = t / sample_time the finished episode had reached
        assert torch.equal(info["episode"]["r"], last_ret)            # fp64, summed in the same order: exact
        assert torch.equal(env.episode_stats["ep_return"], ret) and torch.equal(env.episode_stats["ep_length"].long(), length)
        # where done: obs is the new episode's first observation (CGM sample #1 of the reset), the terminal one is in info
        assert torch.equal(obs, env.env.cgm)
        assert torch.equal(env.env.last_cgm[done], obs[done])
        n_done += int(done.sum())
        if bool(done.any()):
            term = info["terminal_observation"]
            assert bool(((term[done] >= 39) & (term[done] <= 600)).all())
    assert n_done > 0
    assert torch.equal((env.env.episode - episode0).long().sum(), torch.tensor(n_done, device=dev))
    assert env.env.sync() == 0


def test_device_mode_with_dopri5_and_custom_reward_runs_and_resets_the_ring():
    import torch
    from simglucose_amd.envs import BatchedGymT1DSimEnv
    n = 256
    f = lambda w: -torch.nan_to_num(w[-1] - 112.5, nan=0.0).abs()
    env = BatchedGymT1DSimEnv(n, patient_name=_names(n), seed=3, auto_reset="device", integrator="dopri5", reward_fun=f)
    env.reset()
    a = torch.full((n,), 0.05, dtype=torch.float64, device=env.env.device)
    total = 0
    for s in range(200):
        obs, rew, done, info = env.step(a)
        # the custom reward saw the finished step's observation, which a restarted env hands out as terminal_observation
        assert torch.equal(rew, -(torch.where(done, info["terminal_observation"], obs) - 112.5).abs())
        w = env.env.cgm_window()
        if bool(done.any()):
            # CGM_hist of a restarted env = [sample #0] only
            assert bool(torch.isnan(w[:-1, done]).all()) and torch.equal(w[-1, done], env.env.cgm0[done])
            assert bool((env.env.h_carry[done] == 0).all())
        total += int(done.sum())
    assert total > 0 and env.env.sync() == 0


def _twenty_steps(env, a):
    ptrs = None
    for s in range(20):
        obs, rew, done, info = env.step(a)
        p = (obs.data_ptr(), rew.data_ptr(), done.data_ptr(), info["terminal_observation"].data_ptr(),
             info["episode"]["r"].data_ptr(), info["episode"]["l"].data_ptr(), info["bg"].data_ptr())
        assert ptrs is None or p == ptrs, s
        ptrs = p


def test_device_mode_buffers_keep_their_addresses():
    import torch
    from simglucose_amd.envs import BatchedGymT1DSimEnv
    n = 4096
    env = BatchedGymT1DSimEnv(n, patient_name=_names(n), seed=3, auto_reset="device")
    env.reset()
    _twenty_steps(env, torch.full((n,), 0.05, dtype=torch.float64, device=env.env.device))
    assert env.env.sync() == 0


def test_device_mode_steps_without_a_host_round_trip():
    """twenty steps under torch's sync debug mode 'error': nothing in step() waits for the device"""
    import torch
    from simglucose_amd.envs import BatchedGymT1DSimEnv
    n = 4096
    env = BatchedGymT1DSimEnv(n, patient_name=_names(n), seed=3, auto_reset="device")
    env.reset()
    a = torch.full((n,), 0.05, dtype=torch.float64, device=env.env.device)
    for _ in range(150):                              # far enough for episodes to end inside the twenty steps
        env.step(a)
    before = env.env.episode.clone()
    probe = torch.ones(1, device=env.env.device)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            supported = False
        except RuntimeError:
            supported = True
        if supported:
            _twenty_steps(env, a)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not supported:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a synchronising call in this torch build on ROCm")
    assert int((env.env.episode - before).sum()) > 0          # episodes did restart inside the window
    assert env.env.sync() == 0
