"""The controllers' collectors on the GPU (BatchedT1DSimEnv.collect_pid / collect_bb -> t1d_collect_pid / t1d_collect_bb,
ctrl_collect_kernel of csrc/t1d_policy.hpp): pinned bit for bit to rollout_pid / rollout_bb (no episode ends) and to the loop of
entry points the header names (episodes that end); the recorded features and action against the contract; shards, window
lengths, a batch that is no multiple of 64; and the warm start the calls are for.  The runs come from support_ctrl.py, each made
once and shared."""
import pytest

from support import (DAYS, EPISODE_STATS, POLICY_STATE, STATE, STATS, bits as _bits, gpu_torch as _torch, gym_env as _mk_gym,
                     same_dicts as _same_dicts, same_env as _same_env, stats as _stats)
from support_ctrl import COLS, CTRL_STATE, PID, _call, collector_run, ctrl_state, feature_policy, loop_run

pytestmark = pytest.mark.gpu
ENV_KEYS = STATE + ("meal_time", "meal_amt", "start_minute", "episode", "cgm0")
LOOP_COLS = tuple(c for c in COLS if c != "action")
KINDS = ["pid", "bb"]
DTYPES = ["float64", "float32"]


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


def _ulp(x):
    """the spacing of the floating-point numbers at |x| (of the smallest normal number below it)"""
    torch = _torch()
    fi = torch.finfo(x.dtype)
    ax = x.abs().clamp_min(fi.tiny)
    return torch.nextafter(ax, torch.full_like(ax, float("inf"))) - ax


def _action_by_hand(kind, workload, cs0, obs, meal, integ, prev, st=3.0):
    """basal + bolus of one step in torch, written as the controllers of the reference write it -> (action, the magnitude
    its rounding is measured against: the sum of the absolute values of the terms)"""
    torch = _torch()
    if kind == "bb":
        corr = torch.where(obs > 150, (obs - 140.0) / cs0["cf"], torch.zeros_like(obs))
        bolus = torch.where(meal > 0, ((meal * st) / cs0["cr"] + corr) / st, torch.zeros_like(obs))
        return cs0["basal"] + bolus, cs0["basal"].abs() + bolus.abs()
    P, I, D, target = PID[workload]
    terms = (P * (obs - target), I * integ, D * (obs - prev) / st)
    return terms[0] + terms[1] + terms[2], terms[0].abs() + terms[1].abs() + terms[2].abs()


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_without_episode_ends_it_is_the_rollout_bit_for_bit(dtype_name, kind):
    torch = _torch()
    dtype = getattr(torch, dtype_name)
    n, K = 256, 60
    pol = feature_policy()
    a, c = _mk_gym(n, dtype), _mk_gym(n, dtype)
    sa, ta = _stats(a), a.new_trace(K)
    ca = ctrl_state(a, kind, "stock")
    _call(a, kind, "stock", False, K, pol, ca, None, stats=sa, trace=ta)
    assert a.sync() == 0
    got = collector_run(kind, "stock", dtype_name, (20, 40), on_done="continue")
    b, tb = got["e"], got["tr"]
    _same_env(a, b)
    _same_dicts(ca, got["cs"], CTRL_STATE[kind])
    _same_dicts(sa, got["acc"], STATS)
    _same_dicts(ta, tb, ("bg", "cgm", "cho", "insulin"))
    assert float(tb["insulin"][1:].max()) > 0 and float(tb["cgm"].std()) > 0 and bool(torch.isfinite(tb["action"][1:]).all())
    # the reward and done of every step: what the env holds after each of K one-step roll-outs
    cc = ctrl_state(c, kind, "stock")
    for s in range(1, K + 1):
        _call(c, kind, "stock", False, 1, pol, cc, None)
        assert torch.equal(_bits(tb["reward"][s]), _bits(c.reward)), s
        assert torch.equal(tb["done"][s], c.done), s
    assert c.sync() == 0
    _same_env(a, c)
    assert float(tb["reward"][1:].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_restart_is_the_loop_of_entry_points_bit_for_bit(dtype_name, kind):
    """400 Dexcom steps in launches of 150 and 250 against the loop, under constants that end episodes low (basal-bolus: envs
    128 .. 255 at 0.05 U/min beside 128 stock envs; PID: the "hot" gains) and under no insulin at all (episodes end high).  The
    entry points record no action: that column is checked against the contract in the test below."""
    out = {}
    for workload, cuts in (("hot", (150, 250)), ("high", (400,))):
        ref = loop_run(kind, workload, dtype_name, 400)
        got = collector_run(kind, workload, dtype_name, cuts)
        _same_run(ref, got, kind)
        out[workload] = ref
    hot = out["hot"]["restarts"][128:] if kind == "bb" else out["hot"]["restarts"]
    print("\n[%s %s] hot envs restarted %d of %d, max restarts per env %d / %d, endings < 70: %d / %d, > 350: %d / %d"
          % (kind, dtype_name, (hot > 0).sum(), len(hot), hot.max(), out["high"]["restarts"].max(), out["hot"]["low"],
             out["high"]["low"], out["hot"]["high"], out["high"]["high"]))
    # asserted on the reference loop, so that the comparison cannot pass on nothing
    assert (hot > 0).sum() >= 0.05 * len(hot)
    assert hot.max() >= 2
    assert out["hot"]["high"] + out["high"]["high"] >= 1


# ---------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_features_and_action_are_what_the_contract_says(dtype_name, kind):
    """On the hot run of the test above.  Features: row s is policy_features before step s of the loop (bit for bit, in the test
    above) and the host's MLPController.features of the loop's windows: entries 0 .. 2 H bit for bit, the time-of-day pair within
    1e-14 / 2e-6 of sin and cos (the bounds of test_action_and_features_are_what_the_contract_says in test_gpu_collect.py).
    Action: basal + bolus from the observation, the meal and the controller state of the step before, in torch.  The kernel's
    expression may be contracted into fused multiply-adds where torch rounds every product, so a word may differ by the rounding
    of one intermediate: 2 ulp of the sum of the terms' magnitudes (an intermediate is no larger, one rounding is half an ulp of
    it; the sum itself may be smaller where the terms cancel).  Measured on an MI355X: at most 1 ulp of the action itself in both
    dtypes and under both controllers, which reads as 2.00 where the terms' sum lies in the binade below the action's."""
    torch = _torch()
    ref, got = loop_run(kind, "hot", dtype_name, 400), collector_run(kind, "hot", dtype_name, (150, 250))
    K, H = 400, 4
    tr, feat, done = got["tr"], got["tr"]["features"], ref["tr"]["done"]
    assert torch.equal(_bits(feat[1:, :2 * H + 1]), _bits(ref["host_feat"][1:, :2 * H + 1]))
    worst_tod = float((feat[1:, 2 * H + 1:].double() - ref["host_feat"][1:, 2 * H + 1:].double()).abs().max())
    assert worst_tod <= (1e-14 if dtype_name == "float64" else 2e-6)
    # the action of every step, from what the loop's step found: the observation (cgm[s - 1], or the new episode's first one),
    # the meal (cho[s - 1], 0 after a restart) and the loop's own integ / prev words
    e, bf = ref["e"], ref["before"]
    cs0 = ctrl_state(e, kind, "hot")
    cont = ~done[1:K].bool()                                                 # step s + 1 follows step s of the same episode
    assert torch.equal(_bits(bf["obs"][2:K + 1][cont]), _bits(ref["tr"]["cgm"][1:K][cont]))
    if kind == "bb":
        assert torch.equal(_bits(bf["prev_meal"][2:K + 1][cont]), _bits(ref["tr"]["cho"][1:K][cont]))
        assert bool((bf["prev_meal"][2:K + 1][~cont] == 0).all())
    z = torch.zeros_like(bf["obs"][1:])
    want, size = _action_by_hand(kind, "hot", cs0, bf["obs"][1:], bf["prev_meal"][1:] if kind == "bb" else z,
                                 bf["integ"][1:] if kind == "pid" else z, bf["prev"][1:] if kind == "pid" else z)
    err = (tr["action"][1:] - want).abs() / _ulp(size)
    worst = float(err.max())
    print("\n[%s %s] max |action - by hand| = %.2f ulp of the terms, max |time-of-day feature - host| = %.3e"
          % (kind, dtype_name, worst, worst_tod))
    assert worst <= 2.0
    assert float(tr["action"][1:].std()) > 0
    if kind == "bb":
        assert float((tr["action"][1:] - cs0["basal"]).max()) > 0           # boluses were given
    # a restarted env's next feature row: every CGM entry its new first observation, no insulin, no meal
    pol = feature_policy(H)
    rows = done[1:K].bool()                                                  # steps 1 .. K - 1: the next row is in the trace
    assert int(rows.sum()) > 0
    nxt = feat[2:K + 1]
    first = ((ref["first"][1:K] - pol.cgm_mean) * pol.cgm_scale).unsqueeze(1).expand(-1, H, -1)
    mask = rows.unsqueeze(1).expand(-1, H, -1)
    assert torch.equal(_bits(nxt[:, :H][mask]), _bits(first[mask]))
    assert bool((nxt[:, H:2 * H + 1][rows.unsqueeze(1).expand(-1, H + 1, -1)] == 0).all())
    # ... and of an env that finished in the last step, in the windows the call hands back
    last = done[K].bool()
    assert torch.equal(_bits(got["ps"]["cgm_hist"][:, last]), _bits(got["e"].cgm[last].unsqueeze(0).expand(H, -1)))
    assert bool((got["ps"]["ins_hist"][:, last] == 0).all()) and bool((got["ps"]["prev_meal"][last] == 0).all())


# ---------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("kind", KINDS)
def test_shards_are_slices_of_the_big_batch_with_restarts_on(kind):
    big = collector_run(kind, "hot", "float64", (150, 250))
    assert int(big["tr"]["done"][1:].sum()) > 0
    for a, cuts in ((0, (400,)), (128, (90, 310))):
        part = collector_run(kind, "hot", "float64", cuts, n=128, env_offset=a)
        _same_run(big, part, kind, slice(a, a + 128), cols=COLS)


# ---------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("history", [1, 12])
def test_window_lengths_and_a_batch_that_is_no_multiple_of_64(history):
    """H = 1 and 12 at 128 envs (the upper 96 hot) against the loop; then 70 envs -- a full wave and a partial one, which the
    network's kernels would refuse -- against the first 70 envs of that loop: an env depends on nothing but itself."""
    K = 200
    ref = loop_run("bb", "hot", "float64", K, n=128, history=history, hot_from=32)
    assert (ref["restarts"] > 0).sum() >= 1
    got = collector_run("bb", "hot", "float64", (77, 123), n=128, history=history, hot_from=32)
    _same_run(ref, got, "bb")
    small = collector_run("bb", "hot", "float64", (123, 77), n=70, history=history, hot_from=32)
    assert (ref["restarts"][:70] > 0).sum() >= 1
    _same_run(ref, small, "bb", slice(0, 70))
    _same_dicts(got["tr"], small["tr"], ("action",), slice(0, 70))


def test_pid_on_a_batch_that_is_no_multiple_of_64():
    ref = loop_run("pid", "hot", "float32", 400)
    small = collector_run("pid", "hot", "float32", (400,), n=70)
    _same_run(ref, small, "pid", slice(0, 70))


# ---------------------------------------------------------------------------------------------------------- 6
def test_warm_start_fits_a_network_to_the_basal_bolus_controller():
    """32 steps of collect_bb, 30 Adam steps of the fused value loss on (features, action), then the fitted network drives the
    envs through collect_mlp."""
    torch = _torch()
    from simglucose_amd.controller import value_loss
    from simglucose_amd.controller.mlp_ctrller import MLPController
    n, K = 128, 32
    e = _mk_gym(n, torch.float64)
    pol = feature_policy()
    tr = e.new_trace(K, columns=("action", "features"), history=pol.history)
    _, ps = e.collect_bb(K, features=pol, trace=tr, on_done="restart", days=DAYS)
    feat, target = tr["features"][1:], tr["action"][1:]
    assert bool(torch.isfinite(feat).all()) and bool(torch.isfinite(target).all()) and float(target.min()) > 0
    params = pol.flat_params().to(e.device).requires_grad_(True)
    opt = torch.optim.Adam([params], lr=1e-2)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = value_loss(params, feat, pol, target=target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("\nbehaviour cloning: loss %.3e -> %.3e" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0]
    fitted = MLPController.from_flat(params.detach().cpu(), pol.widths, history=pol.history, hidden=pol.hidden, output="identity")
    e.collect_mlp(K, fitted, policy_state=ps, on_done="restart", days=DAYS)
    assert e.sync() == 0


# ---------------------------------------------------------------------------------------------------------- 7
def test_rejections_change_nothing_and_exact_mode_envs_are_turned_away():
    torch = _torch()
    import ctypes as C
    from simglucose_amd import _lib
    e = _mk_gym(128, torch.float64)
    pol = feature_policy()
    ps, bb = e.new_policy_state(pol), ctrl_state(e, "bb", "stock")
    before = {k: getattr(e, k).clone() for k in ENV_KEYS}
    before.update({k: v.clone() for k, v in ps.items()})
    extra = torch.zeros(e.n, dtype=e.dtype, device=e.device)
    with pytest.raises(ValueError, match="n_steps"):
        e.collect_bb(0, features=pol, bb_state=bb, policy_state=ps)
    with pytest.raises(ValueError, match="features"):
        e.collect_pid(4, 1e-4, 0.0, 0.0)
    with pytest.raises(ValueError, match="eps"):
        e.collect_bb(4, features=pol, bb_state=bb, policy_state=ps, trace={"row": 0, "eps": extra.repeat(4, 1)})
    with pytest.raises(ValueError, match="on_done"):
        e.collect_bb(4, features=pol, bb_state=bb, policy_state=ps, on_done="stop")
    # through the C ABI, on a batch that is otherwise in order: exploration noise, and a policy window of another length
    p = _lib.Bb()
    p.target = 140.0
    for k in ("basal", "cr", "cf", "prev_meal"):
        setattr(p, k, bb[k].data_ptr())
    f = _lib.Mlp()
    f.history = pol.history
    for k in ("cgm_hist", "ins_hist", "prev_meal"):
        setattr(f, k, ps[k].data_ptr())
    g = _lib.Collect()
    e._b.cho = None

    def call():
        return e._L.t1d_collect_bb(e._ctx, C.byref(e._b), C.byref(p), C.byref(f), C.byref(g), 4, e.minutes_per_step, e.n_sub, e._stream())
    g.sigma = extra.data_ptr()
    assert call() == -1 and b"sigma" in e._L.t1d_last_error()
    g.sigma, g.eps_trace = None, extra.data_ptr()
    assert call() == -1 and b"eps_trace" in e._L.t1d_last_error()
    g.eps_trace, f.history = None, 13
    assert call() == -1 and b"history" in e._L.t1d_last_error()
    f.history = pol.history
    assert e.sync() == 0
    for k, v in before.items():
        assert torch.equal(_bits(v), _bits(ps[k] if k in ps else getattr(e, k))), k
    assert call() == 0 and e.sync() == 0                         # the same structs, nothing in the way: the call runs
    assert not torch.equal(before["state"], e.state)
    # an env in the exact mode has no such collector
    x = _mk_gym(128, torch.float64, exact=True)
    with pytest.raises(_lib.T1DError, match="dopri5"):
        x.collect_bb(4, features=pol)
    with pytest.raises(_lib.T1DError, match="dopri5"):
        x.collect_pid(4, 1e-4, 0.0, 0.0, features=pol)
