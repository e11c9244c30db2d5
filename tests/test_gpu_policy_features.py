"""BatchedT1DSimEnv.policy_features on the GPU (t1d_mlp_features, csrc/t1d_policy.hpp): the features of the step that would
come next, pinned bit for bit to the row the next collect call records -- on a fresh state, after episodes ended and
restarted inside a launch, and in the exact mode; against the host restatement MLPController.features; the rejections; and
one whole actor-critic iteration (collect, critic, bootstrap, gae, PPO loss, backward) whose gradients repeat bit for bit.
The helpers are those of test_gpu_collect.py, copied."""
import ctypes as C
import math

import pytest

pytestmark = pytest.mark.gpu
N = 128
DAYS = 2
STATE = ("state", "istate", "ar_e", "cgm", "bg", "reward", "done", "lbgi", "hbgi", "risk", "meal", "insulin", "meal_time",
         "meal_amt", "start_minute", "episode")
POLICY_STATE = ("cgm_hist", "ins_hist", "prev_meal")


def _torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _mk_gym(n, dtype, seed=3, exact=False):
    """child#001 / adult#001 alternating, random initial glucose, Philox noise, every env in episode 0 of the device's own
    episode stream: the envs of test_gpu_collect.py"""
    torch = _torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    kw = dict(integrator="dopri5") if exact else dict(n_sub=4)
    e = BatchedT1DSimEnv(patient=["child#001", "adult#001"] * (n // 2), sensor="Dexcom", pump="Insulet", dtype=dtype,
                         seed=seed, noise="philox", random_init_bg=True, **kw)
    e.restart_done(mask=torch.ones(n, dtype=torch.uint8, device=e.device), days=DAYS, reset_outputs=True)
    return e


def _mk(n, dtype, seed=5):
    """all 30 patients, a random-meal day from 06:00, reset: the envs of test_gpu_policy.py"""
    torch = _torch()
    import numpy as np
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    from simglucose_amd.scenario_batch import random_meal_tables
    e = BatchedT1DSimEnv(patient=np.arange(n) % 30, sensor="Dexcom", dtype=dtype, seed=seed)
    e.start_minute = torch.full((n,), 360, dtype=torch.int32, device=e.device)
    e.set_meals(*random_meal_tables(n, days=1, start_minute_of_day=e.start_minute, seed=seed, dtype=dtype))
    e.reset()
    return e


def _policy(history=4, widths=(16, 16, 1), n_policies=1, seed=0, hidden="tanh", output="logistic", gain=1.0, **kw):
    torch = _torch()
    from simglucose_amd.controller.mlp_ctrller import MLPController
    g = torch.Generator().manual_seed(seed)
    layers, n_in = [], 2 * history + 3
    for w in widths:
        layers.append((gain * torch.randn(n_policies, w, n_in, generator=g, dtype=torch.float64) / math.sqrt(n_in),
                       gain * 0.1 * torch.randn(n_policies, w, generator=g, dtype=torch.float64)))
        n_in = w
    kw.setdefault("out_scale", 0.06)
    return MLPController(layers, history=history, hidden=hidden, output=output, **kw)


def _hypo_leaning_policy(history, seed=11):
    """small random weights around a constant 0.05 U/min: episodes end low (test_gpu_collect.py)"""
    return _policy(history=history, widths=(8, 1), seed=seed, output="identity", gain=0.02, out_scale=1.0, out_bias=0.05)


def _bits(t):
    torch = _torch()
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()]) if t.is_floating_point() else t


def _snapshot(e, st):
    snap = {k: getattr(e, k).clone() for k in STATE if getattr(e, k, None) is not None}    # an env without a gym loop has no episode counter
    snap.update({k: st[k].clone() for k in POLICY_STATE})
    return snap


def _unchanged(e, st, snap):
    torch = _torch()
    assert len(snap) >= 12 + len(POLICY_STATE)
    for k in STATE:
        if k in snap:
            assert torch.equal(_bits(getattr(e, k)), _bits(snap[k])), k
    for k in POLICY_STATE:
        assert torch.equal(_bits(st[k]), _bits(snap[k])), k


def _next_row(e, pol, st, exact=False, **kw):
    """the feature row the next collect call of one step records"""
    tr = e.new_trace(1, columns=("features",), history=pol.history)
    (e.collect_mlp_dopri5 if exact else e.collect_mlp)(1, pol, policy_state=st, trace=tr, **kw)
    return tr["features"][1]


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("H", [1, 4])
def test_fresh_state(H, dtype_name):
    torch = _torch()
    e = _mk(N, getattr(torch, dtype_name))
    pol = _policy(history=H, widths=(8, 1), seed=H)
    st = e.new_policy_state(pol)
    snap = _snapshot(e, st)
    f = e.policy_features(pol, st)
    assert f.shape == (2 * H + 3, N) and f.dtype == e.dtype and bool(torch.isfinite(f).all())
    _unchanged(e, st, snap)                                           # nothing written, no step taken
    assert torch.equal(_bits(f), _bits(_next_row(e, pol, st, sigma=0.2)))
    assert e.sync() == 0


# ---------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("H", [1, 4])
def test_after_restarts_inside_a_launch(H, dtype_name):
    """150 steps into a hypo-leaning run episodes end; six more steps with on_done="restart", in which at least one env
    starts a new episode: its start_minute, clock and windows are the new episode's."""
    torch = _torch()
    e = _mk_gym(N, getattr(torch, dtype_name))
    pol = _hypo_leaning_policy(H)
    kw = dict(sigma=0.3, explore_seed=99, on_done="restart", days=DAYS)
    st = e.collect_mlp(150, pol, **kw)
    ep0, start0 = e.episode.clone(), e.start_minute.clone()
    e.collect_mlp(6, pol, policy_state=st, **kw)
    restarted = e.episode != ep0
    print("\n[H=%d %s] %d of %d envs restarted in the six steps, %d with a new start hour"
          % (H, dtype_name, int(restarted.sum()), N, int((e.start_minute != start0).sum())))
    assert int(restarted.sum()) >= 1
    snap = _snapshot(e, st)
    f = e.policy_features(pol, st)
    _unchanged(e, st, snap)
    assert torch.equal(_bits(f), _bits(_next_row(e, pol, st, **kw)))
    assert e.sync() == 0


# ---------------------------------------------------------------------------------------------------------- 3
def test_exact_mode():
    torch = _torch()
    e = _mk_gym(N, torch.float64, exact=True)
    pol = _hypo_leaning_policy(4)
    kw = dict(sigma=0.3, explore_seed=99, on_done="restart", days=DAYS)
    st = e.new_policy_state(pol)
    f = e.policy_features(pol, st)
    tr = e.new_trace(3, columns=("features",), history=pol.history)
    e.collect_mlp_dopri5(3, pol, policy_state=st, trace=tr, **kw)
    assert torch.equal(_bits(f), _bits(tr["features"][1]))
    snap = _snapshot(e, st)
    h0 = e.h_carry.clone()
    f = e.policy_features(pol, st)
    _unchanged(e, st, snap)
    assert torch.equal(_bits(e.h_carry), _bits(h0))
    assert torch.equal(_bits(f), _bits(_next_row(e, pol, st, exact=True, **kw)))
    assert e.sync() == 0


# ---------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("H", [1, 4])
def test_against_the_host_restatement(H, dtype_name):
    """MLPController.features on the same windows: the window and meal features are the same two operations, equal; the
    time-of-day pair is the device's sinpi / cospi of m / 720 against torch's sin / cos in fp64, within 4 ulp of 1."""
    torch = _torch()
    e = _mk_gym(N, getattr(torch, dtype_name))
    pol = _policy(history=H, widths=(8, 1), seed=H)
    st = e.collect_mlp(7, pol, sigma=0.2)                             # windows, prev_meal and clock all away from reset
    f = e.policy_features(pol, st)
    cgm_hist = st["cgm_hist"].clone()
    cgm_hist[0] = e.cgm                                               # CGM[0] is the current observation
    minute = e.start_minute.long() + e.t.long()
    host = pol.features(cgm_hist, st["ins_hist"], st["prev_meal"], minute)
    assert torch.equal(_bits(f[:2 * H + 1]), _bits(host[:2 * H + 1]))
    assert float(f[H:2 * H].abs().max()) > 0                          # the insulin window has been filled
    host64 = pol.features(cgm_hist.double(), st["ins_hist"].double(), st["prev_meal"].double(), minute)
    err = float((f[2 * H + 1:].double() - host64[2 * H + 1:]).abs().max())
    ulp = torch.finfo(e.dtype).eps
    print("\n[H=%d %s] max |time-of-day feature - sin, cos| = %.2f ulp of 1" % (H, dtype_name, err / ulp))
    assert err <= 4 * ulp
    assert e.sync() == 0


# ---------------------------------------------------------------------------------------------------------- 5
def test_rejections():
    torch = _torch()
    from simglucose_amd import _lib
    e = _mk_gym(N, torch.float64)
    pol = _policy(history=3, widths=(8, 1))
    st = e.new_policy_state(pol)
    good = e.policy_features(pol, st)
    p, params = e._mlp_struct("policy_features", pol, st)
    e._set_trace(p, None, 0)
    L = e._L
    assert L.t1d_mlp_features(e._ctx, C.byref(e._b), C.byref(p), None, None) == -1
    assert L.t1d_last_error() == b"t1d_mlp_features: feat is NULL"
    out = torch.zeros_like(good)
    assert L.t1d_mlp_features(e._ctx, C.byref(e._b), None, C.c_void_p(out.data_ptr()), None) == -1
    assert L.t1d_mlp_features(None, C.byref(e._b), C.byref(p), C.c_void_p(out.data_ptr()), None) == -1
    p.history = 13
    assert L.t1d_mlp_features(e._ctx, C.byref(e._b), C.byref(p), C.c_void_p(out.data_ptr()), None) == -1
    assert b"t1d_mlp_features" in L.t1d_last_error()
    assert float(out.abs().max()) == 0.0
    for bad in (dict(cgm_hist=st["cgm_hist"][:2].contiguous()), dict(ins_hist=st["ins_hist"][:, :64].contiguous()),
                dict(prev_meal=st["prev_meal"].unsqueeze(0)), dict(cgm_hist=st["cgm_hist"].float())):
        with pytest.raises(ValueError):
            e.policy_features(pol, dict(st, **bad))
    with pytest.raises(ValueError):
        e.policy_features(_policy(history=3, widths=(8, 1), n_policies=4), st)       # 32 envs per policy
    assert torch.equal(_bits(e.policy_features(pol, st)), _bits(good))
    assert e.sync() == 0


# ---------------------------------------------------------------------------------------------------------- 6
def _iteration():
    """collect, critic, bootstrap, gae with moments, the clipped PPO loss with a value loss, backward -> the two gradients"""
    torch = _torch()
    from simglucose_amd.controller import gae, mlp_pre_output
    from simglucose_amd.controller.mlp_ctrller import MLPController
    K, sig, clip = 8, 0.3, 0.2
    e = _mk_gym(N, torch.float64)
    pol = _hypo_leaning_policy(4)
    vpol = _policy(history=4, widths=(8, 1), seed=5, output="identity", out_scale=1.0)
    st = e.collect_mlp(150, pol, sigma=sig, explore_seed=7, on_done="restart", days=DAYS)
    tr = e.new_trace(K, columns=("reward", "done", "eps", "features"), history=pol.history)
    e.collect_mlp(K, pol, sigma=sig, explore_seed=7, policy_state=st, trace=tr, on_done="restart", days=DAYS)
    f, eps = tr["features"][1:].contiguous(), tr["eps"][1:]
    old_params = pol.device_params(e.device, e.dtype)
    params = (old_params.clone() * 1.01).requires_grad_(True)          # one optimiser step away: the ratio is not 1
    vparams = vpol.device_params(e.device, e.dtype).clone().requires_grad_(True)
    y_old = mlp_pre_output(old_params, f, pol)
    z = y_old + sig * eps
    old_logp = MLPController.log_prob((z - y_old) / sig, sig)
    v = mlp_pre_output(vparams, f, vpol)                                                   # [K, n]
    v_last = mlp_pre_output(vparams, e.policy_features(vpol, st)[None], vpol)[0]           # the bootstrap at the cut
    adv, ret, mean, std = gae(tr["reward"][1:].contiguous(), tr["done"][1:].contiguous(), v.detach(), v_last.detach(),
                              gamma=0.99, lam=0.95, n_policies=1, moments=True)
    a = (adv - mean.repeat_interleave(N)) / (std.repeat_interleave(N) + 1e-8)
    y_new = mlp_pre_output(params, f, pol)
    ratio = (MLPController.log_prob((z - y_new) / sig, sig) - old_logp).exp()
    loss = -torch.minimum(ratio * a, ratio.clamp(1 - clip, 1 + clip) * a).mean() + 0.5 * ((v - ret) ** 2).mean()
    loss.backward()
    assert e.sync() == 0
    return params.grad.clone(), vparams.grad.clone(), int(tr["done"][1:].sum())


def test_one_actor_critic_iteration_end_to_end():
    torch = _torch()
    g1, v1, n_done = _iteration()
    for g in (g1, v1):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    g2, v2, _ = _iteration()
    assert torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(v1), _bits(v2))
    print("\n[actor-critic] %d episode ends in the 8 x 128 samples; |grad| max %.3e (actor), %.3e (critic)"
          % (n_done, float(g1.abs().max()), float(v1.abs().max())))
