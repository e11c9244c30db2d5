"""BatchedT1DSimEnv.policy_features on the GPU (t1d_mlp_features, csrc/t1d_policy.hpp): the features of the step that would
come next, pinned bit for bit to the row the next collect call records -- on a fresh state, after episodes ended and
restarted inside a launch, and in the exact mode; against the host restatement MLPController.features; the rejections; and
one whole actor-critic iteration (collect, critic, bootstrap, gae, PPO loss, backward) whose gradients repeat bit for bit.
The envs, policies and the bit comparison are those of test_gpu_collect.py, from support.py."""
import ctypes as C

import pytest

import support
from support import (DAYS, POLICY_STATE, bits as _bits, gpu_torch as _torch, gym_env as _mk_gym,
                     hypo_leaning_policies as _hypo_leaning_policies, meal_day_env as _mk, random_policy as _policy)

pytestmark = pytest.mark.gpu
N = 128
STATE = support.STATE + ("meal_time", "meal_amt", "start_minute", "episode")


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
    pol = _hypo_leaning_policies(1, history=H)
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
    pol = _hypo_leaning_policies(1, history=4)
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
    pol = _hypo_leaning_policies(1, history=4)
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
