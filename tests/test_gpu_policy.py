"""Closed-loop roll-outs under the in-kernel MLP policy on the GPU (BatchedT1DSimEnv.rollout_mlp -> t1d_rollout_mlp,
csrc/t1d_policy.hpp): pinned to rollout_pid bit for bit, against the step() loop with the policy in torch, cut / shard /
multi-policy invariance, the meaning of every feature, and the argument checks.  The envs (_mk: all 30 patients, a
random-meal day from 06:00), the random policies and the comparisons come from support.py."""
import ctypes as C
import math

import numpy as np
import pytest

from support import (ST, STATE, STATS, bits as _bits, gpu_torch as _torch, meal_day_env as _mk, random_policy as _policy,
                     same_dicts as _same_dicts, same_env as _same_env, stats as _stats)

pytestmark = pytest.mark.gpu
# fp32 tolerance of test_against_host_loop: the issue leaves it open.  Summation order is the only legitimate difference
# between the kernel and the host loop, so the yardstick is how far the host loop's own two evaluation orders (torch.matmul
# and bias-first ascending accumulation) drift apart on this workload: FP32_ORDER_DRIFT is the 99.5th percentile over the
# 4 096 envs of that drift (largest |BG or CGM| difference of an env over the 160 steps), to be measured on an MI355X and recorded
# in profiles/policy/README.md; while it is None the test takes that percentile from the run itself.  A percentile, not the maximum: in fp32 nearly every env sees a pump-quantiser tie land on
# the other side somewhere, and the worst env of 4 096 is an outlier that would make the bound meaningless.  The kernel gets
# four times that, for all but the 0.5 % of envs the fp64 form allows as well.
FP32_ORDER_DRIFT = None                  # mg/dL
FP32_DRIFT_FACTOR = 4.0


def _rollout(e, pol, chunks, columns=("bg", "cgm", "cho", "insulin", "action")):
    tr = e.new_trace(sum(chunks), columns=columns)
    stats, state = _stats(e), None
    for ch in chunks:
        state = e.rollout_mlp(ch, pol, policy_state=state, stats=stats, trace=tr)
    assert e.sync() == 0
    return state, stats, tr


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_one_weight_on_cgm0_is_rollout_pid_bit_for_bit(dtype_name):
    """A one-layer net with cgm_mean = target, cgm_scale = 1, weight P on CGM[0] and identity output asks for
    P (CGM - target), which is PIDController with I = D = 0: state, outputs, accumulators and traces of rollout_pid."""
    torch = _torch()
    from simglucose_amd.controller.mlp_ctrller import MLPController
    dtype = getattr(torch, dtype_name)
    n, K, P, target = 192, 60, 1.5e-4, 140.0
    W = torch.zeros(1, 5, dtype=torch.float64); W[0, 0] = P
    pol = MLPController([(W, torch.zeros(1))], history=1, output="identity", cgm_mean=target, cgm_scale=1.0)
    a, b = _mk(n, dtype), _mk(n, dtype)
    sa, ta = _stats(a), a.new_trace(K)
    ps = a.rollout_pid(20, P, 0.0, 0.0, target=target, stats=sa, trace=ta)
    a.rollout_pid(K - 20, P, 0.0, 0.0, target=target, pid_state=ps, stats=sa, trace=ta)
    assert a.sync() == 0
    sb, tb = _stats(b), b.new_trace(K, columns=("bg", "cgm", "cho", "insulin", "action"))
    st = b.rollout_mlp(20, pol, stats=sb, trace=tb)
    b.rollout_mlp(K - 20, pol, policy_state=st, stats=sb, trace=tb)
    assert b.sync() == 0
    _same_env(a, b)
    _same_dicts(sa, sb, STATS)
    _same_dicts(ta, tb, ("bg", "cgm", "cho", "insulin"))
    assert float(tb["insulin"][1:].max()) > 0 and float(tb["cgm"].std()) > 0


# ---------------------------------------------------------------------------------------------------------- 2
def _host_loop(e, pol, K, ordered):
    """the step() loop a user writes today: features and network as torch ops between the launches"""
    torch = _torch()
    st = e.new_policy_state(pol)
    zero = torch.zeros(e.n, dtype=e.dtype, device=e.device)
    bg, cgm = [], []
    for _ in range(K):
        feat = pol.features(st["cgm_hist"], st["ins_hist"], st["prev_meal"], e.start_minute + e.t)
        e.step(pol.forward(feat, ordered=ordered), zero)
        pol.shift(st["cgm_hist"], st["ins_hist"], e.cgm, e.insulin)
        st["prev_meal"] = e.meal.clone()
        bg.append(e.bg.clone()); cgm.append(e.cgm.clone())
    assert e.sync() == 0
    return torch.stack(bg), torch.stack(cgm)


def _worst(a, b):
    """per env: the largest |difference| over the steps and the two traces"""
    torch = _torch()
    return torch.maximum((a[0] - b[0]).abs().max(dim=0).values, (a[1] - b[1]).abs().max(dim=0).values)


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_against_host_loop(dtype_name):
    """4 096 envs, all 30 patients, random meal tables, Dexcom, 160 steps, a random 2-hidden-layer tanh net with logistic
    output.  fp64: BG and CGM within 1e-6 mg/dL for every env but at most 0.5 % of them (a pump-quantiser tie landing on the
    other side); the reference alone (torch.matmul against ordered accumulation) must stay under a tenth of that cap.
    fp32: within four times FP32_ORDER_DRIFT, the recorded drift between the host loop's own two evaluation orders, for all
    but 0.5 % of the envs."""
    torch = _torch()
    dtype = getattr(torch, dtype_name)
    n, K = 4096, 160
    pol = _policy()
    hm = _host_loop(_mk(n, dtype), pol, K, ordered=False)
    ho = _host_loop(_mk(n, dtype), pol, K, ordered=True)
    ref = _worst(hm, ho)
    e = _mk(n, dtype)
    _, _, tr = _rollout(e, pol, (K,), columns=("bg", "cgm"))
    dev = _worst((tr["bg"][1:], tr["cgm"][1:]), ho)
    print("\n[%s] host matmul vs ordered: max %.3e mg/dL, envs > 1e-6: %d;  kernel vs ordered host: max %.3e, envs > 1e-6: %d"
          % (dtype_name, float(ref.max()), int((ref > 1e-6).sum()), float(dev.max()), int((dev > 1e-6).sum())))
    if dtype == torch.float64:
        cap = int(0.005 * n)
        assert int((ref > 1e-6).sum()) <= cap // 10
        assert int((dev > 1e-6).sum()) <= cap
    else:
        q = torch.tensor([0.5, 0.9, 0.99, 0.995, 1.0], device=ref.device)
        print("[float32] quantiles 0.5 / 0.9 / 0.99 / 0.995 / max of the per-env drift: host orders %s;  kernel vs host %s"
              % (["%.3e" % v for v in torch.quantile(ref.double(), q.double()).tolist()],
                 ["%.3e" % v for v in torch.quantile(dev.double(), q.double()).tolist()]))
        seen = float(torch.quantile(ref.double(), 0.995))
        cap = int(0.005 * n)
        drift = seen if FP32_ORDER_DRIFT is None else FP32_ORDER_DRIFT
        assert drift > 0.0 and drift / 2 <= seen <= 2 * drift             # the yardstick describes this workload
        assert int((dev > FP32_DRIFT_FACTOR * drift).sum()) <= cap
    assert float(hm[0].std()) > 5.0                                     # the policy and the meals move the glucose


# ---------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_cut_invariance(dtype_name):
    torch = _torch()
    dtype = getattr(torch, dtype_name)
    pol = _policy(history=5, widths=(12, 7, 1), hidden="relu")
    runs = []
    for chunks in ((40,), (10,) * 4, (1,) * 40):
        e = _mk(256, dtype)
        runs.append((e,) + _rollout(e, pol, chunks))
    for e, st, stats, tr in runs[1:]:
        _same_env(runs[0][0], e)
        _same_dicts(runs[0][1], st, ("cgm_hist", "ins_hist", "prev_meal"))
        _same_dicts(runs[0][2], stats, STATS)
        _same_dicts(runs[0][3], tr, ("bg", "cgm", "cho", "insulin", "action"))
    assert float(runs[0][3]["action"][1:].std()) > 0


# ---------------------------------------------------------------------------------------------------------- 4
def test_shards_equal_slices_of_the_big_batch():
    torch = _torch()
    n, K, epp = 1024, 30, 128
    pol = _policy(n_policies=n // epp, seed=2)
    big = _mk(n, torch.float64)
    st, stats, tr = _rollout(big, pol, (K,))
    from simglucose_amd.controller.mlp_ctrller import MLPController
    for a, b in ((0, 128), (256, 640), (896, 1024)):
        sub = MLPController([(W[a // epp:b // epp], bb[a // epp:b // epp]) for W, bb in zip(pol.W, pol.b)], history=pol.history,
                            hidden=pol.hidden, output=pol.output, out_scale=pol.out_scale)
        e = _mk(b - a, torch.float64, env_offset=a)
        s2, stats2, tr2 = _rollout(e, sub, (K,))
        sl = slice(a, b)
        _same_env(big, e, sl=sl)
        _same_dicts(st, s2, ("cgm_hist", "ins_hist", "prev_meal"), sl)
        _same_dicts(stats, stats2, STATS, sl)
        _same_dicts(tr, tr2, ("bg", "cgm", "cho", "insulin", "action"), sl)


# ---------------------------------------------------------------------------------------------------------- 5
def test_many_policies():
    """8 weight sets x 512 identical envs = eight single-policy batches, and the eight differ from one another"""
    torch = _torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    from simglucose_amd.controller.mlp_ctrller import MLPController
    P, epp, K = 8, 512, 30

    def mk(n):
        # every block of 512 envs is the same 512 envs: ids, patients, meals and noise repeat with period 512
        e = BatchedT1DSimEnv(patient=np.arange(n) % epp % 30, sensor="Dexcom", noise="host",
                             normals=np.tile(np.random.RandomState(1).randn(1 + 10 * 5, epp), (1, n // epp)))
        rs = np.random.RandomState(2)
        mt = np.sort(rs.choice(np.arange(2, K * ST - 2), size=(3, epp), replace=True), axis=0)
        for j in range(1, 3):
            mt[j] = np.maximum(mt[j], mt[j - 1] + 1)
        ma = rs.uniform(20.0, 80.0, size=(3, epp))
        e.set_meals(torch.as_tensor(np.tile(mt, (1, n // epp))), torch.as_tensor(np.tile(ma, (1, n // epp))))
        e.reset()
        return e
    pol = _policy(n_policies=P, seed=4)
    big = mk(P * epp)
    st, stats, tr = _rollout(big, pol, (K,))
    finals = []
    for k in range(P):
        one = MLPController([(W[k:k + 1], b[k:k + 1]) for W, b in zip(pol.W, pol.b)], history=pol.history, hidden=pol.hidden,
                            output=pol.output, out_scale=pol.out_scale)
        e = mk(epp)
        s2, stats2, tr2 = _rollout(e, one, (K,))
        sl = slice(k * epp, (k + 1) * epp)
        _same_env(big, e, sl=sl)
        _same_dicts(st, s2, ("cgm_hist", "ins_hist", "prev_meal"), sl)
        _same_dicts(stats, stats2, STATS, sl)
        _same_dicts(tr, tr2, ("bg", "cgm", "cho", "insulin", "action"), sl)
        finals.append(tr2["action"][1:].clone())
    for j in range(P):
        for k in range(j + 1, P):
            assert not torch.equal(finals[j], finals[k])


# ---------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_feature_semantics(dtype_name):
    """A net whose only weight sits on one feature shows that feature in action_trace: row s (1-based, as new_trace lays
    the rows out) is the action of step s, taken from the observations up to row s - 1."""
    torch = _torch()
    from simglucose_amd.controller.mlp_ctrller import MLPController
    dtype = getattr(torch, dtype_name)
    H, n, K, w, mean = 4, 128, 80, 3.0e-4, 120.0
    F = 2 * H + 3
    starts = 300 + 11 * np.arange(n)                  # every env starts at its own minute of day, 05:00 .. 04:17 next day

    def run(j, **kw):
        W = torch.zeros(1, F, dtype=torch.float64); W[0, j] = w
        pol = MLPController([(W, torch.zeros(1))], history=H, output="identity", cgm_mean=mean, cgm_scale=1.0, ins_scale=1.0,
                            cho_scale=1.0, **kw)
        e = _mk(n, dtype, start=starts)
        obs0 = e.cgm.clone()
        _, _, tr = _rollout(e, pol, (K,))
        return tr, obs0
    wt = torch.tensor(w, dtype=dtype).item()          # the weight as the kernel holds it
    for k in range(H):
        tr, obs0 = run(k)
        # observations: what reset() returned, then cgm rows 1 ..; before the episode the window repeats the first one
        obs = torch.cat([obs0.unsqueeze(0).repeat(H, 1), tr["cgm"][1:]])          # obs[H - 1 + s] = observation after step s
        for s in range(1, K + 1):
            assert torch.equal(tr["action"][s], wt * (obs[H + s - 2 - k] - mean)), (k, s)
        tr, _ = run(H + k)
        ins = torch.cat([torch.zeros(H, n, dtype=dtype, device=tr["insulin"].device), tr["insulin"][1:]])   # ins[H + s - 1] = step s
        for s in range(1, K + 1):
            assert torch.equal(tr["action"][s], wt * ins[H + s - 2 - k]), (k, s)
    tr, _ = run(2 * H)
    cho = torch.cat([torch.zeros(1, n, dtype=dtype, device=tr["cho"].device), tr["cho"][1:]])
    for s in range(1, K + 1):
        assert torch.equal(tr["action"][s], wt * cho[s - 1]), s
    assert float(tr["action"][1:].max()) > 0                    # a meal was announced
    # time of day: sin and cos of 2 pi (start_minute + t) / 1440 at the start of step s, t = 3 (s - 1); the kernel's sinpi /
    # cospi and the product with the weight are each good to a few ulp: 1e-15 / 1e-6 relative to the weight
    tol = w * (1e-14 if dtype == torch.float64 else 2e-6)
    for j, fn in ((2 * H + 1, math.sin), (2 * H + 2, math.cos)):
        tr, _ = run(j)
        for s in range(1, K + 1):
            want = torch.tensor([w * fn(2.0 * math.pi * ((int(m0) + ST * (s - 1)) % 1440) / 1440.0) for m0 in starts],
                                dtype=torch.float64, device=tr["action"].device)
            assert float((tr["action"][s].double() - want).abs().max()) <= tol, (j, s)


# ---------------------------------------------------------------------------------------------------------- 7
def test_rejections_change_nothing():
    torch = _torch()
    from simglucose_amd import _lib
    e = _mk(128, torch.float64)
    pol = _policy(history=3, widths=(8, 1))
    st = e.new_policy_state(pol)
    params = pol.flat_params().to(e.device)
    before = {k: getattr(e, k).clone() for k in STATE}
    before.update({k: v.clone() for k, v in st.items()})
    L = e._L

    def good():
        p = _lib.Mlp()
        pol.fill_struct(p)
        p.n_policies, p.envs_per_policy, p.n_params = 1, e.n, params.shape[1]
        p.params = params.data_ptr()
        for k in ("cgm_hist", "ins_hist", "prev_meal"):
            setattr(p, k, st[k].data_ptr())
        return p

    def call(p, n_steps=2, minutes=3, n_sub=4):
        with torch.cuda.device(e.device):
            return L.t1d_rollout_mlp(e._ctx, C.byref(e._b), C.byref(p) if p is not None else None, n_steps, minutes, n_sub, e._stream())
    bad = []
    for field, value in (("history", 0), ("history", 13), ("n_layers", 0), ("n_layers", 5), ("hidden_act", 2), ("out_act", -1),
                         ("params", None), ("cgm_hist", None), ("ins_hist", None), ("prev_meal", None), ("n_policies", 0),
                         ("n_policies", 2), ("envs_per_policy", 64), ("envs_per_policy", 100), ("n_params", params.shape[1] + 1)):
        p = good(); setattr(p, field, value); bad.append((field, value, p))
    for l, wv in ((0, 0), (0, 33), (1, 2)):
        p = good(); p.width[l] = wv; bad.append(("width[%d]" % l, wv, p))
    for field, value, p in bad:
        assert call(p) == -1, (field, value)
        assert len(L.t1d_last_error()) > len(b"t1d_rollout_mlp: "), (field, value)
        assert L.t1d_last_error().startswith(b"t1d_rollout_mlp"), (field, value)
    assert call(None) == -1 and b"mlp is NULL" in L.t1d_last_error()
    assert call(good(), n_steps=0) == -1 and b"n_steps" in L.t1d_last_error()
    assert call(good(), minutes=0) == -1 and call(good(), n_sub=0) == -1
    assert e.sync() == 0
    for k in STATE:
        assert torch.equal(getattr(e, k), before[k]), k
    for k in st:
        assert torch.equal(st[k], before[k]), k
    with pytest.raises(ValueError):
        e.rollout_mlp(2, _policy(n_policies=4))                 # 128 envs / 4 = 32 per policy
    with pytest.raises(ValueError):
        e.rollout_mlp(0, pol)
    with pytest.raises(ValueError):
        e.rollout_mlp(2, pol, policy_state={"cgm_hist": st["cgm_hist"][:2], "ins_hist": st["ins_hist"], "prev_meal": st["prev_meal"]})
    assert call(good()) == 0 and e.sync() == 0                   # and the good one runs
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    ex = BatchedT1DSimEnv(patient=np.arange(64) % 30, integrator="dopri5")
    ex.reset()
    with pytest.raises(_lib.T1DError):
        ex.rollout_mlp(2, pol)


# ---------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_top_of_the_range(dtype_name):
    """H = 12, four layers, widths 32: 56 rows per lane, so the fp64 launch drops to two waves per workgroup with more than
    64 KiB of dynamic LDS.  Cut invariance bit for bit, and every action against the host's ordered forward pass on the
    features rebuilt from the kernel's own traces -- teacher-forced, so nothing is amplified by the closed loop: the bound is
    the rounding of a few dozen fused multiply-adds per layer and of the two exp-based activations, 1e-13 of the output
    range in fp64, 1e-5 of it in fp32 (the fp32 exp is the hardware's 1-ulp v_exp_f32)."""
    torch = _torch()
    dtype = getattr(torch, dtype_name)
    H, n, K = 12, 256, 24
    pol = _policy(history=H, widths=(32, 32, 32, 1), seed=7)
    starts = 17 * np.arange(n) % 1440
    runs = []
    for chunks in ((K,), (5, 7, 12)):
        e = _mk(n, dtype, start=starts)
        obs0 = e.cgm.clone()
        runs.append((e,) + _rollout(e, pol, chunks))
    _same_env(runs[0][0], runs[1][0])
    _same_dicts(runs[0][1], runs[1][1], ("cgm_hist", "ins_hist", "prev_meal"))
    _same_dicts(runs[0][2], runs[1][2], STATS)
    _same_dicts(runs[0][3], runs[1][3], ("bg", "cgm", "cho", "insulin", "action"))
    e, st, _, tr = runs[0]
    cgm_hist = obs0.unsqueeze(0).repeat(H, 1)
    ins_hist = torch.zeros(H, n, dtype=dtype, device=e.device)
    meal = torch.zeros(n, dtype=dtype, device=e.device)
    worst = 0.0
    for s in range(1, K + 1):
        feat = pol.features(cgm_hist, ins_hist, meal, e.start_minute + ST * (s - 1))
        want = pol.forward(feat.double(), ordered=True)
        worst = max(worst, float((tr["action"][s].double() - want).abs().max()))
        pol.shift(cgm_hist, ins_hist, tr["cgm"][s], tr["insulin"][s])
        meal = tr["cho"][s]
    assert torch.equal(_bits(st["cgm_hist"]), _bits(cgm_hist)) and torch.equal(_bits(st["ins_hist"]), _bits(ins_hist))
    print("\n[%s] top of the range: max |action - host forward| = %.3e U/min" % (dtype_name, worst))
    assert worst <= pol.out_scale * (1e-13 if dtype == torch.float64 else 1e-5)
    assert float(tr["action"][1:].std()) > 0
