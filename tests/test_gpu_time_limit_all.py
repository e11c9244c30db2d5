"""The time limit in every collector, on the GPU: collect_pid_limit, collect_bb_limit (ctrl_collect_limit_kernel),
collect_mlp_dopri5_limit (dopri5_mlp_collect_limit_kernel), collect_pid_dopri5_limit and collect_bb_dopri5_limit
(dopri5_ctrl_collect_limit_kernel) against the loop of existing entry points with the cut mask, bit for bit: cut into launches,
sharded, on a partial wave, with a limit nobody reaches and with the exact mode's calls cut into short launches; the C ABI's
refusals; and gae(truncated=, cut_value=) on a basal-bolus batch.  The design is tests/test_gpu_time_limit.py's; the runs are
support_limit.py's, made once and shared."""
import ctypes as C

import pytest

import support
import support_ctrl
import support_limit as SL
from support import DAYS, ST, bits as _bits, gpu_torch as _torch

pytestmark = pytest.mark.gpu
N = 256
CTRL_CASES = [("pid", "float64", False), ("pid", "float32", False), ("pid", "float64", True),
              ("bb", "float64", False), ("bb", "float32", False), ("bb", "float64", True)]


def _id(case):
    return "%s-%s-%s" % (case[0], case[1], "exact" if case[2] else "fixed")


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("case", CTRL_CASES, ids=_id)
def test_the_controllers_collector_is_the_loop(case):
    """max_episode_steps = s*, 2 s* + 3 steps in launches of (s*, s* - 2, 5) under the "hot" workload: env state (h_carry and
    the summed nfev in the exact mode), feature windows, controller state, accumulators, episode statistics, terminal_obs, every
    trace column the loop has ("truncated" among them) and cut_features are the loop's, bit for bit"""
    kind, dtype_name, exact = case
    s, i0 = SL.ctrl_first_ending(kind, dtype_name, exact)
    B = SL.ctrl_limited_loop(kind, dtype_name, exact)
    SL.check_reference(B, s, i0)
    A = SL.ctrl_limited(kind, dtype_name, exact)
    SL.ctrl_same(A, B, kind, exact, action=False)
    # the action column, which the loop's entry points do not record, is compared with the sibling collector's in test 2; here
    # only that every step wrote one
    assert not bool(_torch().isnan(A["tr"]["action"][1:]).any())


@pytest.mark.parametrize("kind", ["plain", "noisy"])
def test_the_exact_mlp_collector_is_the_loop(kind):
    """the same for collect_mlp_dopri5_limit: under 0.05 U/min, and under two hypo-leaning weight sets with sigma = 0.3, where
    the loop's step is collect_mlp_dopri5(1, sigma, on_done="continue") and the draws ("eps") are compared too"""
    s, i0 = SL.mlp_first_ending(kind)
    B = SL.mlp_limited_loop(kind)
    SL.check_reference(B, s, i0)
    A = SL.mlp_limited(kind)
    SL.mlp_same(A, B)
    if kind == "noisy":
        assert bool((B["tr"]["eps"][1:] != 0).all())


# ---------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("case", [("pid", "float64", False), ("bb", "float32", False), ("bb", "float64", True)], ids=_id)
def test_a_limit_nobody_reaches_is_the_controllers_collector(case):
    """max_episode_steps = 10^6 is collect_*(on_done="restart"), bit for bit, on launches (s*, 7): envs terminate in row s* and
    restart; "truncated" stays 0 and cut_features its sentinel"""
    torch = _torch()
    kind, dtype_name, exact = case
    s, _ = SL.ctrl_first_ending(kind, dtype_name, exact)
    pol = support_ctrl.feature_policy()
    A = SL.ctrl_collector(SL.env(N, dtype_name, exact), kind, pol, (s, 7), SL.FAR, exact)
    B = SL.ctrl_collector(SL.env(N, dtype_name, exact), kind, pol, (s, 7), None, exact)
    assert int(B["tr"]["done"].sum()) > 0
    assert int(A["tr"]["truncated"].sum()) == 0
    assert torch.equal(A["cut_features"], SL.sentinel(A["e"]))
    SL.ctrl_same(A, B, kind, exact)


def test_a_limit_nobody_reaches_is_the_exact_mlp_collector():
    torch = _torch()
    s, _ = SL.mlp_first_ending("noisy")
    pol = SL.mlp_policy("noisy")
    A = SL.mlp_collector(SL.env(N, exact=True), pol, (s, 7), SL.FAR, SL.SIGMA)
    B = SL.mlp_collector(SL.env(N, exact=True), pol, (s, 7), None, SL.SIGMA)
    assert int(B["tr"]["done"].sum()) > 0
    assert int(A["tr"]["truncated"].sum()) == 0
    assert torch.equal(A["cut_features"], SL.sentinel(A["e"]))
    SL.mlp_same(A, B)


# ---------------------------------------------------------------------------------------------------------- 3
def test_shards_of_the_basal_bolus_collector():
    """two envs of 128 with env_offset 0 and 128 are the two halves of the 256-env run under the limit (the hot envs are those
    with global id >= 128: the upper shard)"""
    A = SL.ctrl_limited("bb", "float64", False)
    assert int(A["tr"]["truncated"].sum()) > 0
    for off in (0, 128):
        H = SL.ctrl_limited("bb", "float64", False, n=128, env_offset=off)
        SL.ctrl_same(A, H, "bb", False, sl=slice(off, off + 128))


def test_shards_of_the_exact_mlp_collector():
    """the same for collect_mlp_dopri5_limit with noise: one weight set per half"""
    A = SL.mlp_limited("noisy")
    for off in (0, 128):
        H = SL.mlp_limited("noisy", n=128, env_offset=off, half=off // 128)
        SL.mlp_same(A, H, sl=slice(off, off + 128))


@pytest.mark.parametrize("case", [("bb", "float64", False), ("pid", "float64", True)], ids=_id)
def test_a_partial_wave(case):
    """150 envs -- two waves and 22 lanes of a third -- are the envs [0:150] of the 256-env run"""
    kind, dtype_name, exact = case
    A = SL.ctrl_limited(kind, dtype_name, exact)
    S = SL.ctrl_limited(kind, dtype_name, exact, n=150)
    assert int(S["tr"]["truncated"][:, 128:].sum()) > 0                               # the partial wave is cut too
    SL.ctrl_same(A, S, kind, exact, sl=slice(0, 150))


# ---------------------------------------------------------------------------------------------------------- 4
def test_launch_cutting_of_the_exact_mlp_collector():
    """max_minutes_per_launch = 3 ST: every call in launches of three steps, each under the same limit, gives the default's bits"""
    A, B = SL.mlp_limited("plain"), SL.mlp_limited("plain", max_minutes_per_launch=3 * ST)
    assert int(B["tr"]["truncated"].sum()) > 0
    SL.mlp_same(A, B)


def test_launch_cutting_of_the_exact_basal_bolus_collector():
    A, B = SL.ctrl_limited("bb", "float64", True), SL.ctrl_limited("bb", "float64", True, max_minutes_per_launch=3 * ST)
    assert int(B["tr"]["truncated"].sum()) > 0
    SL.ctrl_same(A, B, "bb", True)


# ---------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("name", SL.ENTRY_POINTS)
def test_invalid_arguments_at_the_c_abi(name):
    """the five refusals of check_time_limit at each entry point: -1, the message under the entry point's name, and env, windows
    and controller state as they were"""
    torch = _torch()
    from simglucose_amd import _lib
    method = name[len("t1d_"):]
    exact = SL.METHODS[method][3]
    kind = "pid" if "_pid" in name else "bb" if "_bb" in name else "mlp"
    e = SL.env(128, exact=exact)
    pol = support.constant_policy(0.05) if kind == "mlp" else support_ctrl.feature_policy()
    st = e.new_policy_state(pol)
    cs = None if kind == "mlp" else support_ctrl.ctrl_state(e, kind, "hot")
    keys = support.GYM_STATE + (("h_carry",) if exact else ())
    before = {k: getattr(e, k).clone() for k in keys}
    before.update({k: v.clone() for k, v in st.items()})
    before.update({"ctrl_" + k: v.clone() for k, v in (cs or {}).items()})
    L = e._L

    def structs(on_done="restart"):
        draw = (None, None) if kind == "mlp" else None
        _, p, g, keep = e._collect_structs(method, 2, pol, st, None, None, on_done, DAYS, None, None, False, draw=draw, keep_h_carry=exact)
        if kind == "mlp":
            front = (p,)
        else:
            ctl = e._pid_struct(*support_ctrl.PID["hot"], cs, None)[1] if kind == "pid" else e._bb_struct(140.0, cs, None)[1]
            front = (ctl, p)
        e._set_trace(front[0], None, 2)
        return front, g, keep

    def limit(max_minutes=2 * ST, reserved=0):
        lim = _lib.TimeLimit()
        lim.max_minutes, lim.reserved, lim.cut_trace, lim.cut_feat = max_minutes, reserved, None, None
        return lim

    def call(front, g, lim, n_steps=2, minutes=ST):
        tail = (C.c_void_p(e.h_carry.data_ptr()), C.c_void_p(e.nfev.data_ptr()), n_steps, minutes) if exact else (n_steps, minutes, e.n_sub)
        with torch.cuda.device(e.device):
            return getattr(L, name)(e._ctx, C.byref(e._b), *[C.byref(x) for x in front], C.byref(g),
                                    C.byref(lim) if lim is not None else None, *tail, e._stream())

    f, g, keep = structs()
    f0, g0, keep0 = structs("continue")
    g0.on_done = 0
    for what, args, text in (("NULL limit", (f, g, None), b"limit is NULL"), ("max_minutes = 0", (f, g, limit(max_minutes=0)), b"max_minutes"),
                             ("reserved = 1", (f, g, limit(reserved=1)), b"reserved"), ("on_done = 0", (f0, g0, limit()), b"on_done"),
                             ("n_steps * minutes > max_minutes", (f, g, limit(max_minutes=2 * ST - 1)), b"n_steps * minutes")):
        assert call(*args) == -1, what
        assert L.t1d_last_error().startswith(name.encode() + b": ") and text in L.t1d_last_error(), (what, L.t1d_last_error())
    assert e.sync() == 0
    for k in keys:
        assert torch.equal(getattr(e, k), before[k]), k
    for k in st:
        assert torch.equal(st[k], before[k]), k
    for k in (cs or {}):
        assert torch.equal(cs[k], before["ctrl_" + k]), k


# ---------------------------------------------------------------------------------------------------------- 6
def test_end_to_end_the_bootstrap_at_a_cut_of_the_baseline():
    """gae(truncated, cut_value) on the basal-bolus fp64 traces of test 1 with a small critic: in the last row of cuts the
    advantage of a cut env is reward + gamma v_cut - v (lambda's term ends at the cut), computed in torch from the same words,
    within tests/test_gpu_gae.py's bound 4 (K - s) eps scale"""
    torch = _torch()
    from simglucose_amd.controller import gae, gae_reference, mlp_pre_output
    A = SL.ctrl_limited("bb", "float64", False)
    s, i0 = SL.ctrl_first_ending("bb", "float64", False)
    ea = A["e"]
    vpol = support.identity_policy(widths=(8, 1), seed=9)
    vparams = vpol.device_params(ea.device, ea.dtype)
    tr = A["tr"]
    K = tr["row"] - 1
    f, rew = tr["features"][1:].contiguous(), tr["reward"][1:].contiguous()
    done, trunc = tr["done"][1:].contiguous(), tr["truncated"][1:].contiguous()
    v = mlp_pre_output(vparams, f, vpol).detach().contiguous()
    v_cut = mlp_pre_output(vparams, A["cut_features"][None].contiguous(), vpol)[0].detach().contiguous()
    v_last = mlp_pre_output(vparams, ea.policy_features(vpol, A["ps"])[None], vpol)[0].detach().contiguous()
    gamma, lam = 0.99, 0.95
    adv, ret = gae(rew, done, v, v_last, gamma=gamma, lam=lam, truncated=trunc, cut_value=v_cut)
    _, _, scale = gae_reference(rew, done, v, v_last, gamma=gamma, lam=lam, truncated=trunc, cut_value=v_cut)
    # the last cut of every env is the one cut_features holds: row 2 s* for most, row s* for those that ended in between
    eps = torch.finfo(torch.float64).eps
    row = 2 * s - 1                                                                   # 0-based row of the last wave of cuts
    cut = trunc[row].bool()
    assert int(cut.sum()) > 0
    want = rew[row] + gamma * v_cut - v[row]
    err = (adv[row] - want).abs()
    print("\n[gae on collect_bb_limit] %d cut envs in row 2 s* = %d, max err / bound = %.3f"
          % (int(cut.sum()), 2 * s, float((err[cut] / (4 * (K - row) * eps * scale[row][cut])).max())))
    assert bool((err[cut] <= 4 * (K - row) * eps * scale[row][cut]).all())
    # an env cut in row s* and not again: its cut_features are row s*'s
    once = trunc[s - 1].bool() & (trunc.sum(dim=0) == 1)
    if int(once.sum()) > 0:
        want = rew[s - 1] + gamma * v_cut - v[s - 1]
        assert bool(((adv[s - 1] - want).abs()[once] <= 4 * (K - s + 1) * eps * scale[s - 1][once]).all())
    assert bool(done[s - 1, i0]) and float((adv[s - 1, i0] - (rew[s - 1, i0] - v[s - 1, i0])).abs()) <= 4 * eps * float(scale[s - 1, i0])
