"""Time-limited episodes on the GPU: collect_mlp_limit (t1d_collect_mlp_limit, mlp_collect_limit_kernel) against
the loop of existing entry points with the cut mask, bit for bit, under the plain, the hybrid and the relative policy, with and
without exploration noise, cut into launches, sharded, and with a limit nobody reaches; the C ABI's refusals; gae(truncated=,
cut_value=) (t1d_gae_limit) against gae_reference; and the two together."""
import ctypes as C
import functools

import pytest

import support
from support import DAYS, ST, bits as _bits, gpu_torch as _torch

pytestmark = pytest.mark.gpu
N = 256
COLS = support.MLP_TRACE + ("reward", "done", "eps", "features", "truncated")
ENV_KEYS = support.STATE + ("meal_time", "meal_amt", "start_minute", "episode", "cgm0")
SIGMA, EXPLORE_SEED = 0.3, 0xC0FFEE
KINDS = [("plain", "float64"), ("plain", "float32"), ("bolus", "float64"), ("rel", "float64"), ("rel", "float32")]


def _policy(kind):
    """plain: 0.05 U/min whatever the net sees; bolus: that with a meal bolus; rel: small random weights around six times each
    env's own basal rate with a meal bolus (the envs alternate between two patients); noisy: two hypo-leaning weight sets"""
    if kind == "plain":
        return support.constant_policy(0.05)
    if kind == "bolus":
        pol = support.constant_policy(0.05)
        return type(pol)(list(zip(pol.W, pol.b)), history=pol.history, output="identity", out_scale=1.0, out_bias=0.05, meal_bolus=140)
    if kind == "rel":
        return support.random_policy(widths=(8, 1), seed=6, output="identity", gain=0.02, out_scale=1.0, out_bias=6.0,
                                     relative_to="basal", meal_bolus=140)
    assert kind == "noisy"
    return support.hypo_leaning_policies(2)


def _sigma(kind):
    return SIGMA if kind == "noisy" else None


def _columns(pol):
    return COLS + (("bolus",) if pol.meal_bolus is not None else ())


def _loop(e, pol, K, L, sigma, cut_features, st=None):
    """What a trainer does without the limit's collector, K times: the one-step call (rollout_mlp(1); with sigma collect_mlp(1,
    on_done="continue")), cut = ~done & (t >= L ST), policy_features where cut, restart_done(mask = done | cut), the torch
    reset of the masked envs' windows.  L = None: no limit -> everything the collector's call leaves, as a dict"""
    torch = _torch()
    st = e.new_policy_state(pol) if st is None else st
    acc, es, term = support.stats(e), support.episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
    tr = e.new_trace(K, columns=_columns(pol), history=pol.history)
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    for _ in range(K):
        row = tr["row"]
        if sigma is None:
            tr["features"][row] = e.policy_features(pol, st)
            e.rollout_mlp(1, pol, policy_state=st, stats=acc, trace=tr)
            tr["reward"][row] = e.reward; tr["done"][row] = e.done; tr["eps"][row] = 0
        else:
            e.collect_mlp(1, pol, sigma=sigma, explore_seed=EXPLORE_SEED, policy_state=st, stats=acc, trace=tr, on_done="continue")
        done = e.done.bool()
        cut = ~done & (e.t >= L * ST) if L is not None else torch.zeros_like(done)
        tr["truncated"][row] = cut
        if L is not None:
            cut_features.copy_(torch.where(cut, e.policy_features(pol, st), cut_features))
        mask = done | cut
        e.restart_done(mask=mask, days=DAYS, terminal_obs=term, episode_stats=es)
        st["cgm_hist"].copy_(torch.where(mask, e.cgm, st["cgm_hist"]))             # new_policy_state for the envs that restarted
        st["ins_hist"].copy_(torch.where(mask, zero, st["ins_hist"]))
        st["prev_meal"].copy_(torch.where(mask, zero, st["prev_meal"]))
    assert e.sync() == 0
    return dict(st=st, acc=acc, es=es, term=term, tr=tr, cut_features=cut_features)


def _collector(e, pol, cuts, L, sigma, cut_features):
    """the collector in launches of `cuts` steps -> the same dict"""
    torch = _torch()
    acc, es, term = support.stats(e), support.episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
    tr = e.new_trace(sum(cuts), columns=_columns(pol), history=pol.history)
    st = None
    kw = dict(sigma=sigma, explore_seed=EXPLORE_SEED, stats=acc, trace=tr, days=DAYS, terminal_obs=term, episode_stats=es)
    for k in cuts:
        if L is not None:
            st = e.collect_mlp_limit(k, pol, L, cut_features, policy_state=st, **kw)
        else:                                                                        # no limit: "truncated" stays 0
            st = e.collect_mlp(k, pol, policy_state=st, on_done="restart", **kw)
    assert e.sync() == 0
    return dict(st=st, acc=acc, es=es, term=term, tr=tr, cut_features=cut_features)


def _same(A, B, ea, eb, pol, sl=slice(None)):
    """run B (of env eb) is the envs `sl` of run A (of env ea), bit for bit"""
    support.same_env(ea, eb, keys=ENV_KEYS, sl=sl)
    support.same_dicts(A["st"], B["st"], support.POLICY_STATE, sl=sl)
    support.same_dicts(A["acc"], B["acc"], support.STATS, sl=sl)
    support.same_dicts(A["es"], B["es"], support.EPISODE_STATS, sl=sl)
    support.same_dicts(A, B, ("term", "cut_features"), sl=sl)
    support.same_dicts(A["tr"], B["tr"], _columns(pol), sl=sl)
    assert A["tr"]["row"] == B["tr"]["row"]


def _sentinel(e, pol):
    torch = _torch()
    return torch.full((2 * pol.history + 3, e.n), -77.0, dtype=e.dtype, device=e.device)


# ---------------------------------------------------------------------------------------------------------- 0
@functools.lru_cache(maxsize=None)
def _first_ending(kind, dtype_name):
    """The no-limit reference loop under the policy of `kind`, 300 steps from the common start -> (s*, the first env that
    terminates there): s* is the first row in which any env terminates.  2 <= s* <= 300 is asserted, so that no test below
    passes on nothing.  (tests/test_gpu_collect.py relies on >= 5 % of these envs ending within 400 steps under 0.05 U/min.)
    Computed once per policy and dtype; the non-noisy kinds run support.loop_of_entry_points."""
    torch = _torch()
    pol, K = _policy(kind), 300
    e = support.gym_env(N, getattr(torch, dtype_name))
    if _sigma(kind) is None:
        tr = e.new_trace(K, columns=support.MLP_TRACE + ("reward", "done"))
        support.loop_of_entry_points(e, pol, K, support.stats(e), tr, torch.zeros(N, dtype=e.dtype, device=e.device),
                                     support.episode_stats(e))
    else:
        tr = _loop(e, pol, K, None, _sigma(kind), None)["tr"]
    rows = tr["done"].bool().any(dim=1).nonzero().flatten()
    assert rows.numel() > 0, "no env terminates within 300 steps"
    s = int(rows[0])
    assert 2 <= s <= 300, s
    print("\n[time limit %s %s] first termination in row s* = %d (%d envs)" % (kind, dtype_name, s, int(tr["done"][s].sum())))
    return s, int(tr["done"][s].nonzero().flatten()[0])


@functools.lru_cache(maxsize=None)
def _pair(kind, dtype_name):
    """A: the collector under max_episode_steps = s* in launches of (s*, s* - 2, 5) steps; B: the loop -> (A, B, env A, env B, s*,
    the env that terminates in row s*).  Shared by the tests below; treat as read-only."""
    torch = _torch()
    s, i0 = _first_ending(kind, dtype_name)
    pol, dt = _policy(kind), getattr(torch, dtype_name)
    ea, eb = support.gym_env(N, dt), support.gym_env(N, dt)
    cuts = tuple(k for k in (s, s - 2, 5) if k > 0)
    A = _collector(ea, pol, cuts, s, _sigma(kind), _sentinel(ea, pol))
    B = _loop(eb, pol, 2 * s + 3 if s > 2 else sum(cuts), s, _sigma(kind), _sentinel(eb, pol))
    return A, B, ea, eb, s, i0


def _check_pair(kind, dtype_name):
    torch = _torch()
    A, B, ea, eb, s, i0 = _pair(kind, dtype_name)
    pol = _policy(kind)
    # on the reference loop: what the comparison covers
    done, trunc = B["tr"]["done"].bool(), B["tr"]["truncated"].bool()
    assert int((done & trunc).sum()) == 0
    assert not bool(done[:s].any()) and not bool(trunc[:s].any())
    assert bool(done[s, i0]) and not bool(trunc[s, i0])                               # done wins in the row of the limit
    assert bool((trunc[s] | done[s]).all()) and int(trunc[s].sum()) >= N - int(done[s].sum()) > 0   # every other env is cut there
    if s > 2:
        assert int(trunc[2 * s].sum()) > 0                                            # second cuts, mid-launch (row s* closes a launch)
        assert bool((trunc[2 * s] | done[s + 1:2 * s + 1].any(dim=0)).all())
    sent = _bits(_sentinel(eb, pol))
    written = (_bits(B["cut_features"]) != sent).any(dim=0)
    assert bool((written == trunc.any(dim=0)).all())                                  # written for cut envs only
    assert int(B["es"]["last_length"].max()) <= s and int((B["es"]["last_length"] == s).sum()) > 0
    # the collector is the loop
    _same(A, B, ea, eb, pol)
    assert ea._clock is None
    return A, B, s


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kind,dtype_name", KINDS)
def test_the_collector_is_the_loop(kind, dtype_name):
    """max_episode_steps = s*, 2 s* + 3 steps in launches of (s*, s* - 2, 5): env state, policy state, accumulators, episode
    statistics, terminal_obs, every trace column ("truncated" among them) and cut_features are the loop's, bit for bit"""
    _check_pair(kind, dtype_name)


# ---------------------------------------------------------------------------------------------------------- 2
def test_with_exploration_noise():
    """the same under two hypo-leaning weight sets with sigma = 0.3 and an explore_seed of its own: the loop's step is
    collect_mlp(1, sigma, on_done="continue"), and the draws ("eps") are compared too"""
    A, B, s = _check_pair("noisy", "float64")
    assert bool((B["tr"]["eps"][1:] != 0).all())


# ---------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("kind", ["plain", "bolus", "rel", "noisy"])
def test_a_limit_nobody_reaches(kind):
    """max_episode_steps = 10^6 is collect_mlp(on_done="restart"), bit for bit: "truncated" stays 0, cut_features its sentinel"""
    torch = _torch()
    s, _ = _first_ending(kind, "float64")
    pol, cuts = _policy(kind), (s, 7)                                                 # envs terminate in row s* and restart
    ea, eb = support.gym_env(N), support.gym_env(N)
    A = _collector(ea, pol, cuts, 10 ** 6, _sigma(kind), _sentinel(ea, pol))
    B = _collector(eb, pol, cuts, None, _sigma(kind), _sentinel(eb, pol))
    assert int(B["tr"]["done"].sum()) > 0
    assert int(A["tr"]["truncated"].sum()) == 0
    assert torch.equal(A["cut_features"], _sentinel(ea, pol))
    _same(A, B, ea, eb, pol)


# ---------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("kind", ["rel", "noisy"])
def test_shards(kind):
    """two envs of 128 with env_offset 0 and 128 are the two halves of the 256-env run under the limit"""
    torch = _torch()
    A, _, ea, _, s, _ = _pair(kind, "float64")
    pol = _policy(kind)
    cuts = tuple(k for k in (s, s - 2, 5) if k > 0)
    for off in (0, 128):
        eh = support.gym_env(128, torch.float64, env_offset=off)
        if kind == "noisy":                                                           # one weight set per half
            half = type(pol)([(w[off // 128:off // 128 + 1], b[off // 128:off // 128 + 1]) for w, b in zip(pol.W, pol.b)],
                             history=pol.history, hidden=pol.hidden, output=pol.output, out_scale=pol.out_scale, out_bias=pol.out_bias)
        else:
            half = pol
        H = _collector(eh, half, cuts, s, _sigma(kind), _sentinel(eh, half))
        _same(A, H, ea, eh, pol, sl=slice(off, off + 128))


# ---------------------------------------------------------------------------------------------------------- 5
def test_invalid_arguments_at_the_c_abi():
    torch = _torch()
    from simglucose_amd import _lib
    e = support.gym_env(128)
    pol = support.constant_policy(0.05)
    st = e.new_policy_state(pol)
    before = {k: getattr(e, k).clone() for k in support.GYM_STATE}
    before.update({k: v.clone() for k, v in st.items()})
    L = e._L

    def structs(on_done="restart"):
        _, p, g, keep = e._collect_structs("collect_mlp", 2, pol, st, None, None, on_done, DAYS, None, None, False, draw=(None, None))
        e._set_trace(p, None, 2)
        return p, g, keep

    def limit(max_minutes=2 * ST, reserved=0):
        lim = _lib.TimeLimit()
        lim.max_minutes, lim.reserved, lim.cut_trace, lim.cut_feat = max_minutes, reserved, None, None
        return lim

    def call(p, g, lim, n_steps=2, minutes=ST):
        with torch.cuda.device(e.device):
            return L.t1d_collect_mlp_limit(e._ctx, C.byref(e._b), C.byref(p), C.byref(g), None, None,
                                           C.byref(lim) if lim is not None else None, n_steps, minutes, e.n_sub, e._stream())

    p, g, keep = structs()
    p0, g0, keep0 = structs("continue")
    g0.on_done = 0
    for what, args, text in (("NULL limit", (p, g, None), b"limit is NULL"), ("max_minutes = 0", (p, g, limit(max_minutes=0)), b"max_minutes"),
                             ("reserved = 1", (p, g, limit(reserved=1)), b"reserved"), ("on_done = 0", (p0, g0, limit()), b"on_done"),
                             ("n_steps * minutes > max_minutes", (p, g, limit(max_minutes=2 * ST - 1)), b"n_steps * minutes")):
        assert call(*args) == -1, what
        assert L.t1d_last_error().startswith(b"t1d_collect_mlp_limit: ") and text in L.t1d_last_error(), (what, L.t1d_last_error())
    assert e.sync() == 0
    for k in support.GYM_STATE:
        assert torch.equal(getattr(e, k), before[k]), k
    for k in st:
        assert torch.equal(st[k], before[k]), k


# ---------------------------------------------------------------------------------------------------------- 6
GAE_SHAPES = [(64, 1), (100, 1), (192, 1), (192, 3)]           # a full wave; a partial one; three waves as one policy and as three
GAE_K = 21                                                     # two groups of eight rows and a short first one
GAMMA_LAMBDA = [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0)]


@functools.lru_cache(maxsize=None)
def _gae_inputs(n, dtype_name):
    """reward, done, value, last_value, truncated, cut_value on the GPU, drawn once per shape with a fixed seed and shared; done
    and truncated with probability 0.15 each, some rows with both, the first and the last row with a cut and without; the
    floating words rounded to the call's type"""
    torch = _torch()
    K = GAE_K
    g = torch.Generator().manual_seed(77 * n + K)
    dt = getattr(torch, dtype_name)
    r = torch.randn(K, n, generator=g, dtype=torch.float64).to(dt)
    v = (3.0 * torch.randn(K, n, generator=g, dtype=torch.float64)).to(dt)
    vl = (3.0 * torch.randn(n, generator=g, dtype=torch.float64)).to(dt)
    vc = (3.0 * torch.randn(n, generator=g, dtype=torch.float64)).to(dt)
    d = (torch.rand(K, n, generator=g) < 0.15).to(torch.uint8)
    t = (torch.rand(K, n, generator=g) < 0.15).to(torch.uint8)
    for row in (0, K - 1):
        t[row, 0], d[row, 0], t[row, 1], d[row, 1], t[row, 2], d[row, 2] = 1, 0, 0, 0, 1, 1
    assert int((d & t).sum()) > 2 and int((t & (1 - d)).sum()) > n
    return tuple(x.cuda().contiguous() for x in (r, d, v, vl, t, vc))


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("n,P", GAE_SHAPES)
def test_gae_against_the_reference(n, P, dtype_name):
    """tests/test_gpu_gae.py's comparison, the row's bootstrap being one more selected word: |adv - ref| <= 4 (K - s) eps
    scale[s], |ret - ref| <= that + eps |ret|.  Two calls give equal bits; the moments are the exact sums of the kernel's own
    advantages to 1e-12 of the sum of magnitudes."""
    torch = _torch()
    from simglucose_amd.controller import gae, gae_reference
    eps = torch.finfo(getattr(torch, dtype_name)).eps
    r, d, v, vl, t, vc = _gae_inputs(n, dtype_name)
    K = GAE_K
    left = torch.arange(K, 0, -1, dtype=torch.float64, device=r.device).unsqueeze(1)
    for gamma, lam in GAMMA_LAMBDA:
        adv, ret, mean, std = gae(r, d, v, vl, gamma=gamma, lam=lam, n_policies=P, moments=True, truncated=t, cut_value=vc)
        ra, rr, scale = gae_reference(r, d, v, vl, gamma=gamma, lam=lam, truncated=t, cut_value=vc)
        ea, er = (adv.double() - ra).abs(), (ret.double() - rr).abs()
        bound = 4 * left * eps * scale
        print("\n[gae_limit %s n=%d P=%d g=%.2f l=%.2f] max |adv - ref| / (eps scale) = %.3f" % (dtype_name, n, P, gamma, lam,
                                                                                                float((ea / (eps * scale)).max())))
        assert bool((ea <= bound).all()) and bool((er <= bound + eps * rr.abs()).all()), (gamma, lam)
        # the cut differs from a plain call: the mask is read
        plain, _ = gae(r, d, v, vl, gamma=gamma, lam=lam, n_policies=P)
        assert not torch.equal(_bits(plain), _bits(adv))
        # moments of the kernel's own advantages
        x = adv.double().reshape(K, P, n // P)
        want_mean = x.mean(dim=(0, 2))
        want_sq = (x * x).mean(dim=(0, 2))
        assert bool(((mean - want_mean).abs() <= 1e-12 * x.abs().mean(dim=(0, 2)) + 1e-300).all())
        assert bool(((std * std + mean * mean - want_sq).abs() <= 1e-11 * want_sq + 1e-300).all())
        again = gae(r, d, v, vl, gamma=gamma, lam=lam, n_policies=P, moments=True, truncated=t, cut_value=vc)
        for a, b in zip((adv, ret, mean, std), again):
            assert torch.equal(_bits(a), _bits(b))
        # without value and done (not the streaming form): the same bound
        adv2, _ = gae(r, None, None, None, gamma=gamma, lam=lam, n_policies=P, truncated=t, cut_value=vc)
        ra2, _, scale2 = gae_reference(r, None, None, None, gamma=gamma, lam=lam, truncated=t, cut_value=vc)
        assert bool(((adv2.double() - ra2).abs() <= 4 * left * eps * scale2).all())


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("n,P", GAE_SHAPES)
def test_gae_with_an_all_zero_mask_is_gae(n, P, dtype_name):
    torch = _torch()
    from simglucose_amd.controller import gae
    r, d, v, vl, t, vc = _gae_inputs(n, dtype_name)
    zero = torch.zeros_like(t)
    nan = torch.full_like(vc, float("nan"))
    for gamma, lam in GAMMA_LAMBDA:
        for args in ((d, v, vl), (None, None, None), (d, None, vl)):
            old = gae(r, *args, gamma=gamma, lam=lam, n_policies=P, moments=True)
            for cv in (vc, nan, None):
                new = gae(r, *args, gamma=gamma, lam=lam, n_policies=P, moments=True, truncated=zero, cut_value=cv)
                for a, b in zip(old, new):
                    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("n,P", GAE_SHAPES)
def test_gae_nothing_behind_a_cut_reaches_the_row_before(n, P, dtype_name):
    """NaN in value[s + 1] behind every cut, and in the cut_value of the envs that are never cut, changes no bit of the rows
    <= s of that env"""
    torch = _torch()
    from simglucose_amd.controller import gae
    r, d, v, vl, t, vc = _gae_inputs(n, dtype_name)
    K = GAE_K
    cut = (t != 0) & (d == 0)
    adv, ret = gae(r, d, v, vl, truncated=t, cut_value=vc)
    v2, vl2, vc2 = v.clone(), vl.clone(), vc.clone()
    v2[1:][cut[:-1]] = float("nan")
    vl2[cut[K - 1]] = float("nan")
    vc2[~cut.any(dim=0)] = float("nan")
    assert int(torch.isnan(v2).sum()) > 0 and int(torch.isnan(vl2).sum()) > 0
    adv2, ret2 = gae(r, d, v2, vl2, truncated=t, cut_value=vc2)
    # A row is clean if its own value is, and the row behind it is clean or cut off by a cut or a done in this row: the rows
    # <= s of every cut at s, up to the next poisoned value of the env
    clean = ~torch.isnan(v2)
    ends = cut | (d != 0)
    for s in range(K - 2, -1, -1):
        clean[s] = clean[s] & (clean[s + 1] | ends[s])
    assert int((clean & cut).sum()) > n // 2 and int(clean.sum()) > K * n // 5           # the comparison is not empty
    assert torch.equal(_bits(adv)[clean], _bits(adv2)[clean]) and torch.equal(_bits(ret)[clean], _bits(ret2)[clean])
    assert not bool(torch.isnan(adv2[clean]).any())


def test_gae_writes_nothing_beyond_its_outputs():
    torch = _torch()
    from simglucose_amd.controller.gae import gae_call
    n, P = 100, 4
    r, d, v, vl, t, vc = _gae_inputs(n, "float64")
    K, pad = GAE_K, 64
    guard = lambda shape, dt=torch.float64: torch.full(shape, -5.0, dtype=dt, device=r.device)
    adv, ret, mom = guard((K * n + 2 * pad,)), guard((K * n + 2 * pad,)), guard((2 * P + 2 * pad,))
    ws = torch.full((16 * P * 1 + 2 * pad,), 0x5A, dtype=torch.uint8, device=r.device)
    ins = [x.clone() for x in (r, d, v, vl, t, vc)]
    gae_call(r, d, v, vl, n_policies=P, adv=adv[pad:pad + K * n].view(K, n), ret=ret[pad:pad + K * n].view(K, n),
             moments=mom[pad:pad + 2 * P].view(P, 2), workspace=ws[pad:pad + 16 * P], truncated=t, cut_value=vc)
    torch.cuda.synchronize()
    for buf, size in ((adv, K * n), (ret, K * n), (mom, 2 * P)):
        assert bool((buf[:pad] == -5.0).all()) and bool((buf[pad + size:] == -5.0).all())
        assert not bool((buf[pad:pad + size] == -5.0).any())
    assert bool((ws[:pad] == 0x5A).all()) and bool((ws[pad + 16 * P:] == 0x5A).all())
    for a, b in zip(ins, (r, d, v, vl, t, vc)):
        assert torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------- 7
def test_end_to_end_the_bootstrap_at_a_cut():
    """gae(truncated, cut_value) on the traces of test 1 with a small critic: in row s* the advantage of a cut env is reward +
    gamma v_cut - v (lambda's term ends at the cut), computed in torch from the same words, within test 6's bound"""
    torch = _torch()
    from simglucose_amd.controller import gae, gae_reference, mlp_pre_output
    A, _, ea, _, s, i0 = _pair("plain", "float64")
    vpol = support.identity_policy(widths=(8, 1), seed=9)
    vparams = vpol.device_params(ea.device, ea.dtype)
    tr = A["tr"]
    K = tr["row"] - 1
    f, rew = tr["features"][1:].contiguous(), tr["reward"][1:].contiguous()
    done, trunc = tr["done"][1:].contiguous(), tr["truncated"][1:].contiguous()
    v = mlp_pre_output(vparams, f, vpol).detach().contiguous()
    v_cut = mlp_pre_output(vparams, A["cut_features"][None].contiguous(), vpol)[0].detach().contiguous()
    v_last = mlp_pre_output(vparams, ea.policy_features(vpol, A["st"])[None], vpol)[0].detach().contiguous()
    gamma, lam = 0.99, 0.95
    adv, ret = gae(rew, done, v, v_last, gamma=gamma, lam=lam, truncated=trunc, cut_value=v_cut)
    _, _, scale = gae_reference(rew, done, v, v_last, gamma=gamma, lam=lam, truncated=trunc, cut_value=v_cut)
    # the last cut of every env is the one cut_features holds: row 2 s* for most, row s* for those that ended in between
    eps = torch.finfo(torch.float64).eps
    row = 2 * s - 1 if s > 2 else s - 1                                               # 0-based row of the last wave of cuts
    cut = trunc[row].bool()
    assert int(cut.sum()) > 0
    want = rew[row] + gamma * v_cut - v[row]
    err = (adv[row] - want).abs()
    assert bool((err[cut] <= 4 * (K - row) * eps * scale[row][cut]).all())
    # an env cut in row s* and not again: its cut_features are row s*'s
    once = trunc[s - 1].bool() & (trunc.sum(dim=0) == 1)
    if int(once.sum()) > 0:
        want = rew[s - 1] + gamma * v_cut - v[s - 1]
        assert bool(((adv[s - 1] - want).abs()[once] <= 4 * (K - s + 1) * eps * scale[s - 1][once]).all())
    assert bool(done[s - 1, i0]) and float((adv[s - 1, i0] - (rew[s - 1, i0] - v[s - 1, i0])).abs()) <= 4 * eps * float(scale[s - 1, i0])
