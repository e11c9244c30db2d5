"""What the test files share: constants, bit-for-bit comparisons, the random policies, the env builders and the collectors'
reference loops.  Imported by bare name (`import support`), as test_gpu_step_trim.py imports test_gpu_parity.  Importing it
touches no device; only the env builders and gpu_torch() ask for one."""
import csv
import functools
import math
import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ST = 3                                   # Dexcom's sample time, minutes
START = 360                              # episodes start at 06:00, so that breakfast and lunch fall inside 160 steps
DAYS = 2
STATE = ("state", "istate", "ar_e", "cgm", "bg", "reward", "done", "lbgi", "hbgi", "risk", "meal", "insulin")
STATE_EXACT = STATE + ("h_carry",)
GYM_STATE = STATE + ("meal_time", "meal_amt", "start_minute", "cgm0")
STATS = ("sum_risk", "min_bg", "max_bg", "n_low", "n_high")
POLICY_STATE = ("cgm_hist", "ins_hist", "prev_meal")
MLP_TRACE = ("bg", "cgm", "cho", "insulin", "action")
EPISODE_STATS = ("ep_return", "ep_length", "last_return", "last_length")


def gpu_torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def kernel_asm():
    """tools/kernel_asm.py, by bare name as the tools import it: the one device compile that every test reading the
    library's assembly shares (kernel_asm().kernels(kernel_asm().device_asm()))"""
    import sys
    if os.path.join(ROOT, "tools") not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_asm
    return kernel_asm


# ------------------------------------------------------------------------------------------------ comparisons
def bits(t):
    """the words of a tensor as integers: equal bit patterns compare equal, also the NaN rows new_trace leaves unwritten"""
    import torch
    t = t.contiguous()
    return t.view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()]) if t.is_floating_point() else t


def _equal(a, b, by):
    """by="bits": the same words (equal NaNs pass, +0.0 against -0.0 fails); by="value": torch.equal (any NaN fails)"""
    import torch
    assert by in ("bits", "value"), by
    return torch.equal(bits(a), bits(b)) if by == "bits" else torch.equal(a, b)


def same_env(a, b, keys=STATE, sl=slice(None), by="bits"):
    """the attributes `keys` of env a, its envs `sl`, are those of env b"""
    for k in keys:
        assert _equal(getattr(a, k)[..., sl], getattr(b, k), by), k


def same_dicts(a, b, keys, sl=slice(None), by="bits"):
    for k in keys:
        assert _equal(a[k][..., sl], b[k], by), k


def same_env_at(a, b, keys, idx, by="bits", what=""):
    """the attributes `keys` of env a (or the entries of dict a) are those of b in the envs `idx` (a tensor of indices
    into the last dimension)"""
    get = (lambda o, k: o[k]) if isinstance(a, dict) else getattr
    for k in keys:
        ta, tb = get(a, k), get(b, k)
        if ta is None and tb is None:
            continue
        assert _equal(ta.index_select(-1, idx), tb.index_select(-1, idx), by), (what, k)


# ------------------------------------------------------------------------------------------------ policies
def random_policy(history=4, widths=(16, 16, 1), n_policies=1, seed=0, hidden="tanh", output="logistic", gain=1.0, bias_gain=None,
                  **kw):
    """layer by layer from one generator: weights gain N(0, 1) / sqrt(fan-in), biases bias_gain 0.1 N(0, 1) (None: as gain)"""
    import torch
    from simglucose_amd.controller.mlp_ctrller import MLPController
    bias_gain = gain if bias_gain is None else bias_gain
    g = torch.Generator().manual_seed(seed)
    layers, n_in = [], 2 * history + 3
    for w in widths:
        layers.append((gain * torch.randn(n_policies, w, n_in, generator=g, dtype=torch.float64) / math.sqrt(n_in),
                       bias_gain * 0.1 * torch.randn(n_policies, w, generator=g, dtype=torch.float64)))
        n_in = w
    # the logistic output spans [0, 0.06] U/min, about four times a basal rate and far below the pump's 0.5 U/min
    kw.setdefault("out_scale", 0.06)
    return MLPController(layers, history=history, hidden=hidden, output=output, **kw)


# for t1d_mlp_grad and t1d_mlp_loss: y itself is the output, and the biases do not follow `gain`
identity_policy = functools.partial(random_policy, output="identity", bias_gain=1.0, out_scale=1.0, out_bias=0.0)


def constant_policy(basal, history=4):
    """a one-layer net with zero weights and identity output: `basal` U/min whatever it sees"""
    import torch
    from simglucose_amd.controller.mlp_ctrller import MLPController
    return MLPController([(torch.zeros(1, 2 * history + 3, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))],
                         history=history, output="identity", out_scale=1.0, out_bias=basal)


def hypo_leaning_policies(P, seed=11, **kw):
    """small random weights around a constant 0.05 U/min: episodes end low"""
    kw.setdefault("history", 4); kw.setdefault("widths", (8, 1))
    return random_policy(n_policies=P, seed=seed, output="identity", gain=0.02, out_scale=1.0, out_bias=0.05, **kw)


def mlp_struct(widths=(8, 8, 1), history=4, n_policies=2, envs_per_policy=64, params=0x1000):
    """a host-side t1d_mlp for the argument checks: the network's fields set, `params` an address nothing reads"""
    from simglucose_amd import _lib
    from simglucose_amd.controller.mlp_ctrller import MLPController
    p = _lib.Mlp()
    p.history, p.n_layers = history, len(widths)
    for k in range(4):
        p.width[k] = widths[k] if k < len(widths) else 0
    p.hidden_act = 0
    p.n_policies, p.envs_per_policy = n_policies, envs_per_policy
    p.n_params = MLPController.count_params(history, widths)
    p.params = params
    return p


# ------------------------------------------------------------------------------------------------ accumulators
def stats(e):
    torch = gpu_torch()
    z = lambda dt=e.dtype: torch.zeros(e.n, dtype=dt, device=e.device)
    return {"sum_risk": z(), "min_bg": z() + 1000.0, "max_bg": z(), "n_low": z(torch.int32), "n_high": z(torch.int32)}


def episode_stats(e):
    torch = gpu_torch()
    z = lambda dt=e.dtype: torch.zeros(e.n, dtype=dt, device=e.device)
    return {"ep_return": z(), "ep_length": z(torch.int32), "last_return": z(), "last_length": z(torch.int32)}


# ------------------------------------------------------------------------------------------------ envs
def plain_env(**kw):
    """BatchedT1DSimEnv(**kw) on a machine that has a GPU; plain_env(integrator="dopri5", ...) is the exact mode"""
    gpu_torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    return BatchedT1DSimEnv(**kw)


CLOSED_LOOP = {"rollout_pid": (1, 0.0, 0.0, 0.0), "rollout_bb": (1,), "rollout_mlp": (1, None), "collect_mlp": (1, None),
               "collect_pid": (1, 0.0, 0.0, 0.0), "collect_bb": (1,)}         # the fixed-step methods with their shortest calls
CLOSED_LOOP_EXACT = ("rollout_pid", "rollout_bb", "rollout_mlp", "collect_mlp")  # ... and those with a *_dopri5 sibling


def mode_refusal(method, integrator):
    """The T1DError text with which `method` turns away an env of the other mode.  The env is a bare object that has its
    integrator and nothing else, so a method that reads anything before it refuses ends in an AttributeError instead.
    Needs no device."""
    import pytest
    from simglucose_amd import _lib
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    e = object.__new__(BatchedT1DSimEnv)
    e.integrator = integrator
    with pytest.raises(_lib.T1DError) as err:
        getattr(e, method)(*CLOSED_LOOP[method[:-len("_dopri5")] if method.endswith("_dopri5") else method])
    return str(err.value)


def meal_day_env(n, dtype, env_offset=0, seed=5, meals=True, start=None, **kw):
    """all 30 patients, a random-meal day from START (or from `start`: int32 [n] minute of day per env), reset"""
    torch = gpu_torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    from simglucose_amd.scenario_batch import random_meal_tables
    pid = (np.arange(n) + env_offset) % 30
    e = BatchedT1DSimEnv(patient=pid, sensor="Dexcom", dtype=dtype, seed=seed, env_offset=env_offset, **kw)
    e.start_minute = torch.full((n,), START, dtype=torch.int32, device=e.device) if start is None else \
        torch.as_tensor(start, dtype=torch.int32).to(e.device).contiguous()
    if meals:
        e.set_meals(*random_meal_tables(n, days=1, start_minute_of_day=e.start_minute, seed=seed, dtype=dtype, env_offset=env_offset))
    e.reset()
    return e


def gym_env(n, dtype=None, seed=3, env_offset=0, exact=False, sensor_row=None, use_pump=True):
    """child#001 / adult#001 alternating, random initial glucose, Philox noise, every env in episode 0 of the device's own
    episode stream (started through restart_done); dtype None: fp64.  n_sub = 4 and integrator = None are the constructor's
    defaults, and the exact mode ignores n_sub.  sensor_row: a custom row in place of Dexcom's."""
    torch = gpu_torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    e = BatchedT1DSimEnv(patient=["child#001", "adult#001"] * (n // 2), sensor="Dexcom", pump="Insulet", dtype=dtype or torch.float64,
                         n_sub=4, seed=seed, env_offset=env_offset, noise="philox", random_init_bg=True,
                         integrator="dopri5" if exact else None, sensor_row=sensor_row, use_pump=use_pump)
    e.restart_done(mask=torch.ones(n, dtype=torch.uint8, device=e.device), days=DAYS, reset_outputs=True)
    return e


def exact_inputs(n, K, seed=3):
    """per-env inputs that do not depend on the env's index in a batch: patient row, host normals, a meal table"""
    rs = np.random.RandomState(seed)
    pid = np.arange(n) % 30
    z = rs.randn(1 + 10 * (2 + K * ST // 150), n)
    mt = np.sort(rs.choice(np.arange(2, max(8, K * ST - 2)), size=(n, 4)), axis=1).T.copy()      # [4][n], ascending
    for j in range(1, 4):                                            # at most one entry per minute
        mt[j] = np.maximum(mt[j], mt[j - 1] + 1)
    ma = rs.uniform(15.0, 90.0, size=(4, n))
    return pid, z, mt.astype(np.int64), ma


def host_noise_env(pid, z, mt, ma, cols=None, exact=True, start=START, **kw):
    """Dexcom, host normals and explicit meal tables (exact_inputs), the columns `cols` of them; start=None: no start_minute"""
    torch = gpu_torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    if cols is not None:
        pid, z, mt, ma = pid[cols], z[:, cols], mt[:, cols], ma[:, cols]
    e = BatchedT1DSimEnv(patient=pid, sensor="Dexcom", noise="host", normals=z, integrator="dopri5" if exact else None, **kw)
    e.set_meals(torch.as_tensor(mt), torch.as_tensor(ma))
    if start is not None:
        e.start_minute = torch.full((e.n,), start, dtype=torch.int32, device=e.device)
    e.reset()
    return e


def basal_of(pid):
    from simglucose_amd import params
    _, tab = params.patient_table()
    return tab[pid, params.P_COL["u2ss"]] * tab[pid, params.P_COL["BW"]] / 6000.0


def dense_cho(mt, ma, sample, minutes):
    """the meal tables of the envs `sample` as grams per minute [minutes, len(sample)], for the oracle"""
    t_s, a_s = mt[:, sample].cpu().numpy().astype(np.int64), ma[:, sample].double().cpu().numpy()
    cho = np.zeros((minutes, len(sample)))
    for j in range(len(sample)):
        for tt, aa in zip(t_s[:, j], a_s[:, j]):
            if 0 <= tt < minutes:
                cho[tt, j] = aa
    return cho


# ------------------------------------------------------------------------------------------------ files
def golden_hist(name):
    """a history CSV of tests/golden -> ({column: values, NaN where empty}, the Time column)"""
    with open(os.path.join(GOLDEN, name), newline="") as f:
        rows = list(csv.DictReader(f))
    return {k: np.array([float(r[k]) if r[k] else np.nan for r in rows]) for k in rows[0] if k != "Time"}, \
        [r["Time"] for r in rows]


def header_fields(name):
    """the fields of `typedef struct name` in include/t1d.h -> [(field, C type, is a pointer, array length)]"""
    src = open(os.path.join(ROOT, "include", "t1d.h")).read()
    body = src[src.index("typedef struct %s {" % name):src.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct %s {" % name, "")
    out = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        ctype = re.match(r"(const\s+)?(\w+)", stmt).group(2)
        for part in stmt.split(","):
            m = re.search(r"([A-Za-z_0-9]+)(\[(\d+)\])?\s*$", part.strip())
            out.append((m.group(1), ctype, "*" in stmt, int(m.group(3) or 1)))
    return out


# ------------------------------------------------------------------------------------------------ the collectors' references
# One body for collect_mlp and collect_mlp_dopri5: `exact` picks the entry points.  The right-hand-side counts (nfev) ride
# along; a fixed-step env has none and its sums stay 0.
TRACES = MLP_TRACE + ("reward", "done", "eps", "features")


def loop_of_entry_points(e, pol, K, acc, tr, term, es, exact=False, st=None, restart=True):
    """what a trainer does without the collector: per step rollout_mlp(1) or rollout_mlp_dopri5(1), restart_done, the torch
    reset of the policy state -> policy state, low endings, high endings, summed nfev.  st: the policy state of an earlier
    call, to go on from it; restart=False: no restart_done (term and es are not used), the loop a multi-step roll-out is"""
    torch = gpu_torch()
    rollout = e.rollout_mlp_dopri5 if exact else e.rollout_mlp
    st = e.new_policy_state(pol) if st is None else st
    low = high = 0
    zero = torch.zeros((), dtype=e.dtype, device=e.device)
    nf = torch.zeros(e.n, dtype=torch.int64, device=e.device)
    for _ in range(K):
        row = tr["row"]
        rollout(1, pol, policy_state=st, stats=acc, trace=tr)
        nf += e.nfev if exact else 0
        done = e.done.bool()
        tr["reward"][row] = e.reward; tr["done"][row] = e.done
        low = low + (done & (e.bg < 70)).sum(); high = high + (done & (e.bg > 350)).sum()
        if not restart:
            continue
        e.restart_done(days=DAYS, terminal_obs=term, episode_stats=es)
        st["cgm_hist"].copy_(torch.where(done, e.cgm, st["cgm_hist"]))           # new_policy_state for the envs that restarted
        st["ins_hist"].copy_(torch.where(done, zero, st["ins_hist"]))
        st["prev_meal"].copy_(torch.where(done, zero, st["prev_meal"]))
    assert e.sync() == 0
    return st, int(low), int(high), nf


def restart_pair(pol, cuts, dtype=None, exact=False, seed=3, sensor_row=None, **kw):
    """A: the collector in launches of `cuts` steps; B: the loop of existing entry points; equal bit for bit
    -> what happened in B: restarts per env, low endings, high endings"""
    torch = gpu_torch()
    n, K = 256, sum(cuts)
    cols = MLP_TRACE + ("reward", "done", "eps")
    A, B = (gym_env(n, dtype, seed, exact=exact, sensor_row=sensor_row) for _ in range(2))
    collect = A.collect_mlp_dopri5 if exact else A.collect_mlp
    z = lambda: torch.zeros(n, dtype=A.dtype, device=A.device)
    sa, ta, terma, esa = stats(A), A.new_trace(K, columns=cols), z(), episode_stats(A)
    sb, tb, termb, esb = stats(B), B.new_trace(K, columns=cols[:7]), z(), episode_stats(B)
    sta = None
    nfa = torch.zeros(n, dtype=torch.int64, device=A.device)
    for k in cuts:
        sta = collect(k, pol, policy_state=sta, stats=sa, trace=ta, on_done="restart", days=DAYS, terminal_obs=terma,
                      episode_stats=esa, **kw)
        nfa += A.nfev if exact else 0
    assert A.sync() == 0
    stb, low, high, nfb = loop_of_entry_points(B, pol, K, sb, tb, termb, esb, exact)
    same_env(B, A, keys=(STATE_EXACT if exact else STATE) + ("meal_time", "meal_amt", "start_minute", "episode", "cgm0"))
    same_dicts(stb, sta, POLICY_STATE)
    same_dicts(sb, sa, STATS)
    same_dicts(esb, esa, EPISODE_STATS)
    assert torch.equal(bits(termb), bits(terma))
    same_dicts(tb, ta, cols[:7])
    assert torch.equal(nfb, nfa)
    assert bool((ta["eps"][1:] == 0).all())
    assert A._clock is None
    return (B.episode - 1).cpu().numpy(), low, high


def noisy_run(e, pol, sigma, warm, chunks, explore_seed=99, exact=False, **kw2):
    """`warm` steps in one launch (far enough for episodes to end in what follows), then the traced chunks (**kw2 to them)
    -> policy state, accumulators, episode statistics with terminal_obs and the summed nfev, trace"""
    torch = gpu_torch()
    collect = e.collect_mlp_dopri5 if exact else e.collect_mlp
    acc, es, term = stats(e), episode_stats(e), torch.zeros(e.n, dtype=e.dtype, device=e.device)
    kw = dict(sigma=sigma, explore_seed=explore_seed, stats=acc, on_done="restart", days=DAYS, terminal_obs=term, episode_stats=es)
    st = collect(warm, pol, **kw)
    tr = e.new_trace(sum(chunks), columns=TRACES, history=pol.history)
    nf = torch.zeros(e.n, dtype=torch.int64, device=e.device)
    for ch in chunks:
        collect(ch, pol, policy_state=st, trace=tr, **kw, **kw2)
        nf += e.nfev if exact else 0
    assert e.sync() == 0
    es["terminal_obs"] = term
    es["nfev"] = nf
    return st, acc, es, tr


def draw_of_pair(m):
    """the draw index of t1d_philox_normals whose value is philox_pair(.., pair = m).x"""
    return np.where(m >= 3, 1 + 10 * ((m - 3) // 5) + 2 * ((m - 3) % 5), 0)


# ------------------------------------------------------------------------------------------------ the sensor grid
# Custom sample times (test_sensor_grid_host.py, test_gpu_sensor_grid.py): the Dexcom row with another sample_time, 150 envs
# (two full 64-env chunks and a partial one), host normals, one 60 g meal in every third env, an action that moves with the
# step.  Importing and building the inputs touches no device.
GRID_N = 150
GRID_STS = (2, 4, 7, 10, 15, 20, 30, 50, 100, 150)           # the sample times the device runs
GRID_STS_HOST = GRID_STS + (60, 75)                          # ... and the oracle alone
GRID_OUT = ("cgm", "bg", "reward", "risk", "done")


def grid_sensor_row(st):
    """the Dexcom row with column 5 (sample_time) replaced"""
    from simglucose_amd import params
    row = np.array(params.sensor_row("Dexcom"), dtype=np.float64)
    row[5] = st
    return row


@functools.lru_cache(maxsize=None)
def grid_inputs(st, n=GRID_N, seed=17, feed=3):
    """-> dict: row, pid, S = samples per noise block, K steps (the reset's two samples and K steps open a third block),
    z = host normals [1 + 10 ceil((K + 2) / S), n], mt / ma = the meal table [1, n] (60 g at the first minute of step 1 in
    every `feed`-th env), cho = the same meals per minute [K st, n], basal [n]"""
    from simglucose_amd import _lib
    S = 150 // st
    K = max(5, 2 * S + 1)
    pid = np.arange(n) % 30
    z = np.random.RandomState(seed).randn(1 + 10 * math.ceil((K + 2) / S), n)
    fed = np.arange(n) % feed == 0
    mt = np.where(fed, st, _lib.MEAL_UNUSED).astype(np.int64)[None, :]
    ma = np.where(fed, 60.0, 0.0)[None, :]
    cho = np.zeros((K * st, n))
    cho[st, fed] = 60.0
    return dict(st=st, row=grid_sensor_row(st), n=n, pid=pid, S=S, K=K, z=z, mt=mt, ma=ma, cho=cho, basal=basal_of(pid))


def grid_action(inp, k):
    return inp["basal"] * (0.5 + 0.5 * (k % 3))


def grid_oracle_run(st, integrator="split_adaptive", z=None, n=GRID_N, feed=3):
    """the oracle over the grid's inputs (z: other normals, e.g. the device's Philox draws) -> dict: GRID_OUT as arrays
    [K + 1, n] (row 0 = after reset; reward and risk of row 0 as reset leaves them), x [13, n], t, last_cgm, level_count"""
    from oracle import t1d_oracle as O
    inp = grid_inputs(st, n, feed=feed)
    orc = O.OracleEnv(inp["pid"], normals=inp["z"] if z is None else z, integrator=integrator, n_sub=4,
                      sensor_row_override=inp["row"])
    rows = [orc.reset()]
    for k in range(inp["K"]):
        rows.append(orc.step(grid_action(inp, k), None, inp["cho"][k * st:(k + 1) * st]))
    out = {key: np.stack([r[key] for r in rows]) for key in GRID_OUT}
    out.update(x=orc.x.copy(), t=orc.t.copy(), last_cgm=orc.last_cgm.copy(), level_count=orc.level_count.copy())
    return out


@functools.lru_cache(maxsize=None)
def grid_oracle(st, integrator="split_adaptive"):
    """grid_oracle_run on the grid's own normals, computed once per sample time and integrator; treat as read-only"""
    return grid_oracle_run(st, integrator)


def uneven_cuts(st, total):
    """launch lengths that are not the sample time: (1, 2, st + 1, 2 st, 1, st - 1, 3 st + 2) repeated and cut off at
    `total` - st, then one launch of st minutes.  The last launch is a whole step because prev_risk is the risk index of the
    last launch's mean CGM: it compares with a run in steps of st minutes only where the two last launches span the same
    minutes (at st = 7 the plain cut-off would end on a launch of one minute)."""
    pattern, cuts, k = (1, 2, st + 1, 2 * st, 1, st - 1, 3 * st + 2), [], 0
    while sum(cuts) < total - st:
        cuts.append(min(pattern[k % len(pattern)], total - st - sum(cuts)))
        k += 1
    return cuts + [st]


def whole_pair_launch(st, cuts):
    """the first launch of 2 st minutes in `cuts` that starts on a step boundary -> (its index, the index of the first of
    the two steps of st minutes it spans), None if there is none"""
    t0 = 0
    for j, m in enumerate(cuts):
        if m == 2 * st and t0 % st == 0:
            return j, t0 // st
        t0 += m
    return None


def grid_env(st, n=GRID_N, options=(), z=None, meals=True, feed=3, **kw):
    """the device env of the grid: custom sensor row, host normals (noise="philox" in kw: none), the meal table, `options`
    as (name, value) pairs set before reset(), reset"""
    torch = gpu_torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    inp = grid_inputs(st, n, feed=feed)
    if kw.get("noise", "host") == "host":
        kw.update(noise="host", normals=inp["z"] if z is None else z)
    kw.setdefault("n_sub", 4)
    e = BatchedT1DSimEnv(patient=inp["pid"], sensor="Dexcom", sensor_row=inp["row"], **kw)
    for name, value in options:
        e.set_option(name, value)
    if meals:
        e.set_meals(torch.as_tensor(inp["mt"]), torch.as_tensor(inp["ma"]))
    e.reset()
    return e


def grid_level2_lanes(st, n, feed=1):
    """per step of the grid's oracle run: how many envs spend at least one minute at level 2 of the step-size rule.  The
    patient's minutes do not depend on the sensor noise, and action and meal depend on the env through its patient and on
    whether it is fed alone: one single-env oracle per (patient, fed) says it for every env -> int array [K]"""
    from oracle import t1d_oracle as O
    inp = grid_inputs(st, n, feed=feed)
    K, count = inp["K"], np.zeros(inp["K"], dtype=np.int64)
    seen = {}
    for i in range(n):
        key = (int(inp["pid"][i]), bool(inp["cho"][st, i] > 0))
        if key not in seen:
            orc = O.OracleEnv(inp["pid"][i:i + 1], normals=inp["z"][:, i:i + 1], integrator="split_adaptive", n_sub=4,
                              sensor_row_override=inp["row"])
            orc.reset()
            flags = np.zeros(K, dtype=bool)
            for k in range(K):
                before = int(orc.level_count[2])
                orc.step(grid_action(inp, k)[i:i + 1], None, inp["cho"][k * st:(k + 1) * st, i:i + 1])
                flags[k] = int(orc.level_count[2]) > before
            seen[key] = flags
        count += seen[key]
    return count


# ------------------------------------------------------------------------------------------------ status word, non-finite data
# test_status_host.py, test_gpu_status.py: 150 envs (two full 64-env chunks and a partial one), all 30 patients, host normals,
# 70 g at the first minute of step `meal_step` in every `feed`-th env, grid_action's moving basal.  Two steps, then one state
# word of three lanes is made non-finite, then three more steps.  Importing and building the inputs touches no device.
STATUS_N = 150
STATUS_PRE, STATUS_POST = 2, 3
POISONS = {"x12_nan": (12, float("nan")), "x0_nan": (0, float("nan")), "x5_nan": (5, float("nan")), "x12_inf": (12, float("inf"))}
STATUS_SCHEMES = {False: "split_adaptive", True: "dopri"}       # exact mode? -> the oracle's integrator


@functools.lru_cache(maxsize=None)
def status_inputs(sensor="Navigator", n=STATUS_N, feed=3, meal_step=1, seed=23):
    """-> dict: st, pid, z = host normals [31, n], mt / ma = the meal table [1, n], cho = the same meal per minute [K st, n],
    basal [n], vmin / vmax = the sensor's range, K = STATUS_PRE + STATUS_POST"""
    from simglucose_amd import _lib, params
    row = np.array(params.sensor_row(sensor), dtype=np.float64)
    st, K = int(row[5]), STATUS_PRE + STATUS_POST
    pid = np.arange(n) % 30
    fed = np.arange(n) % feed == 0
    cho = np.zeros((K * st, n))
    cho[meal_step * st, fed] = 70.0
    return dict(sensor=sensor, st=st, n=n, K=K, pid=pid, z=np.random.RandomState(seed).randn(31, n), fed=fed,
                mt=np.where(fed, meal_step * st, _lib.MEAL_UNUSED).astype(np.int64)[None, :], ma=np.where(fed, 70.0, 0.0)[None, :], cho=cho,
                basal=basal_of(pid), vmin=float(row[6]), vmax=float(row[7]))


def status_oracle_env(inp, integrator, cols=None):
    from oracle import t1d_oracle as O
    cols = slice(None) if cols is None else cols
    return O.OracleEnv(inp["pid"][cols], sensor=inp["sensor"], normals=inp["z"][:, cols], integrator=integrator, n_sub=4)


def oracle_step(orc, basal, bolus, cho):
    """OracleEnv.step that reports a solver that gave up instead of raising: the C side has written the state (an env whose
    solver gives up keeps its last accepted one) and every output by then -> (outputs, gave up?)"""
    try:
        return orc.step(basal, bolus, cho), False
    except RuntimeError:
        return {k: v.copy() for k, v in orc.out.items()}, True


@functools.lru_cache(maxsize=None)
def status_lanes(sensor="Navigator", n=STATUS_N, feed=3, meal_step=1):
    """the three lanes that get the non-finite word: one in chunk 0, one in the partial chunk, and the first env of chunk 1
    (failing that, of the rest) that the oracle's step-size rule puts at level 2 in the first minute after the STATUS_PRE
    steps.  Found as grid_level2_lanes finds them: the patient's minutes depend on the env through its patient and on whether
    it is fed alone, and not on the sensor, so one single-env oracle per (patient, fed) with a one-minute sensor says it."""
    from oracle import t1d_oracle as O
    inp = status_inputs(sensor, n, feed, meal_step)
    st, t0 = inp["st"], STATUS_PRE * inp["st"]
    first, last = 5, n - 9
    seen = {}
    for i in list(range(64, min(n, 128))) + list(range(0, 64)) + list(range(128, n)):
        key = (int(inp["pid"][i]), bool(inp["fed"][i]))
        if key not in seen:
            orc = O.OracleEnv(inp["pid"][i:i + 1], sensor="Navigator", normals=inp["z"][:, i:i + 1], integrator="split_adaptive", n_sub=4)
            assert orc.sample_time == 1
            orc.reset()
            for m in range(t0):
                orc.step(grid_action(inp, m // st)[i:i + 1], None, inp["cho"][m:m + 1, i:i + 1])
            before = int(orc.level_count[2])
            orc.step(grid_action(inp, STATUS_PRE)[i:i + 1], None, inp["cho"][t0:t0 + 1, i:i + 1])
            seen[key] = int(orc.level_count[2]) > before
        if seen[key] and i not in (first, last):
            return (first, last, i)
    raise AssertionError("no lane at level 2 in the minute after the first %d steps" % STATUS_PRE)


@functools.lru_cache(maxsize=None)
def status_oracle(sensor="Navigator", exact=False, poison=None, n=STATUS_N, feed=3, meal_step=1):
    """The oracle over the status inputs (exact: its DOPRI5, else the default scheme); poison: a key of POISONS written into
    status_lanes after STATUS_PRE steps, None: the clean run.  Computed once per argument set; treat as read-only.
    -> dict: lanes; per step after the poison, arrays [STATUS_POST, n]: x12_bad (stored x[12] not finite), bg_bad, done,
    last_cgm, gave_up (bool [STATUS_POST]); x = the final state"""
    inp = status_inputs(sensor, n, feed, meal_step)
    st = inp["st"]
    lanes = status_lanes(sensor, n, feed, meal_step)
    orc = status_oracle_env(inp, STATUS_SCHEMES[exact])
    orc.reset()
    rows = {k: [] for k in ("x12_bad", "bg_bad", "done", "last_cgm", "gave_up", "bg", "insulin")}
    for k in range(inp["K"]):
        if k == STATUS_PRE and poison is not None:
            word, value = POISONS[poison]
            orc.x[word, list(lanes)] = value
        r, gave_up = oracle_step(orc, grid_action(inp, k), None, inp["cho"][k * st:(k + 1) * st])
        assert k >= STATUS_PRE or not gave_up
        if k >= STATUS_PRE:
            rows["x12_bad"].append(~np.isfinite(orc.x[12])); rows["bg_bad"].append(~np.isfinite(r["bg"]))
            rows["done"].append(r["done"].copy()); rows["last_cgm"].append(orc.last_cgm.copy()); rows["gave_up"].append(gave_up)
            rows["bg"].append(r["bg"]); rows["insulin"].append(r["insulin"])
    out = {k: np.stack(v) for k, v in rows.items()}
    out.update(lanes=lanes, x=orc.x.copy())
    return out


def status_env(sensor="Navigator", n=STATUS_N, feed=3, options=(), dtype=None, exact=False, z=None, meal_step=1, make=None, inputs=None, **kw):
    """the device env of the status inputs: host normals (z: others), the meal table, `options` as (name, value) pairs
    set before reset(), reset.  make: what builds the env from BatchedT1DSimEnv's arguments (test_gpu_parity._env with its
    variant bound, for the generic kernel's other schemes), None: BatchedT1DSimEnv itself.  inputs: what builds the inputs
    from (sensor, n, feed, meal_step), None: status_inputs (gut_inputs: the same with more meals)"""
    torch = gpu_torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    inp = (inputs or status_inputs)(sensor, n, feed, meal_step)
    e = (make or BatchedT1DSimEnv)(patient=inp["pid"], sensor=sensor, noise="host", normals=inp["z"] if z is None else z, n_sub=4,
                                   dtype=dtype or torch.float64, integrator="dopri5" if exact else None, **kw)
    for name, value in options:
        e.set_option(name, value)
    e.set_meals(torch.as_tensor(inp["mt"]), torch.as_tensor(inp["ma"]))
    e.reset()
    return e


# ------------------------------------------------------------------------------------------------ model branch points
# test_edge_states_host.py, test_gpu_edge_states.py: the status inputs again, but what is written after the STATUS_PRE steps
# is finite: states at which the model itself branches.  One function edits the oracle's state and the device's.
EDGE_LANES = {                                   # kind -> lanes: each kind in chunk 0, in chunk 1 and in the partial chunk
    "held3": (64, 70, 101, 149, 12),             # x3 < 0: the reference holds it (t1d_oracle.c:58)
    "cross_m1": (20, 90, 140),                   # x3 falls through 0 in the first minute after the edit ...
    "cross_m2": (22, 92, 142),                   # ... in the second: the middle minute of a Dexcom step
    "neg4": (3, 17, 40, 130, 100),               # x4 < 0, held (:63)
    "neg12": (5, 17, 63, 131, 80),               # x12 < 0, held (:82): BG < 0, `done`
    "ke2_down": (7, 71, 133),                    # x3 falls through the renal threshold ke2 in the first minute (:55)
    "ke2_up": (9, 72, 135),                      # ... rises through it
    "egp_neg": (11, 74, 137),                    # EGPt < 0, clamped (:57)
    "done_high": (40, 100, 145),                 # BG a little above 350 mg/dL (lanes 40 and 100: also neg4)
    "done_low": (42, 104, 147),                  # BG a little below 70 mg/dL
}
EDGE_CROSSING = {"cross_m1": 1, "cross_m2": 2}   # kind -> the minute after the edit in which x3 reaches 0
EDGE_HELD = {"held3": (3, -0.25), "neg4": (4, -1e-3), "neg12": (12, -2e-3)}     # kind -> the word the reference holds, its value
EDGE_SNAP = -1e-10                               # where the fixed-step scheme leaves an x3 that a step took below 0 (o_knob[3])
EDGE_OUT = GRID_OUT + ("last_cgm", "x")
GUT_WORDS = ("planned", "last_qsto", "last_food")    # the meal bookkeeping beside the state (t1dpatient.py:82-107, 222-236)


def edge_states(x, pid):
    """x: the state [13, n] of the oracle (numpy) or of a device env (torch), n >= 150, edited in place after the STATUS_PRE
    steps; pid: the patient row per env.  Every value is formed on the host in fp64 and written as a Python float, so the
    oracle and an fp64 env receive the same words.  -> EDGE_LANES.
    done_high and done_low write x3 along with x12: x12 follows x3 at ksc (0.06 to 0.2 per minute), so a lone x12 = 351 Vg is
    back at 332 to 335 mg/dL, and a lone 69.5 Vg at 76 to 78, by the end of the first minute and `done` is never raised
    (test_edge_states_host.py shows it on the oracle).  With x3 = 380 Vg (62 Vg) beside it, BG stays within 3 mg/dL of the
    threshold for the first step after the edit, beyond it in some lanes and short of it in others."""
    from simglucose_amd import params
    _, tab = params.patient_table()
    pid = np.asarray(pid)
    ke2, vg = tab[pid, params.P_COL["ke2"]], tab[pid, params.P_COL["Vg"]]

    def put(word, i, value):
        x[word][i] = float(value)

    L = EDGE_LANES
    for kind, (word, value) in EDGE_HELD.items():
        for i in L[kind]:
            put(word, i, value)
    for i in L["cross_m1"] + L["cross_m2"]:
        put(3, i, 0.05 if i in L["cross_m1"] else 1.4); put(4, i, 0.0); put(8, i, 500.0)
    for i in L["ke2_down"]:
        put(3, i, ke2[i] + 0.3)
    for i in L["ke2_up"]:
        put(3, i, ke2[i] - 0.3); put(4, i, float(x[4][i]) * 1.5)
    for i in L["egp_neg"]:
        put(8, i, 500.0)
    for i in L["done_high"]:
        put(12, i, 351.0 * vg[i]); put(3, i, 380.0 * vg[i])
    for i in L["done_low"]:
        put(12, i, 69.5 * vg[i]); put(3, i, 62.0 * vg[i])
    return L


def edge_lanes(*kinds):
    """the lanes of the given kinds, sorted, each once"""
    return sorted({i for k in kinds for i in EDGE_LANES[k]})


def edge_oracle_run(sensor="Navigator", integrator="split_adaptive", feed=3, meal_step=1, after_edit=None, minutes=False,
                    inputs=None, edit=None):
    """The oracle over the status inputs with edge_states written after STATUS_PRE steps (after_edit(x): a further edit of
    the state, in place).  minutes: the same patients' minutes under a one-minute sensor, minute by minute, as status_lanes
    drives them -- the patient does not depend on the sensor.  inputs, edit: gut_inputs and gut_states in place of
    status_inputs and edge_states (edit(orc, pid) -> the lane table).
    -> dict: EDGE_OUT and the meal words GUT_WORDS after every step (minute) as arrays [K, n] (x: [K, 13, n]), x_edit = the
    state as written, level2 = lane-minutes at level 2 per step [K], final = the last x, lanes = the lane table.  A solver
    that gives up raises."""
    from oracle import t1d_oracle as O
    inp = (inputs or status_inputs)(sensor, STATUS_N, feed, meal_step)
    st = inp["st"]
    if minutes:
        orc = O.OracleEnv(inp["pid"], sensor="Navigator", normals=inp["z"], integrator=integrator, n_sub=4)
        assert orc.sample_time == 1
    else:
        orc = status_oracle_env(inp, integrator)
    per = st if minutes else 1                                   # oracle steps per step of the inputs
    orc.reset()
    x_reset = orc.x.copy()
    rows = {k: [] for k in EDGE_OUT + GUT_WORDS + ("level2",)}
    x_edit, lanes = None, EDGE_LANES
    for k in range(inp["K"] * per):
        if k == STATUS_PRE * per:
            lanes = edge_states(orc.x, inp["pid"]) if edit is None else edit(orc, inp["pid"])
            if after_edit is not None:
                after_edit(orc.x)
            x_edit = orc.x.copy()
        before = int(orc.level_count[2])
        r = orc.step(grid_action(inp, k // per), None, inp["cho"][k:k + 1] if minutes else inp["cho"][k * st:(k + 1) * st])
        for key in GRID_OUT:
            rows[key].append(r[key].copy())
        rows["last_cgm"].append(orc.last_cgm.copy()); rows["x"].append(orc.x.copy())
        for key in GUT_WORDS:
            rows[key].append(getattr(orc, key).copy())
        rows["level2"].append(int(orc.level_count[2]) - before)
    out = {k: np.stack(v) for k, v in rows.items()}
    out.update(x_reset=x_reset, x_edit=x_edit, final=orc.x.copy(), lanes=lanes)
    return out


@functools.lru_cache(maxsize=None)
def edge_oracle(sensor="Navigator", integrator="split_adaptive", feed=3, meal_step=1):
    """edge_oracle_run, computed once per argument set; treat as read-only"""
    return edge_oracle_run(sensor, integrator, feed, meal_step)


# ------------------------------------------------------------------------------------------------ gastric-emptying edge states
# test_gut_states_host.py, test_gpu_gut_states.py: the status inputs with more meals, and after the STATUS_PRE steps an edit of
# the gut words (x0, x1, last_qsto, last_food and, on the device, the dbar row beside them) that takes the tanh pair of
# t1dpatient.py:135-142 to arguments no trajectory from an empty stomach reaches.  The edited lanes are unfed lanes of the
# feed = 3 inputs (neither eating nor with a meal planned: the one-minute kernels read `dbar` in place of the two words
# there), but for the two transition kinds: an argument moves by more than the step-size rule's kMove = 4 in a minute only
# while the lane eats (emptying moves qsto by kgut x1 < 0.07 qsto a minute), so these sit in fed lanes, which are eating at
# the edit: last_food = 1 g becomes 6 g in the next minute and qsto is b (d) times 6 g.  A 70 g meal is eaten for 14 minutes, longer than the minutes left after the edit, so a lane that the table feeds
# is still eating when a further meal arrives and takes no new last_qsto (meal_while_eating); the second_meal lanes get their
# full stomach by the edit instead -- 45 g in transit of a finished 70 g meal -- and then 30 g through the table.
GUT_LANES = {                                    # kind -> lanes: each kind in chunk 0, in chunk 1 and in the partial chunk
    "no_dbar": (1, 65, 130),                     # grams in the stomach, Dbar = 0: kgut = kmax (:142)
    "overfull": (4, 32, 64, 128),                # qsto = 30 Dbar (4, 64: patient row 4, b = 0.988; 32: row 2, the smallest b)
    "deep_negative": (34, 26, 94, 86, 146),      # qsto = 0 (34, 86) or 0.1 g (the others), Dbar = 70 g, b >= 0.952
    "at_transition_b": (6, 69, 132),             # fed lanes: qsto = b Dbar exactly at the start of the first minute ...
    "at_transition_d": (9, 72, 135),             # ... = d Dbar exactly, Dbar = 6 g and growing by 5 g a minute
    "tiny_dbar": (10, 73, 134),                  # Dbar = 50 mg, 40 mg in the stomach
    "huge_in_transit": (11, 74, 136),            # last_food = 400 g, 370 g in the stomach
    "residue": (13, 76, 137),                    # x0 = 1e-300, x1 = 5e-324 (fp32: both round to 0), Dbar = 70 g
    "second_meal": (14, 77, 139, 16, 79, 140),   # 45 g in transit by the edit, then 30 g: first minute / (16, 79, 140) second
    "tiny_meal": (17, 80, 142),                  # 0.05 g on an empty stomach
    "huge_meal": (19, 82, 143),                  # 400 g on an empty stomach
    "back_to_back": (20, 83, 145),               # 4 g and 3 g in the last minute of a step and the first of the next
    "meal_while_eating": (21, 84, 147),          # fed lanes of the feed = 3 inputs: 30 g more while the 70 g are being eaten
}
GUT_DEEP_ZERO = (34, 86)
GUT_SECOND_LATE = (16, 79, 140)
GUT_EDITED = ("no_dbar", "overfull", "deep_negative", "at_transition_b", "at_transition_d", "tiny_dbar", "huge_in_transit",
              "residue", "second_meal")
GUT_OVERFULL, GUT_DBAR_SMALL, GUT_DBAR_EATING, GUT_DBAR_MEAL, GUT_DBAR_HUGE = 30.0, 2.0, 1.0, 70.0, 400.0   # a ratio; grams


def gut_meals(st):
    """the meals after the edit: lane -> [(minute, grams)]; t0 = the first minute after the edit"""
    t0, L, out = STATUS_PRE * st, GUT_LANES, {}
    for i in L["second_meal"]:
        out[i] = [(t0 + (i in GUT_SECOND_LATE), 30.0)]           # Dexcom: the first / the middle minute of the step
    for i in L["tiny_meal"]:
        out[i] = [(t0, 0.05)]
    for i in L["huge_meal"]:
        out[i] = [(t0, 400.0)]
    for i in L["back_to_back"]:
        out[i] = [(t0 + st - 1, 4.0), (t0 + st, 3.0)]
    for i in L["meal_while_eating"]:
        out[i] = [(t0 + 1, 30.0)]
    return out


@functools.lru_cache(maxsize=None)
def gut_inputs(sensor="Navigator", n=STATUS_N, feed=3, meal_step=1):
    """status_inputs with gut_meals added: mt / ma = the meal table [3, n], ascending per env, and cho = the same meals per
    minute.  A meal in the minute of the 70 g meal (feed = 1: every env is fed in the first minute after the edit) is one
    entry with it."""
    from simglucose_amd import _lib
    inp = dict(status_inputs(sensor, n, feed, meal_step))
    meals = [[(int(inp["mt"][0, i]), float(inp["ma"][0, i]))] if inp["fed"][i] else [] for i in range(n)]
    for i, extra in gut_meals(inp["st"]).items():
        for t, g in extra:
            same = [j for j, (tt, _) in enumerate(meals[i]) if tt == t]
            if same:
                meals[i][same[0]] = (t, meals[i][same[0]][1] + g)
            else:
                meals[i].append((t, g))
        meals[i].sort()
    rows = max(len(m) for m in meals)
    mt, ma, cho = np.full((rows, n), _lib.MEAL_UNUSED, dtype=np.int64), np.zeros((rows, n)), np.zeros_like(inp["cho"])
    for i, m in enumerate(meals):
        for j, (t, g) in enumerate(m):
            mt[j, i], ma[j, i], cho[t, i] = t, g, g
    inp.update(mt=mt, ma=ma, cho=cho)
    return inp


def fma_word(a, b, c):
    """a * b + c rounded once to fp64, as the device's fma forms it"""
    v = Fraction(a) * Fraction(b) + Fraction(c)
    return v.numerator / v.denominator           # int / int is correctly rounded


def gut_states(target, pid):
    """target: the oracle (numpy rows x [13, n], last_qsto, last_food) or a device env (torch rows, and dbar), n >= 150,
    edited in place after the STATUS_PRE steps; pid: the patient row per env.  Every value is formed on the host in fp64
    and written as a Python float, so the oracle and an fp64 env receive the same words.  dbar is formed from the two words
    as the row holds them, 1000 last_food + last_qsto rounded once, which is what the kernels store there
    (test_gut_states_host.py: in fp64 the plain expression gives the same word in every lane).  -> GUT_LANES."""
    from simglucose_amd import params
    _, tab = params.patient_table()
    pid = np.asarray(pid)
    b, d = tab[pid, params.P_COL["b"]], tab[pid, params.P_COL["d"]]

    def put(i, x0, x1, lq, lf):
        target.x[0][i] = float(x0); target.x[1][i] = float(x1)
        target.last_qsto[i] = float(lq); target.last_food[i] = float(lf)
        if hasattr(target, "dbar"):
            target.dbar[i] = fma_word(float(target.last_food[i]), 1000.0, float(target.last_qsto[i]))

    L = GUT_LANES
    for i in L["no_dbar"]:
        put(i, 3000.0, 5000.0, 0.0, 0.0)
    for i in L["overfull"]:                                          # 20 g + 40 g on a 2 g meal
        q = GUT_OVERFULL * 1000.0 * GUT_DBAR_SMALL
        put(i, q / 3.0, q - q / 3.0, 0.0, GUT_DBAR_SMALL)
    for i in L["deep_negative"]:
        put(i, 0.0, 0.0 if i in GUT_DEEP_ZERO else 100.0, 0.0, GUT_DBAR_MEAL)
    for kind, frac in (("at_transition_b", b), ("at_transition_d", d)):
        for i in L[kind]:                                            # two equal halves: their sum is the product, exactly
            q = float(frac[i]) * (1000.0 * (GUT_DBAR_EATING + 5.0))
            put(i, 0.5 * q, 0.5 * q, 0.0, GUT_DBAR_EATING)
    for i in L["tiny_dbar"]:                                         # both words in use: 20 mg + 1000 * 0.03 g
        put(i, 15.0, 25.0, 20.0, 0.03)
    for i in L["huge_in_transit"]:
        put(i, 150000.0, 220000.0, 0.0, GUT_DBAR_HUGE)
    for i in L["residue"]:
        put(i, 1e-300, 5e-324, 0.0, GUT_DBAR_MEAL)
    for i in L["second_meal"]:
        put(i, 20000.0, 25000.0, 0.0, GUT_DBAR_MEAL)
    return L


def gut_lanes(*kinds):
    """the lanes of the given kinds, sorted, each once"""
    return sorted({i for k in kinds for i in GUT_LANES[k]})


def gut_arguments(o, pid):
    """from a gut_oracle run made minute by minute: the doubled arguments of the tanh pair -- what the kernels' exponentials
    take, 2 aa (qsto - b Dbar) and 2 cc (qsto - d Dbar) of t1dpatient.py:136-140 -- at the start of every minute, with the
    meal words as that minute uses them -> (A2, C2, Dbar, qsto), each [minutes, n]; A2 = C2 = 0 where Dbar = 0"""
    from simglucose_amd import params
    _, tab = params.patient_table()
    b, d = tab[pid, params.P_COL["b"]], tab[pid, params.P_COL["d"]]
    start = np.concatenate([o["x_reset"][None], o["x"][:-1]])
    t0 = len(start) * STATUS_PRE // (STATUS_PRE + STATUS_POST)
    start[t0] = o["x_edit"]
    qsto = start[:, 0] + start[:, 1]
    dbar = o["last_qsto"] + 1000.0 * o["last_food"]
    safe = np.where(dbar > 0, dbar, 1.0)
    a2 = np.where(dbar > 0, 5.0 / (1.0 - b) / safe * (qsto - b * safe), 0.0)
    c2 = np.where(dbar > 0, 5.0 / d / safe * (qsto - d * safe), 0.0)
    return a2, c2, dbar, qsto


def gut_oracle_run(sensor="Navigator", integrator="split_adaptive", feed=3, meal_step=1, after_edit=None, minutes=False):
    """edge_oracle_run over gut_inputs with gut_states as the edit"""
    return edge_oracle_run(sensor, integrator, feed, meal_step, after_edit, minutes, inputs=gut_inputs, edit=gut_states)


@functools.lru_cache(maxsize=None)
def gut_oracle(sensor="Navigator", integrator="split_adaptive", feed=3, meal_step=1, minutes=False):
    """gut_oracle_run, computed once per argument set; treat as read-only"""
    return gut_oracle_run(sensor, integrator, feed, meal_step, minutes=minutes)


# ------------------------------------------------------------------------------------------------ the random streams
# test_streams_host.py, test_gpu_streams.py: what the device draws against oracle/t1d_streams.py, the host restatement written
# from include/t1d.h and rocRAND's headers.  The cases live here so that the host test can take its census of rounding ties
# over exactly what the GPU test compares.  Importing and building the references touches no device.
STREAM_SEED = 11
STREAM_OFF = 2 ** 32 - 65                 # 130 envs from here straddle 2^32
# envs of seed 11, start 0, days = 2 in which a meal lands on the minute of the meal before it (found by the restatement
# among the first 2^21 envs: for c in range(8): random_meals(11, c << 18, 1 << 18, 2, 0).cand["same_minute"])
SAME_MINUTE_GIDS = (740847, 749116, 1298792, 1588297, 203870, 1617688, 1452703, 418289, 1937777, 1867863)
# name -> (env_offset, n, start: a minute of day, or "table" for start_table(n))
MEAL_CASES = {"start0": (0, 4096, 0), "start14h": (0, 4096, 14 * 60), "start_table": (0, 4096, "table"),
              "past_2_32": (STREAM_OFF, 130, 0)}
MEAL_CASES.update({"same_minute_%d" % g: (g - 1, 3, 0) for g in SAME_MINUTE_GIDS})
RESTART_SEED, RESTART_N, RESTART_EPISODES = 3, 130, (0, 1, 5)
NORMALS_N, NORMALS_DRAW0, NORMALS_DRAWS = 130, -3, 29
NORMALS_OFFSETS = (0, 2 ** 32 - 65, 2 ** 40 + 3)
NORMALS_EPISODES = (0, 1, 255, 256, 2 ** 32 - 1)
NORMALS_SEEDS = (0, 0x9E3779B97F4A7C15)


def streams():
    """oracle/t1d_streams.py"""
    from oracle import t1d_streams
    return t1d_streams


def start_table(n):
    """a start minute per env that is no whole hour: every minute of the day comes up"""
    return ((np.arange(n, dtype=np.int64) * 37 + 5) % 1440).astype(np.int32)


@functools.lru_cache(maxsize=None)
def meal_reference(case):
    """the restatement's Meals of a case of MEAL_CASES; computed once, treat as read-only"""
    off, n, start = MEAL_CASES[case]
    return streams().random_meals(STREAM_SEED, off, n, DAYS, start_table(n) if isinstance(start, str) else start)


@functools.lru_cache(maxsize=None)
def restart_reference(k):
    """what t1d_restart_done gives env STREAM_OFF + i of seed RESTART_SEED at episode index k: (start_minute int64 [n], the
    restatement's Meals under seed * 7919 + k); the start hour by the package's host formula"""
    import torch
    from simglucose_amd.envs.batched_gym_env import start_hours
    gid = torch.arange(RESTART_N, dtype=torch.int64) + STREAM_OFF
    start = 60 * start_hours(RESTART_SEED, k, gid).numpy()
    return start, streams().random_meals(RESTART_SEED * 7919 + k, STREAM_OFF, RESTART_N, DAYS, start)


@functools.lru_cache(maxsize=None)
def normals_reference(seed, env_offset, episode):
    """the restatement's Normals (float64 and high precision) of one case of the NORMALS_* cross product"""
    return streams().normals(seed, env_offset, NORMALS_N, episode, NORMALS_DRAW0, NORMALS_DRAWS, mp=True)


def normal_error(z, ref):
    """|z - (hi + lo)| in units of eps * s, s the sqrt(-2 ln u) of the draw's pair: the error of a set of normals against
    the high-precision values -> array like z"""
    return np.abs((z - ref.hi) - ref.lo) / (np.finfo(np.float64).eps * ref.s)


def meal_tables_cover_the_branches():
    """so that an exact comparison of the MEAL_CASES cannot pass on nothing; asserted on the restatement alone"""
    for case in ("start0", "start14h", "start_table", "past_2_32"):
        c = meal_reference(case).cand
        assert (~c["present"]).any() and (c["present"] & ~c["in_range"]).any(), case         # absent; present but filtered
        assert (c["kept"] & (c["g_raw"] < -0.5)).any() and (c["kept"] & (c["grams"] > 0)).any(), case   # grams clamped to 0
    c0, c14, ctab = (meal_reference(case).cand for case in ("start0", "start14h", "start_table"))
    for c in (c14, ctab):                                                      # filtered on both sides of the episode
        assert (c["present"] & (c["minute"] < 0)).any() and (c["present"] & (c["minute"] >= 1440 * DAYS)).any()
    assert c0["kept"][DAYS - 1].all(axis=0).any()                                # a full last day: all six meals of it
    assert c14["kept"][DAYS].any() and not c0["kept"][DAYS].any()                # ... and a cut one after a late start
    assert any(meal_reference("same_minute_%d" % g).cand["same_minute"].any() for g in SAME_MINUTE_GIDS)


# ------------------------------------------------------------------------------------------------ outcome statistics
# test_outcome_host.py, test_gpu_outcome.py: t1d_outcome_stats (outcome_kernel) against references that share no code with
# it.  The inputs are built here so that the host file can show that they reach what they are meant to reach -- every
# threshold, both sides of every zone bound, every kind of row the risk trace skips -- on exactly what the GPU file runs.
OUT_NS = (1, 63, 64, 65, 257, 300)            # a lane, a wave short of / at / past its end, past a 256-thread block
OUT_ROWS = (1, 2, 3, 40, 41, 481)
OUT_QS = ((2.5, 97.5), (0.0, 100.0), (50.0, 50.0), (33.3, 99.9))
OUT_U = Fraction(1, 2 ** 53)
OUT_KINDS = ("distinct", "constant", "two_valued", "sign_mixed", "tie_at_rank", "adjacent_at_rank", "negative", "thresholds")
OUT_THRESHOLDS = (50, 70, 180, 250)
RISK_ROWS, RISK_N = 127, 70                   # 127 is prime: no chunk but 1 and 127 divides it
RISK_CHUNKS = (1, 7, 60, RISK_ROWS, RISK_ROWS + 5)
RISK_C_LIMIT = 64                             # an asserted C beyond this is an arithmetic error, not rounding


def out_np(dtype):
    return {"f64": np.float64, "f32": np.float32}[dtype]


def out_ut(dtype):
    """the unit roundoff of the final cast: none in fp64"""
    return Fraction(0) if dtype == "f64" else Fraction(1, 2 ** 24)


def _next(v, up):
    v = np.asarray(v)
    return np.nextafter(v, np.array(np.inf if up else -np.inf, v.dtype))


def outcome_threshold_pool(ft):
    """50, 70, 180 and 250 with the float of type ft on either side of each, and five values away from them"""
    t = np.array(OUT_THRESHOLDS, ft)
    return np.concatenate([_next(t, False), t, _next(t, True), np.array([30, 60, 100, 200, 300], ft)])


def outcome_threshold_inputs(n, rows, dtype, seed=3):
    """[rows, n]: every env draws its rows from the threshold pool with weights of its own, so that the counters differ"""
    pool = outcome_threshold_pool(out_np(dtype))
    out = np.empty((rows, n), pool.dtype)
    for i in range(n):
        rs = np.random.RandomState(seed * 100003 + i * 13 + rows)
        out[:, i] = rs.choice(pool, rows, p=rs.dirichlet(np.ones(len(pool))))
    return out


def outcome_counts(bg):
    """the five counters of percent_stats by numpy's comparisons in the inputs' own type -> int64 [5, n]; NaN is in no range"""
    with np.errstate(invalid="ignore"):
        return np.stack([(bg > 180).sum(0), (bg < 70).sum(0), ((bg >= 70) & (bg <= 180)).sum(0), (bg > 250).sum(0),
                         (bg < 50).sum(0)]).astype(np.int64)


def rank_of(rows, q):
    """pos = (rows - 1) q / 100 exactly (q as the double the kernel gets) -> (pos, floor(pos))"""
    pos = Fraction(rows - 1) * Fraction(float(q)) / 100
    return pos, pos.numerator // pos.denominator


def outcome_columns(n, rows, dtype, qs=OUT_QS[0], seed=1):
    """[rows, n], a column per env and no two alike, the kinds of OUT_KINDS in turn: distinct values; one value; two values;
    both signs with both zeros, subnormals and values near the top of the format; the order statistics k and k + 1 of either
    percentile of qs equal, and adjacent floats; all negative; draws from the threshold pool"""
    ft = out_np(dtype)
    big, sub = (1e300, 5e-324) if dtype == "f64" else (1e38, 1.4e-45)
    ranks = [rank_of(rows, q)[1] for q in qs]
    out = np.empty((rows, n), ft)
    for i in range(n):
        rs = np.random.RandomState(seed * 100003 + i * 7 + rows)
        kind = OUT_KINDS[i % len(OUT_KINDS)]
        if kind == "distinct":
            c = rs.uniform(40, 400, rows)
        elif kind == "constant":
            c = np.full(rows, 100 + 0.37 * i)
        elif kind == "two_valued":
            c = np.where(rs.rand(rows) < 0.4, 80 + 0.01 * i, 200 + 0.01 * i)
        elif kind == "sign_mixed":
            pool = np.array([0.0, -0.0, sub, -sub, 3 * sub, -7 * sub, big, -big, 0.5 * big, -0.25 * big, 1.5 + i, -2.5 - i,
                             1e-3 * (i + 1), -1e-3 * (i + 1)])
            c = rs.permutation(pool)[:rows]
            c = np.concatenate([c, rs.uniform(-300, 300, rows - len(c))])
        elif kind in ("tie_at_rank", "adjacent_at_rank"):
            c = np.sort(rs.uniform(40, 400, rows).astype(ft))
            for k in ranks:
                if k + 1 < rows:
                    c[k + 1] = c[k] if kind == "tie_at_rank" else _next(c[k], True)
        elif kind == "negative":
            c = -rs.uniform(1e-3, 500, rows)
        else:
            c = rs.choice(outcome_threshold_pool(ft), rows)
        out[:, i] = np.asarray(c).astype(ft)[rs.permutation(rows)]
    return out


def percentile_reference(bg, q, dtype):
    """The q-th percentile of every column of bg [rows, n] (the values the kernel sees) in exact rational arithmetic:
    pos = (rows - 1) q / 100, lo = floor(pos), a + (b - a)(pos - lo) over the sorted column -> (ref, bound), a Fraction per
    env, None for a column that holds a NaN.

    bound = (2 pos + 3) u |b - a| + (2 u + u_T) |ref| + underflow, u = 2^-53: two roundings in pos, three in the lerp, two
    of the result and the final cast (u_T = 2^-24 in fp32).  Those are relative errors, which a product that ends below the
    normal range does not keep: the lerp's one product may then be off by half the smallest fp64 subnormal, 2^-1075, and a
    cast that ends below fp32's normal range by 2^-150.  That is the underflow term; it is below every other term unless
    |b - a| and |ref| are both subnormal.  The bound takes floor(pos) in floating point to be the exact one
    (test_outcome_host.py checks that for every pair of OUT_ROWS and OUT_QS)."""
    bg = np.asarray(bg)
    rows, n = bg.shape
    pos, lo = rank_of(rows, q)
    hi, t = min(lo + 1, rows - 1), pos - lo
    s = np.sort(bg.astype(np.float64), axis=0)                  # by value; NaN sorts last
    under = Fraction(1, 2 ** 1075) + (Fraction(0) if dtype == "f64" else Fraction(1, 2 ** 150))
    ref, bound = [], []
    for i in range(n):
        if np.isnan(s[-1, i]):
            ref.append(None); bound.append(None)
            continue
        a, b = Fraction(float(s[lo, i])), Fraction(float(s[hi, i]))
        r = a + (b - a) * t
        ref.append(r)
        bound.append((2 * pos + 3) * OUT_U * abs(b - a) + (2 * OUT_U + out_ut(dtype)) * abs(r) + under)
    return ref, bound


def percentile_error(got, ref, bound):
    """|got - ref| / bound per env -> float [n]; by value, so -0.0 is +0.0; a NaN where the reference has one is 0, any
    other non-finite result +Inf"""
    out = np.zeros(len(ref))
    for i, (r, b) in enumerate(zip(ref, bound)):
        g = float(got[i])
        if r is None or not math.isfinite(g):
            out[i] = 0.0 if (r is None and math.isnan(g)) else math.inf
        else:
            out[i] = float(abs(Fraction(g) - r) / b)
    return out


def worst_by_kind(err):
    """the largest entry of err [n] among the sign_mixed columns (where the underflow term of the bound can be the one that
    counts) and among all others -> (others, sign_mixed)"""
    mixed = np.arange(len(err)) % len(OUT_KINDS) == OUT_KINDS.index("sign_mixed")
    return float(err[~mixed].max(initial=0.0)), float(err[mixed].max(initial=0.0))


# the comparisons of CVGA_analysis (report.py:198-217), one row per zone: its code and its alternatives, each a conjunction
CVGA_CLAUSES = (
    (0, ((("mn", ">", 90), ("mn", "<=", 110), ("mx", ">=", 110), ("mx", "<", 180)),)),
    (1, ((("mn", ">", 70), ("mn", "<=", 110), ("mx", ">=", 110), ("mx", "<", 300)),)),
    (2, ((("mn", ">", 90), ("mn", "<=", 110), ("mx", ">=", 300)), (("mn", "<=", 70), ("mx", ">=", 110), ("mx", "<", 180)))),
    (3, ((("mn", ">", 70), ("mn", "<=", 90), ("mx", ">=", 300)), (("mn", "<=", 70), ("mx", ">=", 180), ("mx", "<", 300)))),
    (4, ((("mn", "<=", 70), ("mx", ">=", 300)),)),
)
_CVGA_OPS = {">": np.greater, ">=": np.greater_equal, "<": np.less, "<=": np.less_equal}
_CVGA_FLIP = {">": ">=", ">=": ">", "<": "<=", "<=": "<"}
CVGA_COMPARISONS = tuple((z, a, t) for z, alts in CVGA_CLAUSES for a, alt in enumerate(alts) for t in range(len(alt)))


def cvga_alternatives(mn, mx, flip=None):
    """{(zone, alternative): bool [n]} on the clipped percentiles; flip = (zone, alternative, term) moves the equality of
    that one comparison to its other side (> for >=, < for <=, and back)"""
    v = {"mn": np.clip(np.asarray(mn, np.float64), 50, 400), "mx": np.clip(np.asarray(mx, np.float64), 50, 400)}
    out = {}
    for z, alts in CVGA_CLAUSES:
        for a, alt in enumerate(alts):
            ok = np.ones(v["mn"].shape, bool)
            for t, (name, op, b) in enumerate(alt):
                ok &= _CVGA_OPS[_CVGA_FLIP[op] if flip == (z, a, t) else op](v[name], b)
            out[z, a] = ok
    return out


def cvga_zone_codes(mn, mx, flip=None):
    """the zone code of every env, first zone that holds in the order A..E, else 5: a restatement of the oracle's
    report_cvga from the table above, held to it by test_outcome_host.py; flip as in cvga_alternatives"""
    alt = cvga_alternatives(mn, mx, flip)
    code = np.full(np.shape(mn), 5)
    for z, alts in reversed(CVGA_CLAUSES):
        hit = np.zeros(np.shape(mn), bool)
        for a in range(len(alts)):
            hit |= alt[z, a]
        code = np.where(hit, z, code)
    return code


@functools.lru_cache(maxsize=None)
def zone_grid(dtype):
    """Two-row columns [2, n] whose min and max walk every zone bound and both clip bounds: the bound and the float of the
    batch's type on either side of it, and values between and beyond the bounds, in every combination with min <= max.
    With q = (0, 100) the percentiles are the min and the max themselves.  -> (bg, mn, mx); which row holds the min
    alternates with the env.  Read-only."""
    ft = out_np(dtype)

    def around(bounds, other):
        b = np.array(bounds, ft)
        return np.concatenate([_next(b, False), b, _next(b, True), np.array(other, ft)])
    mn_vals = around((50, 70, 90, 110, 400), (30, 60, 80, 100, 150, 450))
    mx_vals = around((50, 110, 180, 300, 400), (40, 100, 150, 250, 350, 500))
    pairs = np.array([(a, b) for a in mn_vals for b in mx_vals if a <= b], ft)
    mn, mx = pairs[:, 0].copy(), pairs[:, 1].copy()
    swap = np.arange(len(mn)) % 2 == 1
    bg = np.stack([np.where(swap, mx, mn), np.where(swap, mn, mx)])
    for a in (bg, mn, mx):
        a.setflags(write=False)
    return bg, mn, mx


@functools.lru_cache(maxsize=None)
def risk_inputs(dtype):
    """[RISK_ROWS, RISK_N], read-only: BG-like columns, twelve that stay low (f < 0), twelve high (f > 0), eight around
    112.5 mg/dL where f changes sign, and in the first eight envs the rows risk_index_trace skips: BG <= 0 with both zeros,
    0 < BG < 1, BG = 1 (ln = 0, the lowest usable f), +Inf, a first week of rows and a last chunk of 60 with nothing usable,
    and a column with no usable row at all"""
    rs = np.random.RandomState(5)
    bg = rs.uniform(40, 400, (RISK_ROWS, RISK_N))
    bg[:, 8:20] = rs.uniform(45, 100, (RISK_ROWS, 12))
    bg[:, 20:32] = rs.uniform(150, 400, (RISK_ROWS, 12))
    bg[:, 32:40] = rs.uniform(105, 120, (RISK_ROWS, 8))
    bg[3, 0], bg[5, 0], bg[3, 1], bg[3, 2], bg[64, 2], bg[3, 3], bg[10, 4] = 0.0, -0.0, -5.0, 0.5, 1e-30, 1.0, np.inf
    bg[0:7, 5] = (0.0, -1.0, 0.5, -0.0, 0.25, -3.0, 0.999)
    bg[:, 6] = 0.5
    bg[120:, 7] = 0.0
    bg = bg.astype(out_np(dtype))
    bg.setflags(write=False)
    return bg


def risk_terms(bg):
    """per sample, at 50 digits: ln(BG)^1.084 where 1.509 (ln(BG)^1.084 - 5.381) is a real number -- BG >= 1, +Inf
    included -- and None elsewhere (BG <= 0, NaN, and 0 < BG < 1, the power of a negative logarithm) -> object [rows, n].
    The constants are the doubles the code holds."""
    import mpmath
    out = np.empty(bg.shape, object)
    with mpmath.workdps(50):
        for idx, v in np.ndenumerate(np.asarray(bg, np.float64)):
            out[idx] = mpmath.log(mpmath.mpf(float(v))) ** mpmath.mpf(1.084) if v >= 1 else None
    return out


def risk_reference(terms, chunk):
    """risk_index_trace from risk_terms: per chunk and env (cnt, f, S) -> three arrays [n_chunks, n]; f = the mean of
    1.509 (p - 5.381) over the cnt usable rows (None without one), S = 1.509 (mean p + 5.381) the scale of its rounding"""
    import mpmath
    rows, n = terms.shape
    nch = (rows + chunk - 1) // chunk
    cnt, f, S = np.zeros((nch, n), np.int64), np.empty((nch, n), object), np.empty((nch, n), object)
    with mpmath.workdps(50):
        a, b = mpmath.mpf(1.509), mpmath.mpf(5.381)
        for c in range(nch):
            for i in range(n):
                p = [v for v in terms[c * chunk:(c + 1) * chunk, i] if v is not None]
                cnt[c, i] = len(p)
                mean = mpmath.fsum(p) / len(p) if p else None
                f[c, i] = a * (mean - b) if p else None
                S[c, i] = a * (mean + b) if p else None
    return cnt, f, S


def risk_compare(lbgi, hbgi, ref, dtype, C):
    """LBGI and HBGI [n_chunks, n] of a run against risk_reference -> dict:
    nan_equal: NaN exactly where the reference has no usable row; where f is +Inf (a +Inf sample) LBGI = 0 and HBGI = +Inf;
    c_needed:  fp64 only -- the largest |f - f_ref| / (u S) - cnt, f recovered from the outputs as -sqrt(LBGI / 10) or
               +sqrt(HBGI / 10) at 50 digits (an fp32 output carries f to 2^-25 only, so there the next figure is the check);
    worst:     the largest error of LBGI or HBGI over 10 (2 |f_ref| D + D^2) + (3 u + u_T) |ref|, D = (cnt + C) u S."""
    import mpmath
    cnt, f, S = ref
    u, ut = mpmath.mpf(2) ** -53, mpmath.mpf(float(out_ut(dtype)))
    res = {"nan_equal": True, "c_needed": -math.inf, "worst": 0.0}
    with mpmath.workdps(50):
        for idx in np.ndindex(cnt.shape):
            L, H = float(lbgi[idx]), float(hbgi[idx])
            if f[idx] is None:
                res["nan_equal"] &= math.isnan(L) and math.isnan(H)
                continue
            if math.isnan(L) or math.isnan(H):
                res["nan_equal"] = False
                continue
            if mpmath.isinf(f[idx]):
                res["nan_equal"] &= L == 0.0 and H == math.inf
                continue
            fr = f[idx]
            if dtype == "f64":
                fg = -mpmath.sqrt(mpmath.mpf(L) / 10) if L > 0 else mpmath.sqrt(mpmath.mpf(H) / 10)
                res["c_needed"] = max(res["c_needed"], float(abs(fg - fr) / (u * S[idx]) - int(cnt[idx])))
            D = (int(cnt[idx]) + C) * u * S[idx]
            for got, want in ((L, 10 * fr * fr if fr < 0 else mpmath.mpf(0)), (H, 10 * fr * fr if fr > 0 else mpmath.mpf(0))):
                bound = 10 * (2 * abs(fr) * D + D * D) + (3 * u + ut) * abs(want)
                res["worst"] = max(res["worst"], float(abs(mpmath.mpf(got) - want) / bound))
    return res


NAN_N, NAN_ROWS = 300, 41
# env -> (rows that hold a NaN, its sign bit): first row, last row, an inner row, the last env, and a whole column
NAN_CASES = {5: ((0,), 0), 64: ((NAN_ROWS - 1,), 1), 130: ((7,), 0), 299: ((0,), 1), 257: (tuple(range(NAN_ROWS)), None)}


def nan_inputs(dtype):
    """-> (clean, poisoned): outcome_columns for NAN_N envs, and a copy with the NaNs of NAN_CASES (None: alternating signs)"""
    clean = outcome_columns(NAN_N, NAN_ROWS, dtype)
    bad = clean.copy()
    for env, (rows, sign) in NAN_CASES.items():
        for r in rows:
            bad[r, env] = np.copysign(np.nan, -1.0 if (r % 2 if sign is None else sign) else 1.0)
    return clean, bad


@functools.lru_cache(maxsize=None)
def risk_reference_of(dtype, chunk):
    """risk_reference of risk_inputs(dtype); the 50-digit terms are computed once per dtype.  Read-only."""
    return risk_reference(_risk_terms_of(dtype), chunk)


@functools.lru_cache(maxsize=None)
def _risk_terms_of(dtype):
    return risk_terms(risk_inputs(dtype))
