"""The single-minute launch after its trim: the LDS tables staged from an image kept with the context, and the risk index
of a freshly clamped CGM value without numpy's special cases.  Small batches (150 envs = two full chunks and a partial one,
64 envs), states at the branch points of the model: negative and held compartments, a step through x3 = 0, lanes the
step-size rule sets aside, CGM at both ends of the sensor range.

Tolerances: HIP vs the oracle's restatement of the same scheme is test_gpu_parity's TOL_ORACLE (1e-8 mg/dL on BG / CGM;
the 13 states, whose magnitudes reach 1e4, relative to max(1, |value|)); reward / risk 1e-6 as there; fp32 against fp64
0.05 mg/dL as test_gpu_configs holds the fp32 kernels to.  One kernel against another in fp64: equal bit for bit."""
import numpy as np
import pytest

from test_gpu_parity import TOL_ORACLE

gpu = pytest.mark.gpu

TOL_F32 = 0.05
N = 150


def _basal(pid):
    from oracle import t1d_oracle as O
    _, tab = O.patient_table()
    return tab[pid, O.IDX["u2ss"]] * tab[pid, O.IDX["BW"]] / 6000.0


def _edge_states(x):
    """x: [13, n] array-like (numpy or torch), edited in place.  Chunk 0: x4 and x12 slightly negative in a few lanes; chunk
    1: x3 < 0 (held) in a few lanes, and one lane whose x3 is small with a rate of about -1 mg/kg/min (no hepatic
    production under a large delayed-insulin signal, an empty tissue compartment), so that the step crosses zero; a lane
    close to x3 = 0 in every chunk (the step-size rule's x3 condition: level 2).  Chunk 2 otherwise all positive."""
    for i in (3, 17, 40):
        x[4][i] = -1e-3
    for i in (5, 17, 63):
        x[12][i] = -2e-3
    for i in (64, 70, 101, 127):
        x[3][i] = -0.25
    for i in (90, 20, 140):
        x[3][i] = 0.05; x[4][i] = 0.0; x[8][i] = 500.0


def _make(dtype=None, n=N, **opts):
    import torch
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    pid = np.arange(n) % 30
    z = np.random.RandomState(5).randn(24, n)
    env = BatchedT1DSimEnv(patient=pid, sensor="Navigator", noise="host", normals=z, n_sub=4,
                           dtype=dtype or torch.float64)
    for k, v in opts.items():
        env.set_option(k, v)
    return env, pid, z


def _run(env, pid, minutes, edge=True):
    """reset, two minutes that start a meal in a third of the lanes, the edge states, then `minutes` more"""
    import torch
    n = env.n
    b = torch.as_tensor(_basal(pid), dtype=env.dtype, device=env.device)
    env.reset()
    for k in range(2):
        cho = np.zeros((1, n)); cho[0, ::3] = 70.0 if k == 0 else 0.0
        env.step(b, cho=cho)
    if edge:
        _edge_states(env.x)
    for k in range(minutes):
        env.step(b * (0.5 + 0.5 * (k % 3)), cho=np.zeros((1, n)))
    assert env.sync() == 0
    return env.x.double().cpu().numpy(), env.bg.double().cpu().numpy(), env.cgm.double().cpu().numpy()


@pytest.fixture(scope="module")
def oracle5():
    """the same five minutes on the CPU oracle (split scheme with per-minute step sizes)"""
    from oracle import t1d_oracle as O
    pid = np.arange(N) % 30
    z = np.random.RandomState(5).randn(24, N)
    orc = O.OracleEnv(pid, sensor="Navigator", normals=z, integrator="split_adaptive", n_sub=4)
    b = _basal(pid)
    orc.reset()
    for k in range(2):
        cho = np.zeros((1, N)); cho[0, ::3] = 70.0 if k == 0 else 0.0
        orc.step(b, None, cho)
    _edge_states(orc.x)
    lev0 = orc.level_count.copy()
    for k in range(5):
        r = orc.step(b * (0.5 + 0.5 * (k % 3)), None, np.zeros((1, N)))
    # the oracle takes the negative-state inputs finitely, and the rule has put lanes at level 2
    assert np.isfinite(orc.x).all() and np.isfinite(r["bg"]).all()
    assert (orc.level_count - lev0)[2] > 0
    return orc.x.copy(), r["bg"].copy(), r["cgm"].copy()


def test_oracle_takes_negative_states(oracle5):
    """no GPU: the reference side of the comparisons below is finite, holds x3 < 0 and ends a crossing at -1e-10"""
    ox, obg, _ = oracle5
    assert ox[3, 90] == -1e-10 and (ox[3, [64, 70, 101, 127]] == -0.25).all() and np.isfinite(obg).all()


@gpu
def test_negative_states_vs_oracle_and_generic_kernel(oracle5):
    env, pid, _ = _make()
    x, bg, cgm = _run(env, pid, 5)
    ox, obg, ocgm = oracle5
    ex = np.abs(x - ox) / np.maximum(1.0, np.abs(ox))
    print("negative states: max |HIP - oracle| states (rel.) %.3e BG %.3e CGM %.3e" % (ex.max(), np.abs(bg - obg).max(), np.abs(cgm - ocgm).max()))
    assert ex.max() < TOL_ORACLE and np.abs(bg - obg).max() < TOL_ORACLE and np.abs(cgm - ocgm).max() < TOL_ORACLE
    assert x[3, 90] == -1e-10 and (x[3, [64, 70, 101, 127]] == -0.25).all()       # crossed zero; held
    gen, _, _ = _make(single_minute_kernel=0)
    gx, gbg, gcgm = _run(gen, pid, 5)
    # states and BG bit for bit; the sensor sample Gsub + noise is contracted into FMAs per kernel instance: TOL_ORACLE
    assert np.array_equal(x, gx) and np.array_equal(bg, gbg) and np.abs(cgm - gcgm).max() < TOL_ORACLE
    assert np.abs(env.reward.cpu().numpy() - gen.reward.cpu().numpy()).max() < 1e-6


@gpu
def test_set_aside_lanes_equal_in_place_form():
    """lanes of level 2 in every chunk (set aside, integrated by the pass over the list) against adaptive_gut = 2, every
    lane in place"""
    a, pid, _ = _make()
    b, _, _ = _make(adaptive_gut=2)
    xa, bga, cgma = _run(a, pid, 3)
    xb, bgb, cgmb = _run(b, pid, 3)
    assert np.array_equal(xa, xb) and np.array_equal(bga, bgb) and np.abs(cgma - cgmb).max() < TOL_ORACLE
    assert np.abs(a.reward.cpu().numpy() - b.reward.cpu().numpy()).max() < 1e-6


@gpu
def test_risk_at_both_clamps_vs_oracle():
    """CGM driven to the sensor's lower end (large negative noise) and to its upper end (large positive noise; BG above the
    range): reward and the carried risk index against the oracle."""
    import torch
    from oracle import t1d_oracle as O
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    n = 64
    pid = np.arange(n) % 30
    z = np.random.RandomState(6).randn(24, n)
    z[:, 0:24] -= 9.0
    z[:, 24:40] += 9.0
    env = BatchedT1DSimEnv(patient=pid, sensor="Navigator", noise="host", normals=z, n_sub=4)
    orc = O.OracleEnv(pid, sensor="Navigator", normals=z, integrator="split_adaptive", n_sub=4)
    env.reset(); orc.reset()
    vg = env.table[pid, O.IDX["Vg"]]
    hi = 700.0 * vg[40:48]
    env.x[12][40:48] = torch.as_tensor(hi, device=env.device); orc.x[12, 40:48] = hi
    vmin, vmax = env.sensor_row[6], env.sensor_row[7]
    b = _basal(pid)
    worst = 0.0
    for k in range(4):
        obs, rew, done, info = env.step(torch.as_tensor(b), cho=np.zeros((1, n)))
        r = orc.step(b, None, np.zeros((1, n)))
        cgm = obs.cpu().numpy()
        worst = max(worst, np.abs(rew.cpu().numpy() - r["reward"]).max(), np.abs(cgm - r["cgm"]).max())
        f = 1.509 * (np.log(r["cgm"]) ** 1.084 - 5.381)
        worst = max(worst, np.abs(env.prev_risk.cpu().numpy() - 10.0 * f * f).max())
        # both ends of the range and the open interval between them occur in every step
        assert (cgm == vmin).any() and (cgm == vmax).any() and ((cgm > vmin) & (cgm < vmax)).any()
    print("risk at the clamps: max |HIP - oracle| %.3e" % worst)
    assert env.sync() == 0 and worst < 1e-6


@gpu
def test_table_image_follows_n_sub():
    """step at n_sub = 4, change to 8, step on: equal, bit for bit, to a fresh env created at n_sub = 8 that takes over the
    state -- tables left over from n_sub = 4 would not be."""
    import torch
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    n = 64
    pid = np.arange(n) % 30
    z = np.random.RandomState(7).randn(24, n)
    b = torch.as_tensor(_basal(pid))
    a = BatchedT1DSimEnv(patient=pid, sensor="Navigator", noise="host", normals=z, n_sub=4)
    a.reset()
    cho = np.zeros((1, n)); cho[0, ::2] = 50.0
    a.step(b, cho=cho)
    a.step(b, cho=np.zeros((1, n)))
    x4 = a.x.cpu().numpy().copy()
    f = BatchedT1DSimEnv(patient=pid, sensor="Navigator", noise="host", normals=z, n_sub=8)
    f.reset()
    f.load_state_dict(a.state_dict())
    a.n_sub = 8
    for k in range(3):
        a.step(b, cho=np.zeros((1, n))); f.step(b, cho=np.zeros((1, n)))
    assert a.sync() == 0 and f.sync() == 0
    assert np.array_equal(a.x.cpu().numpy(), f.x.cpu().numpy()) and np.array_equal(a.cgm.cpu().numpy(), f.cgm.cpu().numpy())
    assert np.array_equal(a.reward.cpu().numpy(), f.reward.cpu().numpy())
    # and the step size did change: at n_sub = 4 the same three minutes end elsewhere
    c = BatchedT1DSimEnv(patient=pid, sensor="Navigator", noise="host", normals=z, n_sub=4)
    c.reset()
    c.load_state_dict(f.state_dict())
    c.x.copy_(torch.as_tensor(x4, device=c.device))
    c.step(b, cho=np.zeros((1, n)))
    f.x.copy_(torch.as_tensor(x4, device=f.device))
    f.step(b, cho=np.zeros((1, n)))
    assert not np.array_equal(c.x.cpu().numpy(), f.x.cpu().numpy())


@gpu
def test_negative_states_fp32_vs_fp64():
    import torch
    e64, pid, _ = _make()
    e32, _, _ = _make(dtype=torch.float32)
    x64, bg64, cgm64 = _run(e64, pid, 5)
    x32, bg32, cgm32 = _run(e32, pid, 5)
    print("negative states fp32 vs fp64: BG %.3e CGM %.3e" % (np.abs(bg32 - bg64).max(), np.abs(cgm32 - cgm64).max()))
    assert np.abs(bg32 - bg64).max() < TOL_F32 and np.abs(cgm32 - cgm64).max() < TOL_F32
