"""step1d_kernel in fp64 at four waves per SIMD (sixteen waves per workgroup): the set-aside form (adaptive_gut = 3) against
the in-place form (adaptive_gut = 2) where the waves of a workgroup draw several chunks each and where most of them find
the queue empty, its independence of which wave drew which chunk, and the oracle's restatement of the scheme.  fp64,
Navigator, Philox noise, n_sub = 4.

Tolerances: one form against the other as test_deferred_refinement_equals_in_place_refinement holds them (1e-9 on BG, CGM
and reward, 1e-7 on the 13 states: the two instantiations may contract FMAs differently); HIP against the oracle as
test_full_size_24h_run_sampled_envs_match_oracle does on this very workload (test_gpu_parity's TOL_ORACLE = 1e-8 mg/dL on
BG and CGM, 1e-6 on the states, whose magnitudes reach 1e4; reward 1e-6 as test_gpu_step_trim)."""
import numpy as np
import pytest

from support import basal_of, plain_env
from test_gpu_parity import TOL_ORACLE

pytestmark = pytest.mark.gpu

TOL, TOL_X = 1e-9, 1e-7
N1, K1 = 64 * 40 - 7, 60           # one workgroup: two and a half rounds for sixteen waves, the last chunk partly masked
N2, K2 = 64 * 5 + 1, 30            # fewer chunks than waves
SHARED1, SHARED2 = 640, 130
N_ORACLE = 300
OUT = ("x", "cgm", "bg", "reward", "done", "t")


def _tables(n, shared):
    """random meal tables from 06:00; the first `shared` envs take the plan of the env whose first meal is closest to minute
    15, so that they start it in the same minute and whole waves are listed at once"""
    import torch
    from simglucose_amd import scenario_batch as sb
    mt, ma = sb.random_meal_tables(n, days=1, start_minute_of_day=6 * 60, seed=11, device="cuda:0", dtype=torch.float64)
    first = torch.where((mt >= 0) & (ma > 0), mt, torch.full_like(mt, 1 << 30)).min(0).values      # every env's first meal
    j = int((first.double() - 15.0).abs().argmin())
    assert 8 <= int(first[j]) <= 25, int(first[j])
    mt[:, :shared] = mt[:, j:j + 1]; ma[:, :shared] = ma[:, j:j + 1]
    return mt, ma


def _action(b, k):
    return b * (0.5 + 0.25 * (k % 7))


def _run(n, minutes, form, blocks, mt, ma):
    """-> the env after `minutes` launches and its BG after every tenth"""
    import torch
    pid = np.arange(n) % 30
    e = plain_env(patient=pid, sensor="Navigator", dtype=torch.float64, noise="philox", seed=4, n_sub=4, extra_outputs=False)
    e.set_option("adaptive_gut", form)
    e.set_option("s1_blocks", blocks)
    e.set_meals(mt, ma)
    e.reset()
    b = torch.as_tensor(basal_of(pid), device="cuda:0", dtype=torch.float64)
    bgs = []
    for k in range(minutes):
        e.step(_action(b, k))
        if k % 10 == 9:
            bgs.append(e.bg.clone())
    return e, bgs


@pytest.fixture(scope="module")
def shape1():
    """one workgroup over 40 chunks for 60 minutes: in place, set aside, and set aside once more from the same reset"""
    mt, ma = _tables(N1, SHARED1)
    runs = {name: _run(N1, K1, form, 1, mt, ma) for name, form in (("in_place", 2), ("set_aside", 3), ("again", 3))}
    return runs, mt, ma


def _compare(a, b, bgs_a, bgs_b):
    import torch
    for k, (x, y) in enumerate(zip(bgs_a, bgs_b)):
        assert float((x - y).abs().max()) < TOL, 10 * k + 9
    d = {key: float((getattr(a, key).double() - getattr(b, key).double()).abs().max()) for key in ("bg", "cgm", "reward", "x")}
    print("set aside against in place: max |difference|", d)
    assert torch.equal(a.t, b.t) and torch.equal(a.done, b.done)
    assert d["bg"] < TOL and d["cgm"] < TOL and d["reward"] < TOL and d["x"] < TOL_X, d
    assert a.sync() == 0 and b.sync() == 0


def test_one_workgroup_more_chunks_than_waves(shape1):
    runs, _, _ = shape1
    (a, bgs_a), (b, bgs_b) = runs["in_place"], runs["set_aside"]
    assert int(b.t.min()) == K1 == int(b.t.max())
    _compare(a, b, bgs_a, bgs_b)


def test_fewer_chunks_than_waves():
    mt, ma = _tables(N2, SHARED2)
    a, bgs_a = _run(N2, K2, 2, 0, mt, ma)
    b, bgs_b = _run(N2, K2, 3, 0, mt, ma)
    assert int(b.t.min()) == K2 == int(b.t.max())
    _compare(a, b, bgs_a, bgs_b)


def test_result_does_not_depend_on_which_wave_drew_which_chunk(shape1):
    import torch
    runs, _, _ = shape1
    (a, bgs_a), (b, bgs_b) = runs["set_aside"], runs["again"]
    for key in OUT:
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert all(torch.equal(x, y) for x, y in zip(bgs_a, bgs_b))
    assert a.sync() == 0 and b.sync() == 0


def test_set_aside_form_against_the_oracle(shape1):
    """the first 300 envs of shape 1 (all on the shared meal plan) on the oracle with the normals, meals and actions the
    kernel used; the rule lists more than 128 envs of the workgroup in one minute, so that both the inputs parked in LDS
    and the groups fetched again are behind the figures compared"""
    import torch
    from oracle import t1d_oracle as O
    from support import dense_cho
    _, mt, ma = shape1
    sample = np.arange(N_ORACLE)
    pid = np.arange(N1) % 30
    e = plain_env(patient=pid, sensor="Navigator", dtype=torch.float64, noise="philox", seed=4, n_sub=4, extra_outputs=False)
    e.set_option("adaptive_gut", 3)
    e.set_option("s1_blocks", 1)
    e.set_meals(mt, ma)
    z = e.philox_normals(1 + 10 * (1 + K1 // 150), draw0=0, episode=1)[:, :N_ORACLE].cpu().numpy()
    cho = dense_cho(mt, ma, sample, K1)
    orc = O.OracleEnv(pid[sample], sensor="Navigator", normals=z, integrator="split_adaptive", n_sub=4)
    o0, r0 = e.reset(), orc.reset()
    assert np.abs(o0[:N_ORACLE].cpu().numpy() - r0["cgm"]).max() < 1e-9
    b = torch.as_tensor(basal_of(pid), device="cuda:0", dtype=torch.float64)
    worst = {"bg": 0.0, "cgm": 0.0, "reward": 0.0}
    listed = 0
    for k in range(K1):
        a = _action(b, k)
        e.step(a)
        before = orc.level_count.copy()
        r = orc.step(a[:N_ORACLE].cpu().numpy(), None, cho[k:k + 1])
        listed = max(listed, int((orc.level_count - before)[2]))
        for key in worst:
            worst[key] = max(worst[key], float(np.abs(getattr(e, key)[:N_ORACLE].cpu().numpy() - r[key]).max()))
    ex = float(np.abs(e.x[:, :N_ORACLE].cpu().numpy() - orc.x).max())
    print("set-aside form against the oracle: max |difference|", worst, "states", ex, "most envs of the 300 at level 2 in one minute", listed)
    # envs of one patient on the shared plan take the same actions, so the 640 sharing envs hold at least twice these
    assert 2 * listed > 128, listed
    assert worst["bg"] < TOL_ORACLE and worst["cgm"] < TOL_ORACLE and worst["reward"] < 1e-6 and ex < 1e-6, (worst, ex)
    assert e.sync() == 0
