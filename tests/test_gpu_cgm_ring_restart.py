"""The CGM ring (cgm_history=True, BatchedT1DSimEnv.cgm_window) across episodes that end inside a launch: after collect_mlp /
collect_pid / collect_bb / collect_mlp_dopri5 with on_done="restart" the ring is what the documented loop of one-step roll-outs
and restart_done() leaves, bit for bit, and the shadow clock is gone; with on_done="continue" the clock goes on and the ring
holds the last observation.  128 envs of one adult patient (two waves, one policy of 128), Dexcom, fp64, Philox noise; the
glucose words of envs 64 .. 127 are tripled after reset(), so that their first step ends the episode above 350 mg/dL: with K = 1
the last step of the call ends episodes in half of the batch, with K = 2 it ends none and the restarts lie one step back."""
import pytest

from support import DAYS, MLP_TRACE, episode_stats, gpu_torch, loop_of_entry_points, plain_env, random_policy, stats
from support_ctrl import feature_policy, run_collector, run_loop

pytestmark = pytest.mark.gpu

N, HIGH_FROM, FACTOR = 128, 64, 3.0


def _env(exact=False):
    torch = gpu_torch()
    e = plain_env(patient="adult#001", n_envs=N, sensor="Dexcom", dtype=torch.float64, seed=3, noise="philox", cgm_history=True,
                  integrator="dopri5" if exact else None)
    e.start_minute = torch.zeros(N, dtype=torch.int32, device=e.device)     # the loops' host features read it before a restart
    e.reset()
    for row in (3, 4, 12):                                    # plasma, tissue and subcutaneous glucose
        e.x[row, HIGH_FROM:] *= FACTOR
    return e


def _same_ring(a, b):
    torch = gpu_torch()
    wa, wb = a.cgm_window(), b.cgm_window()
    assert wa.shape == (a.window, N)
    assert torch.equal(wa.isnan(), wb.isnan())
    assert torch.equal(wa.view(torch.int64), wb.view(torch.int64))
    assert a._clock is None and b._clock is None


def _precondition(done_rows, K):
    """done_rows: the loop's done [K, n].  K = 1: the last step ended some episodes and not others; K = 2: it ended none, the
    step before it did"""
    last = done_rows[K - 1].bool()
    if K == 1:
        assert bool(last.any()) and not bool(last.all())
    else:
        assert not bool(last.any()) and bool(done_rows[0].bool().any())


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("exact", [False, True], ids=["collect_mlp", "collect_mlp_dopri5"])
def test_ring_after_the_policy_collectors_is_the_loops(exact, K):
    torch = gpu_torch()
    pol = random_policy()
    A, B = _env(exact), _env(exact)
    collect = A.collect_mlp_dopri5 if exact else A.collect_mlp
    collect(K, pol, on_done="restart", days=DAYS)
    assert A.sync() == 0
    tr = B.new_trace(K, columns=MLP_TRACE + ("reward", "done"))
    loop_of_entry_points(B, pol, K, stats(B), tr, torch.zeros(N, dtype=B.dtype, device=B.device), episode_stats(B), exact)
    _precondition(tr["done"][1:], K)
    _same_ring(A, B)


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("kind", ["pid", "bb"])
def test_ring_after_the_controllers_collectors_is_the_loops(kind, K):
    pol = feature_policy()
    A = run_collector(_env(), kind, "stock", pol, (K,))["e"]
    loop = run_loop(_env(), kind, "stock", pol, K)
    _precondition(loop["tr"]["done"][1:], K)
    _same_ring(A, loop["e"])


def test_continue_keeps_the_clock_and_leaves_the_last_observation():
    torch = gpu_torch()
    e = _env()
    e.collect_mlp(2, random_policy(), on_done="continue")
    assert e.sync() == 0
    assert e._clock == 2 * e.minutes_per_step
    w = e.cgm_window()
    assert torch.equal(w[-1].view(torch.int64), e.cgm.view(torch.int64)) and not bool(e.cgm.isnan().any())
    assert bool(w[:-1].isnan().all())
