"""The device's random streams against oracle/t1d_streams.py, the host restatement that test_streams_host.py ties to
Random123's known answers, to rocRAND's host generator and to the scenario's analytic law: t1d_philox_normals draw for draw
(within the error of a float64 Box-Muller), t1d_random_meals and the meal columns of t1d_restart_done entry for entry,
exactly.  Every other test of sensor noise, initial glucose, exploration noise and restarts compares with these entry
points, so this file is what anchors them outside the device code."""
import ctypes as C
import functools

import numpy as np
import pytest

import support
from support import DAYS, MEAL_CASES, NORMALS_DRAW0, NORMALS_DRAWS, NORMALS_N, RESTART_EPISODES, RESTART_N, RESTART_SEED, STREAM_OFF, \
    STREAM_SEED

pytestmark = pytest.mark.gpu

NORMALS_CASES = [(s, o, k) for s in support.NORMALS_SEEDS for o in support.NORMALS_OFFSETS for k in support.NORMALS_EPISODES]


@functools.lru_cache(maxsize=None)
def _ctx_env():
    """an env for its context: t1d_philox_normals takes seed, offset and episode as arguments"""
    return support.plain_env(patient="adult#001", n_envs=64)


def _device_normals(seed, env_offset, n, episode, draw0, n_draws):
    torch = support.gpu_torch()
    e = _ctx_env()
    out = torch.empty(n_draws, n, dtype=torch.float64, device=e.device)
    with torch.cuda.device(e.device):
        assert e._L.t1d_philox_normals(e._ctx, seed, env_offset, n, episode, draw0, n_draws, C.c_void_p(out.data_ptr()), e._stream()) == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("seed,env_offset,episode", NORMALS_CASES,
                         ids=["seed%x-off%x-ep%x" % c for c in NORMALS_CASES])
def test_philox_normals_equal_the_restatement_draw_for_draw(seed, env_offset, episode):
    """130 envs, draws -3 .. 25: the random_init_bg draws, the AR(1) start, two and a half noise blocks, both elements of
    every pair.  Yardstick: the error of the float64 restatement (sin(w * pi), numpy's log and sqrt) against the mpmath
    value of the same draws, in units of eps * s with s the pair's sqrt(-2 ln u) -- about 3, from the rounding of w * pi.
    The device (sincospi, ocml's log) must stay within twice that; a wrong pair, element, episode stride, subsequence or
    key word is an error of order 1, some 1e15 of these units.
    The yardstick itself must stay below the 6.3 that test_streams_host.py reasons out, so that a restatement at odds with
    itself cannot widen the bound.
    Measured on an MI355X over the 30 cases: device 0.92 .. 1.27 eps s, yardstick 2.83 .. 3.15 (profiles/streams)."""
    ref = support.normals_reference(seed, env_offset, episode)
    yardstick = float(support.normal_error(ref.z, ref).max())
    assert yardstick <= 6.3
    z = _device_normals(seed, env_offset, NORMALS_N, episode, NORMALS_DRAW0, NORMALS_DRAWS)
    err = float(support.normal_error(z, ref).max())
    print("t1d_philox_normals seed %#x offset %#x episode %#x: device %.2f eps s, float64 restatement %.2f eps s"
          % (seed, env_offset, episode, err, yardstick))
    assert np.isfinite(z).all() and err <= 2.0 * yardstick
    # position-keyed: other cuts of the draw range and other first envs address the same draws
    cuts = ((-3, 2), (-1, 5), (4, 22))
    assert sum(c[1] for c in cuts) == NORMALS_DRAWS
    parts = [_device_normals(seed, env_offset, NORMALS_N, episode, d0, nd) for d0, nd in cuts]
    assert np.array_equal(np.concatenate(parts).view(np.uint64), z.view(np.uint64))
    for shift in (1, 64):
        moved = _device_normals(seed, env_offset + shift, NORMALS_N - shift, episode, NORMALS_DRAW0, NORMALS_DRAWS)
        assert np.array_equal(moved.view(np.uint64), np.ascontiguousarray(z[:, shift:]).view(np.uint64)), shift


def test_compared_meal_tables_cover_the_branches():
    support.meal_tables_cover_the_branches()


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("case", list(MEAL_CASES))
def test_random_meals_equal_the_restatement_exactly(case, dtype_name):
    """every entry of both tables: times as int32, grams bit for bit (whole numbers, so fp32 holds them exactly; a -0 would
    fail).  test_streams_host.py shows that no candidate of these cases is within 1e-9 of a rounding tie, so nothing is
    left out."""
    torch = support.gpu_torch()
    from simglucose_amd.scenario_batch import random_meal_tables
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    off, n, start = MEAL_CASES[case]
    ref = support.meal_reference(case)
    start = torch.as_tensor(support.start_table(n)) if isinstance(start, str) else start
    mt, ma = random_meal_tables(n, days=DAYS, start_minute_of_day=start, seed=STREAM_SEED, dtype=dtype, env_offset=off)
    mt, ma = mt.cpu().numpy(), ma.cpu().numpy()
    assert mt.dtype == np.int32 and mt.shape == ref.time.shape and ma.shape == ref.amt.shape
    bad = np.nonzero(mt != ref.time)
    assert len(bad[0]) == 0, "times differ at (row, env) %s: device %s, restatement %s" % (list(zip(*bad))[:5], mt[bad][:5], ref.time[bad][:5])
    word = np.uint64 if dtype_name == "f64" else np.uint32
    want = ref.amt.astype(ma.dtype)
    assert np.array_equal(want.astype(np.float64), ref.amt)
    bad = np.nonzero(ma.view(word) != want.view(word))
    assert len(bad[0]) == 0, "grams differ at (row, env) %s: device %s, restatement %s" % (list(zip(*bad))[:5], ma[bad][:5], want[bad][:5])


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_restart_done_writes_the_restated_start_and_meals(dtype_name):
    """130 envs across 2^32, all restarted at the episode counters 0, 1 and 5: start_minute = 60 start_hours(seed, k, g) and
    the meal columns are random_meals(seed * 7919 + k, g, days, start) of the restatement."""
    torch = support.gpu_torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    dtype = torch.float64 if dtype_name == "f64" else torch.float32
    e = BatchedT1DSimEnv(patient=["child#001", "adult#001"] * (RESTART_N // 2), sensor="Dexcom", pump="Insulet", dtype=dtype, n_sub=4,
                         seed=RESTART_SEED, env_offset=STREAM_OFF, noise="philox", random_init_bg=True)
    ones = torch.ones(RESTART_N, dtype=torch.uint8, device=e.device)
    word = np.uint64 if dtype_name == "f64" else np.uint32
    for k in RESTART_EPISODES:
        e.episode.fill_(k)
        e.restart_done(mask=ones, days=DAYS, reset_outputs=True)
        assert e.sync() == 0
        start, ref = support.restart_reference(k)
        assert len(np.unique(start)) > 12                                          # the envs start at many hours
        assert np.array_equal(e.episode.cpu().numpy(), np.full(RESTART_N, k + 1)), k
        assert np.array_equal(e.start_minute.cpu().numpy().astype(np.int64), start), k
        mt, ma = e.meal_time.cpu().numpy(), e.meal_amt.cpu().numpy()
        assert mt.dtype == np.int32 and np.array_equal(mt, ref.time), k
        assert np.array_equal(ma.view(word), ref.amt.astype(ma.dtype).view(word)), k
        assert (ref.time != 0x7FFFFFFF).sum() > 6 * RESTART_N and (ref.cand["present"] & (ref.cand["minute"] < 0)).any(), k
