"""oracle/t1d_streams.py, the host restatement of the device's random streams, against what does not share its code:
Random123's known answers for Philox4x32-10, rocRAND's own host-callable generator (streams_probe.cpp), and the analytic
law of the meal scenario.  Then the census that lets test_gpu_streams.py compare every meal exactly: no candidate of the
compared cases is near a rounding tie.  No device."""
import functools
import os
import subprocess

import numpy as np
import pytest

import support
from support import DAYS, MEAL_CASES, RESTART_EPISODES, SAME_MINUTE_GIDS

HERE = os.path.dirname(os.path.abspath(__file__))
S = support.streams()

KNOWN_ANSWERS = (          # Random123 kat_vectors, philox4x32 10: counter, key, result
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def test_philox4x32_10_known_answers():
    for counter, key, want in KNOWN_ANSWERS:
        assert tuple(int(w) for w in S.philox4x32_10(counter, key)) == want
    # vectorised: the three at once
    got = S.philox4x32_10(np.array([k[0] for k in KNOWN_ANSWERS]).T, np.array([k[1] for k in KNOWN_ANSWERS]).T)
    assert np.array_equal(np.stack(got).T, np.array([k[2] for k in KNOWN_ANSWERS], dtype=np.uint64))


def _offset(episode, pair, word=0):
    return 4 * ((episode << 24) + pair) + word


PROBE_TABLE = [            # (seed, subsequence, word offset)
    (0, 0, 0),
    (0x123456789abcdef0, 0x100000005, _offset(3, 7)),
    (11, 2 ** 32 - 1, 0), (11, 2 ** 32, 0), (11, 2 ** 32 + 1, 8),                       # subsequences straddling 2^32
    (11, 2 ** 40 + 3, _offset(1, 3)), (11, 2 ** 63 - 1, 4),
    (5, 7, _offset(255, 2 ** 24 - 1)), (5, 7, _offset(256, 0)), (5, 7, _offset(256, 1)),   # block indices straddling 2^32
    (5, 7, _offset(255, 2 ** 24 - 1, 2)),                                               # ... inside one rocrand4
    (5, 2 ** 32 - 65, _offset(2 ** 32 - 1, 0)), (5, 2 ** 32 + 64, _offset(2 ** 32 - 1, 2 ** 24 - 1)),   # the last episode
    (0x9E3779B97F4A7C15, 1, 0), (0xFFFFFFFF00000000, 1, 0), (0x00000000FFFFFFFF, 1, 0),   # a seed's high word
    (11 ^ S.SCENARIO_KEY, 4095, 8 * 17), (11 ^ S.SCENARIO_KEY, 2 ** 32 + 3, 8 * 17 + 4),
    (3, 9, 1), (3, 9, 2), (3, 9, 3), (3, 9, 5), (3, 9, _offset(1, 0, 3)), (3, 2 ** 32, 4 * 2 ** 32 - 1),   # offsets not divisible by 4
]


def _as_double(word):
    return np.array([int(word, 16)], dtype=np.uint64).view(np.float64)[0]


def test_restatement_equals_rocrand_host_generator(tmp_path):
    """streams_probe.cpp runs rocrand_init / rocrand4 / rocrand_uniform_double2 / rocrand_normal_double2 on the host: words
    and uniforms must be equal, normals within 1 ulp (rocRAND's host branch computes sin(w * pi), as the float64 restatement
    does, but with the C library's sin, cos and log)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "streams_probe")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", os.path.join(HERE, "streams_probe.cpp"),
                           "-o", exe])
    args = ["%x" % v for row in PROBE_TABLE for v in row]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(PROBE_TABLE)
    worst = 0.0
    for (seed, sub, off), line in zip(PROBE_TABLE, lines):
        f = line.split()
        assert [int(v, 16) for v in f[:3]] == [seed, sub, off], line
        w = S.words4(seed, sub, off)
        assert [int(v) for v in w] == [int(v, 16) for v in f[3:7]], line
        ux, uy = S.uniform_double2(w)
        assert (float(ux), float(uy)) == (_as_double(f[7]), _as_double(f[8])), line
        # n: the normals of these four words; c: those of the next four (a uniform pair was drawn before them)
        for ww, cols in ((w, f[9:11]), (S.words4(seed, sub, off + 4), f[11:13])):
            x, y, _ = S.normal_double2(ww)
            for mine, theirs in ((float(x), _as_double(cols[0])), (float(y), _as_double(cols[1]))):
                ulps = abs(mine - theirs) / np.spacing(abs(theirs))
                worst = max(worst, ulps)
                assert ulps <= 1.0, (line, mine, theirs)
    print("normals against rocRAND's host branch: worst %.2f ulp over %d values" % (worst, 4 * len(PROBE_TABLE)))


def test_draw_map_of_philox_normals():
    """the draw-to-pair map as include/t1d.h words it, on the rows themselves"""
    want = {-3: (1, 0), -2: (1, 1), -1: (2, 0), 0: (0, 0), 1: (3, 0), 2: (3, 1), 10: (7, 1), 11: (8, 0), 20: (12, 1), 21: (13, 0), 25: (15, 0)}
    for d, (pair, el) in want.items():
        assert S.draw_pair(d) == (pair, el)
    r = S.normals(7, 2 ** 32 - 2, 5, 256, -3, 29)
    gid = np.arange(5, dtype=np.uint64) + np.uint64(2 ** 32 - 2)
    for d, (pair, el) in want.items():
        assert np.array_equal(r.z[d + 3], S.philox_pair(7, gid, 256, pair)[el]), d
    # cutting the range differently or shifting the envs addresses the same draws
    assert np.array_equal(S.normals(7, 2 ** 32 - 1, 4, 256, 5, 9).z, r.z[8:17, 1:])


def test_float64_normals_against_high_precision():
    """The yardstick of test_gpu_streams.py stays what its reasoning says: in units of eps * s the float64 restatement
    is off by the rounding of w * pi and of pi itself, up to 2 pi * (1/2 + 0.18) eps = 4.3 in the argument of sin / cos,
    plus half an ulp each for sin and the product and about one for s -- below 6.3, measured near 3."""
    worst = 0.0
    for seed, off, ep in ((0, 0, 0), (support.NORMALS_SEEDS[1], support.NORMALS_OFFSETS[1], 256)):
        ref = support.normals_reference(seed, off, ep)
        worst = max(worst, support.normal_error(ref.z, ref).max())
        assert np.array_equal(ref.hi + ref.lo, ref.hi) and np.abs(ref.lo).max() < 1e-15       # hi is the rounded value
    print("float64 restatement against mpmath: worst %.2f eps s" % worst)
    assert 0.5 < worst <= 6.3


# ------------------------------------------------------------------------------------------------ the meal law
LAW_N = 1 << 18


@functools.lru_cache(maxsize=None)
def _law_sample():
    return S.random_meals(support.STREAM_SEED, 0, LAW_N, 2, 0)


def _chi2_p(counts, prob):
    """p-value of Pearson's chi-square of `counts` against the bin probabilities `prob`; tail bins pooled until each
    expects at least 5"""
    from scipy.stats import chi2
    counts, expect = np.asarray(counts, dtype=np.float64), np.asarray(prob) * np.sum(counts)
    assert abs(np.sum(prob) - 1.0) < 1e-12
    small = np.nonzero(expect < 5.0)[0]
    mode = int(np.argmax(expect))
    lo = int(small[small < mode].max()) + 1 if (small < mode).any() else 0          # everything below lo joins bin lo,
    hi = int(small[small > mode].min()) if (small > mode).any() else len(expect)    # everything from hi on joins bin hi - 1
    counts[lo] += counts[:lo].sum(); expect[lo] += expect[:lo].sum()
    counts[hi - 1] += counts[hi:].sum(); expect[hi - 1] += expect[hi:].sum()
    counts, expect = counts[lo:hi], expect[lo:hi]
    assert expect.min() >= 5.0
    return float(chi2.sf(np.sum((counts - expect) ** 2 / expect), len(expect) - 1))


@pytest.mark.parametrize("k", range(6))
def test_meal_restatement_follows_the_analytic_law(k):
    """Seed 11, 2^18 envs, the two kept days, window k: the minute histogram against the truncated normal integrated over
    each minute's rounding interval, the grams histogram against the rounded, clamped normal, the presence rate against p.
    Every p-value >= 1e-4, |z| <= 4."""
    from scipy.special import ndtr
    c = _law_sample().cand
    p, lb, ub, mu, sd, g_mu, g_sd = S.WINDOWS[k]
    lb, ub, mu = 60 * lb, 60 * ub, 60.0 * mu
    kept = c["kept"][:2, k]
    assert np.array_equal(kept, c["present"][:2, k] & ~c["same_minute"][:2, k]) and not c["kept"][2, k].any()
    # minutes: bin m collects (m - 1/2, m + 1/2) cut at the window's bounds
    m = np.arange(lb, ub + 1)
    edges_lo, edges_hi = np.maximum(m - 0.5, lb), np.minimum(m + 0.5, ub)
    pa, pb = ndtr((lb - mu) / sd), ndtr((ub - mu) / sd)
    prob = (ndtr((edges_hi - mu) / sd) - ndtr((edges_lo - mu) / sd)) / (pb - pa)
    tod = c["tod"][:2, k][kept].astype(np.int64)
    assert tod.min() >= lb and tod.max() <= ub
    p_time = _chi2_p(np.bincount(tod - lb, minlength=len(m)), prob)
    # grams: bin 0 collects the clamp
    grams = c["grams"][:2, k][kept].astype(np.int64)
    assert grams.min() >= 0
    top = max(int(grams.max()), int(g_mu + 8 * g_sd)) + 1
    g = np.arange(top + 1)
    prob_g = ndtr((g + 0.5 - g_mu) / g_sd) - np.where(g == 0, 0.0, ndtr((g - 0.5 - g_mu) / g_sd))
    prob_g[-1] = 1.0 - prob_g[:-1].sum()
    p_grams = _chi2_p(np.bincount(grams, minlength=top + 1), prob_g)
    n_cand = 2 * LAW_N
    z = (c["present"][:2, k].sum() - n_cand * p) / np.sqrt(n_cand * p * (1.0 - p))
    print("window %d: %d meals, p(minutes) %.3g, p(grams) %.3g, z(presence) %+.2f" % (k, kept.sum(), p_time, p_grams, z))
    assert p_time >= 1e-4 and p_grams >= 1e-4 and abs(z) <= 4.0


# ------------------------------------------------------------------------------------------------ what the GPU test relies on
def _compared():
    """every Meals that test_gpu_streams.py compares with the device"""
    for case in MEAL_CASES:
        yield case, support.meal_reference(case)
    for k in RESTART_EPISODES:
        yield "restart_%d" % k, support.restart_reference(k)[1]


def test_no_compared_candidate_is_near_a_rounding_tie():
    """Device and host differ in the last bits of erfc, erfinv, log and sincospi: parts in 1e16 of a time of at most 1 440
    minutes (one ulp: 2.3e-13) or of some 100 grams.  With every candidate at least 1e-9 from a rounding tie, four orders
    above that, the rounded values must agree, and the GPU test leaves no entry out."""
    worst_t = worst_g = 1.0
    for case, m in _compared():
        worst_t, worst_g = min(worst_t, m.cand["t_tie"].min()), min(worst_g, m.cand["g_tie"].min())
        assert m.cand["t_tie"].min() > 1e-9 and m.cand["g_tie"].min() > 1e-9, case
        # the clamp of the time of day to its window is a guard: it changes nothing
        assert np.array_equal(m.cand["tod"], np.rint(m.cand["t_raw"])), case
    print("nearest rounding tie: %.3g minutes, %.3g grams" % (worst_t, worst_g))


def test_same_minute_envs_drop_a_meal():
    for g in SAME_MINUTE_GIDS:
        m = support.meal_reference("same_minute_%d" % g)
        dropped = m.cand["same_minute"].any(axis=(0, 1))
        assert dropped.tolist() == [False, True, False], g
        d, k = [int(v[0]) for v in np.nonzero(m.cand["same_minute"][:, :, 1])]
        assert k > 0 and m.cand["kept"][d, k - 1, 1] and m.cand["minute"][d, k - 1, 1] == m.cand["minute"][d, k, 1]
        assert (m.time[:, 1] == m.cand["minute"][d, k, 1]).sum() == 1 and m.amt[:, 1][m.time[:, 1] == m.cand["minute"][d, k, 1]] \
            == m.cand["grams"][d, k - 1, 1]                                       # the earlier meal is the one that stays


def test_compared_tables_cover_the_branches():
    support.meal_tables_cover_the_branches()


def test_meal_tables_are_well_formed():
    for case, m in _compared():
        rows, n = m.time.shape
        assert rows == 6 * (DAYS + 1)
        used = m.time != S.MEAL_UNUSED
        assert np.array_equal(used.sum(axis=0), m.cand["kept"].sum(axis=(0, 1))), case
        assert not (used[1:] & ~used[:-1]).any(), case                                  # the used rows come first
        t = np.where(used, m.time.astype(np.int64), np.int64(2) ** 40 + np.arange(rows)[:, None])
        assert (np.diff(t, axis=0) > 0).all(), case                                   # strictly ascending
        assert m.time[used].min() >= 0 and m.time[used].max() < 1440 * DAYS and (m.amt[~used] == 0).all(), case
        assert not np.signbit(m.amt).any() and np.array_equal(m.amt, np.rint(m.amt)), case
