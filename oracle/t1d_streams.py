"""The device's random streams restated on the host, draw for draw: the normals of t1d_philox_normals (sensor noise,
random_init_bg, the collectors' exploration noise) and the meal tables of t1d_random_meals (and through it of
t1d_restart_done).  numpy, vectorised over envs.  Written from the comments of include/t1d.h and from rocRAND's headers
(rocrand_philox4x32_10.h, rocrand_uniform.h, rocrand_normal.h), not from the kernels: the integer part of Philox is
bit-reproducible, so the words and the uniforms are exact, and what is left between this file and the device is the last
bits of log, sqrt, sin / cos and erfinv.

Conventions (rocRAND's): counter = (block lo, block hi, subsequence lo, subsequence hi), key = (seed lo, seed hi); the word at
offset o of a subsequence is word o % 4 of block o / 4.  Seeds, subsequences and block indices are integers mod 2^64; pass
Python ints or uint64 arrays."""
import collections

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
EPISODE_STRIDE_LOG2 = 24                 # an episode owns 2^24 pairs (t1d_philox_normals)
SCENARIO_KEY = 0x5ce9a7105ce9a710        # t1d_random_meals: key = seed ^ SCENARIO_KEY
MEAL_UNUSED = 0x7FFFFFFF
TWO_M53 = 2.0 ** -53
MASK64 = (1 << 64) - 1


def _u64(v):
    """integers mod 2^64 -> uint64 array (Python ints of any sign, int64 or uint64 arrays)"""
    if isinstance(v, (int, np.integer)):
        return np.asarray(int(v) & MASK64, dtype=np.uint64)
    v = np.asarray(v)
    return v.astype(np.uint64) if v.dtype != np.uint64 else v


# ------------------------------------------------------------------------------------------------ Philox4x32-10
def philox4x32_10(counter, key):
    """Random123's Philox4x32-10: counter = four 32-bit words, key = two (array-likes that broadcast) -> four uint64
    arrays holding 32-bit words"""
    c0, c1, c2, c3 = (_u64(c) & M32 for c in counter)
    k0, k1 = (_u64(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2                    # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & M32, (p0 >> _S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def block(seed, subsequence, block_index):
    """the four words rocRAND holds after rocrand_init(seed, subsequence, 4 * block_index)"""
    s, q, b = _u64(seed), _u64(subsequence), _u64(block_index)
    return philox4x32_10((b & M32, b >> _S32, q & M32, q >> _S32), (s & M32, s >> _S32))


def words4(seed, subsequence, offset):
    """rocrand4 after rocrand_init(seed, subsequence, offset) for any word offset: four consecutive words of the stream,
    which straddle two blocks when offset is no multiple of 4 -> uint64 array [4, ...]"""
    o = _u64(offset)
    b, r = o >> np.uint64(2), (o & np.uint64(3)).astype(np.int64)
    w = np.stack(block(seed, subsequence, b) + block(seed, subsequence, b + np.uint64(1)))            # [8, ...]
    idx = np.broadcast_to(r, w.shape[1:])[None] + np.arange(4).reshape((4,) + (1,) * (w.ndim - 1))
    return np.take_along_axis(w, idx, axis=0)


# ------------------------------------------------------------------------------------------------ rocRAND's conversions
def uniform_double2(w):
    """rocrand_uniform.h, uniform_distribution_double2(uint4): 53 bits = v.x below, the top 21 bits of v.y above;
    (bits + 1) 2^-53, in (0, 1] -> (x, y)"""
    one = lambda lo, hi: TWO_M53 + (lo | ((hi >> np.uint64(11)) << _S32)).astype(np.float64) * TWO_M53
    return one(w[0], w[1]), one(w[2], w[3])


def normal_bits(w):
    """rocrand_normal.h, box_muller_double(uint4): u = (v.x ^ (v.y << 21) + 1) 2^-53 in (0, 1] -- not the uniform path's
    53 bits -- and w = (v.z ^ (v.w << 21) + 1) 2^-52 in (0, 2], the angle in units of pi -> (u, w)"""
    mix = lambda lo, hi: (lo ^ (hi << np.uint64(21))).astype(np.float64)
    return TWO_M53 + mix(w[0], w[1]) * TWO_M53, 2.0 * TWO_M53 + mix(w[2], w[3]) * (2.0 * TWO_M53)


def normal_double2(w):
    """Box-Muller as the host branch of rocRAND writes it: s = sqrt(-2 ln u), (sin(w pi) s, cos(w pi) s) -> (x, y, s)"""
    u, ang = normal_bits(w)
    s = np.sqrt(-2.0 * np.log(u))
    return np.sin(ang * np.pi) * s, np.cos(ang * np.pi) * s, s


def normal_double2_mp(w, bits=120):
    """the same pair from mpmath at `bits` bits with sinpi / cospi, each value as a double-double: -> (x_hi, x_lo, y_hi,
    y_lo) with x = x_hi + x_lo to ~1e-32 relative"""
    import mpmath
    u, ang = normal_bits(w)
    shape = u.shape
    out = np.empty((4, u.size))
    with mpmath.workprec(bits):
        for j, (uj, aj) in enumerate(zip(u.ravel().tolist(), ang.ravel().tolist())):
            s = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(uj)))
            for c, v in ((0, mpmath.sinpi(mpmath.mpf(aj)) * s), (2, mpmath.cospi(mpmath.mpf(aj)) * s)):
                hi = float(v)
                out[c, j], out[c + 1, j] = hi, float(v - mpmath.mpf(hi))
    return tuple(o.reshape(shape) for o in out)


# ------------------------------------------------------------------------------------------------ t1d_philox_normals
def pair_block(episode, pair):
    """block index of pair `pair` of episode `episode`: an episode owns 2^24 pairs"""
    return (_u64(episode) << np.uint64(EPISODE_STRIDE_LOG2)) + _u64(pair)


def philox_pair(seed, gid, episode, pair):
    """the two normals of block (episode << 24) + pair of subsequence gid under key seed -> (x, y, s)"""
    return normal_double2(block(seed, gid, pair_block(episode, pair)))


def draw_pair(draw):
    """draw index of t1d_philox_normals -> (pair, element): -3, -2, -1 = pair 1 .x, pair 1 .y, pair 2 .x (random_init_bg);
    0 = pair 0 .x; 1 + 10 b + j = pair 3 + 5 b + j // 2, element j & 1"""
    d = int(draw)
    if d < -3:
        raise ValueError("draws start at -3")
    if d < 0:
        return 1 + (d + 3) // 2, (d + 3) & 1
    if d == 0:
        return 0, 0
    b, j = divmod(d - 1, 10)
    return 3 + 5 * b + j // 2, j & 1


Normals = collections.namedtuple("Normals", "z s hi lo")


def normals(seed, env_offset, n, episode, draw0, n_draws, mp=False):
    """out[r][i] = draw draw0 + r of env env_offset + i in episode `episode`, as t1d_philox_normals lays them out
    -> Normals: z float64 [n_draws, n]; s = sqrt(-2 ln u) of the draw's pair; with mp, hi + lo = the high-precision value"""
    gid = (_u64(env_offset) + np.arange(n, dtype=np.uint64))
    where = [draw_pair(draw0 + r) for r in range(n_draws)]
    pairs = sorted({p for p, _ in where})
    w = block(seed, gid[None, :], pair_block(episode, np.array(pairs, dtype=np.uint64))[:, None])        # [4] x [pairs, n]
    x, y, s = normal_double2(w)
    row = [pairs.index(p) for p, _ in where]
    el = np.array([e for _, e in where])[:, None]
    z = np.where(el == 0, x[row], y[row])
    hi = lo = None
    if mp:
        xh, xl, yh, yl = normal_double2_mp(w)
        hi, lo = np.where(el == 0, xh[row], yh[row]), np.where(el == 0, xl[row], yl[row])
    return Normals(z, s[row], hi, lo)


# ------------------------------------------------------------------------------------------------ t1d_random_meals
# (p, earliest, latest, mean [hours], sd [minutes], grams mean, grams sd) per window: include/t1d.h, scenario_gen.py:38-45
WINDOWS = ((0.95, 5, 9, 7, 60, 45, 10), (0.3, 9, 10, 9.5, 30, 10, 5), (0.95, 10, 14, 12, 60, 70, 10),
           (0.3, 14, 16, 15, 30, 10, 5), (0.95, 16, 20, 18, 60, 80, 10), (0.3, 20, 23, 21.5, 30, 10, 5))

Meals = collections.namedtuple("Meals", "time amt cand")


def _tie(v):
    """distance of v from the nearest point where rint changes its value (k + 1/2)"""
    return np.abs(v - np.floor(v) - 0.5)


def window_cdf(k):
    """(Phi_a, Phi_b) of window k: the normal CDF at its bounds"""
    from scipy.special import ndtr
    _, lb, ub, mu, sd, _, _ = WINDOWS[k]
    return float(ndtr((60.0 * lb - 60.0 * mu) / sd)), float(ndtr((60.0 * ub - 60.0 * mu) / sd))


def random_meals(seed, env_offset, n, days, start):
    """t1d_random_meals(seed, env_offset, n, days, start): start = minute of day, an int or an array [n]
    -> Meals: time int32 [6 (days + 1), n] (unused = INT32_MAX), amt float64 [rows, n] (whole grams: exact in fp32 too),
    cand = per candidate arrays [days + 1, 6, n]: present, t_raw (unrounded minute of day), tod, g_raw (unrounded grams),
    grams, minute, in_range, kept, same_minute (dropped for that alone), t_tie / g_tie (distance of t_raw / g_raw from a
    rounding tie)"""
    from scipy.special import ndtri
    key = (int(seed) & MASK64) ^ SCENARIO_KEY
    gid = _u64(env_offset) + np.arange(n, dtype=np.uint64)
    start = np.broadcast_to(np.asarray(start, dtype=np.int64), (n,))
    rows = 6 * (days + 1)
    time = np.full((rows, n), MEAL_UNUSED, dtype=np.int32)
    amt = np.zeros((rows, n))
    names = "present t_raw tod g_raw grams minute in_range kept same_minute t_tie g_tie".split()
    cand = {k: np.zeros((days + 1, 6, n), dtype=bool if k in ("present", "in_range", "kept", "same_minute") else np.float64)
            for k in names}
    filled = np.zeros(n, dtype=np.int64)
    last = np.full(n, -1, dtype=np.int64)
    cols = np.arange(n)
    for d in range(days + 1):
        for k, (p, lb, ub, mu, sd, g_mu, g_sd) in enumerate(WINDOWS):
            first = 2 * (6 * d + k)                                   # word offset 8 (6 d + k)
            ux, uy = uniform_double2(block(key, gid, first))
            gx, _, _ = normal_double2(block(key, gid, first + 1))
            pa, pb = window_cdf(k)
            present = ux <= p
            t_raw = 60.0 * mu + sd * ndtri(pa + uy * (pb - pa))
            tod = np.clip(np.rint(t_raw), 60.0 * lb, 60.0 * ub)
            g_raw = g_mu + g_sd * gx
            r = np.rint(g_raw)
            grams = np.where(r > 0.0, r, 0.0)
            minute = 1440 * d + tod.astype(np.int64) - start
            in_range = (minute >= 0) & (minute < 1440 * days)
            same = present & in_range & (minute == last)
            kept = present & in_range & ~same
            time[filled[kept], cols[kept]] = minute[kept]
            amt[filled[kept], cols[kept]] = grams[kept]
            filled += kept
            last = np.where(kept, minute, last)
            for name, v in zip(names, (present, t_raw, tod, g_raw, grams, minute, in_range, kept, same, _tie(t_raw), _tie(g_raw))):
                cand[name][d, k] = v
    return Meals(time, amt, cand)
