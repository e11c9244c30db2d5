"""The inputs and references of test_gpu_outcome.py on the host: that the inputs reach what they are meant to reach, and
that the references alone meet every condition the device is held to.  No GPU.

t1d_outcome_stats (include/t1d.h) is compared with: a percentile in exact rational arithmetic under a stated rounding bound
(support.percentile_reference), numpy's comparisons for the five counters, the oracle's report_cvga for the zones, and a
50-digit mpmath restatement of risk_index_trace (support.risk_reference).  None of the four shares code with the kernel; here
numpy's own percentile is put through the bound first, so that the bound is seen not to be fitted to the kernel."""
import math
from fractions import Fraction

import numpy as np
import pytest

import support
from oracle import t1d_oracle as O
from support import (CVGA_CLAUSES, CVGA_COMPARISONS, NAN_CASES, OUT_KINDS, OUT_NS, OUT_QS, OUT_ROWS, OUT_THRESHOLDS, RISK_CHUNKS,
                     RISK_N, RISK_ROWS)

DTYPES = ("f64", "f32")


def test_floor_of_the_rank_is_the_same_in_floating_point():
    """the bound takes floor((rows - 1) q / 100) to be the same in the kernel's order of operations, in numpy's and exactly"""
    for rows in OUT_ROWS + (support.NAN_ROWS, RISK_ROWS):
        for q in sum(OUT_QS, ()):
            pos, lo = support.rank_of(rows, q)
            assert math.floor((rows - 1) * q / 100.0) == lo == math.floor((rows - 1) * (q / 100.0)), (rows, q)
            assert abs(Fraction((rows - 1) * q / 100.0) - pos) <= 2 * support.OUT_U * pos, (rows, q)


@pytest.mark.parametrize("rows", OUT_ROWS)
def test_numpy_percentile_is_within_the_bound_of_the_rational_reference(rows):
    """np.percentile on the fp64 inputs (every kind of column, every pair of OUT_QS) against the exact percentile"""
    worst = np.zeros(2)
    for qs in OUT_QS:
        bg = support.outcome_columns(OUT_NS[-1], rows, "f64", qs)
        for q in qs:
            ref, bound = support.percentile_reference(bg, q, "f64")
            err = support.percentile_error(np.percentile(bg, q, axis=0), ref, bound)
            assert err.max() <= 1.0, (qs, q, int(err.argmax()), OUT_KINDS[err.argmax() % len(OUT_KINDS)], err.max())
            worst = np.maximum(worst, support.worst_by_kind(err))
    print("rows %d: np.percentile worst error / bound %.3f, sign_mixed columns %.3f" % (rows, worst[0], worst[1]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_columns_are_distinct_and_of_every_kind(dtype):
    """no two envs share a column (a misplaced lane shows), and the kinds hold what their names say"""
    rows, qs = 41, OUT_QS[0]
    bg = support.outcome_columns(OUT_NS[-1], rows, dtype, qs)
    assert bg.dtype == support.out_np(dtype) and np.isfinite(bg).all()
    assert len({bg[:, i].tobytes() for i in range(bg.shape[1])}) == bg.shape[1]
    s = np.sort(bg, axis=0)
    kind = np.array([OUT_KINDS.index(k) for k in OUT_KINDS])[np.arange(bg.shape[1]) % len(OUT_KINDS)]
    of = lambda name: np.flatnonzero(kind == OUT_KINDS.index(name))
    assert all(len(np.unique(bg[:, i])) == rows for i in of("distinct"))
    assert all(len(np.unique(bg[:, i])) == 1 for i in of("constant"))
    assert all(len(np.unique(bg[:, i])) == 2 for i in of("two_valued"))
    mixed = bg[:, of("sign_mixed")]
    tiny = np.finfo(bg.dtype).tiny
    assert (mixed < 0).any() and (mixed > 0).any() and ((mixed != 0) & (np.abs(mixed) < tiny)).any()
    assert (np.abs(mixed) >= (1e300 if dtype == "f64" else 1e38)).any()
    zeros = mixed[mixed == 0]
    assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()
    assert (bg[:, of("negative")] < 0).all()
    for q in qs:
        k = support.rank_of(rows, q)[1]
        assert all(s[k, i] == s[k + 1, i] and s[k - 1, i] < s[k, i] for i in of("tie_at_rank"))          # a tie exactly at k / k + 1
        assert all(s[k + 1, i] == np.nextafter(s[k, i], np.array(np.inf, bg.dtype)) for i in of("adjacent_at_rank"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_count_inputs_hold_every_threshold_and_its_neighbours(dtype):
    bg = support.outcome_threshold_inputs(OUT_NS[-1], 41, dtype)
    ft = bg.dtype.type
    for t in OUT_THRESHOLDS:
        for v in (np.nextafter(ft(t), ft(-np.inf)), ft(t), np.nextafter(ft(t), ft(np.inf))):
            assert (bg == v).any(), (t, v)
        assert np.nextafter(ft(t), ft(-np.inf)) < t < np.nextafter(ft(t), ft(np.inf))
    cnt = support.outcome_counts(bg)
    assert all(len(np.unique(row)) > 1 for row in cnt)                     # every counter differs between envs
    assert (cnt[:3].sum(0) == 41).all() and (cnt[3] <= cnt[0]).all() and (cnt[4] <= cnt[1]).all()
    assert np.array_equal(cnt / 41.0 * 100.0, O.report_percent_stats(bg.astype(np.float64)))
    # a `<=` for the `<` at 70 (and its likes) would move a count: the threshold itself is in no strict range
    assert (cnt[1] != (bg <= 70).sum(0)).any() and (cnt[0] != (bg >= 180).sum(0)).any()
    assert (cnt[3] != (bg >= 250).sum(0)).any() and (cnt[4] != (bg <= 50).sum(0)).any()
    assert (cnt[2] != ((bg > 70) & (bg <= 180)).sum(0)).any() and (cnt[2] != ((bg >= 70) & (bg < 180)).sum(0)).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_zone_grid_has_both_sides_of_every_comparison(dtype):
    bg, mn, mx = support.zone_grid(dtype)
    assert bg.shape[1] > 256 and np.array_equal(bg.min(0), mn) and np.array_equal(bg.max(0), mx)
    assert (mn < 50).any() and (mx > 400).any() and (mn > 400).any() and (mx < 50).any()           # beyond both clip bounds
    rmn, rmx, frac, zone = O.report_cvga(bg.astype(np.float64), 0.0, 100.0)
    assert np.array_equal(rmn, np.clip(mn, 50, 400)) and np.array_equal(rmx, np.clip(mx, 50, 400))
    assert np.array_equal(support.cvga_zone_codes(mn, mx), zone)
    assert set(zone) == {0, 1, 2, 3, 4, 5}
    alt = support.cvga_alternatives(mn, mx)
    for z, alts in CVGA_CLAUSES:                                           # every clause of C and D (and of the rest) occurs
        for a in range(len(alts)):
            assert (alt[z, a] & (zone == z)).any(), (z, a)
    where = {(float(a), float(b)): i for i, (a, b) in enumerate(zip(mn, mx))}
    for z, a, t in CVGA_COMPARISONS:
        name, op, b = CVGA_CLAUSES[z][1][a][t]
        moved = np.flatnonzero(support.cvga_zone_codes(mn, mx, flip=(z, a, t)) != zone)
        assert len(moved), (z, a, t)                                       # the comparison decides some env's zone ...
        v = mn if name == "mn" else mx
        assert (v[moved] == b).all()
        for i in moved:                                                    # ... and its neighbour one ulp away has another zone
            nb = np.nextafter(v[i], np.array(np.inf if op in (">", "<=") else -np.inf, v.dtype))
            j = where.get((float(nb), float(mx[i])) if name == "mn" else (float(mn[i]), float(nb)))
            if j is not None and zone[j] != zone[i]:
                break
        else:
            raise AssertionError("no pair of neighbours across %s %s %g" % (name, op, b))


@pytest.mark.parametrize("dtype", DTYPES)
def test_risk_inputs_hold_every_kind_of_row(dtype):
    bg = support.risk_inputs(dtype)
    assert bg.shape == (RISK_ROWS, RISK_N) and RISK_ROWS * RISK_N <= 130 * 70
    assert all(RISK_ROWS % c for c in RISK_CHUNKS if 1 < c != RISK_ROWS)
    assert (bg < 0).any() and (bg == 0).any() and np.signbit(bg[bg == 0]).any() and ((bg > 0) & (bg < 1)).any()
    assert (bg == 1).any() and np.isposinf(bg).any() and not np.isnan(bg).any()
    terms = support.risk_terms(bg)
    assert np.array_equal(np.vectorize(lambda v: v is None)(terms), ~(bg >= 1))
    seen_none = 0
    for chunk in RISK_CHUNKS:
        cnt, f, S = support.risk_reference(terms, chunk)
        assert cnt.shape == ((RISK_ROWS + chunk - 1) // chunk, RISK_N)
        none = cnt == 0
        seen_none += none.any()
        assert none[:, 6].all()                                            # the column without a usable row
        fin = np.array([[v is not None and math.isfinite(v) for v in row] for row in f])
        fv = np.array([[float(v) if ok else 0.0 for v, ok in zip(row, okr)] for row, okr in zip(f, fin)])
        assert (fv < 0).any() and (fv > 0).any()
        assert any(v is not None and v == math.inf for v in f[:, 4])       # the +Inf sample
        # the numpy restatement of the oracle agrees wherever f is finite (it turns LBGI of f = +Inf into NaN: inf * 0)
        with np.errstate(invalid="ignore"):
            L, H = O.report_risk_index_trace(bg.astype(np.float64), chunk)
        assert np.array_equal(np.isnan(H), none)
        want = 10.0 * fv * fv
        assert np.allclose(np.where(fin, L, 0), np.where(fv < 0, want, 0), rtol=1e-10, atol=1e-12)
        assert np.allclose(np.where(fin, H, 0), np.where(fv > 0, want, 0), rtol=1e-10, atol=1e-12)
    assert seen_none == len(RISK_CHUNKS)
    cnt, f, S = support.risk_reference(terms, 7)
    assert cnt[0, 5] == 0 and cnt[1, 5] == 7                               # the first week of env 5, and the one after
    cnt, f, S = support.risk_reference(terms, 60)
    assert cnt[2, 7] == 0 and cnt[2, 8] == 7                               # the short last chunk


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_inputs_poison_the_percentiles_and_nothing_else(dtype):
    """what the references say of a column that holds a NaN: NaN percentiles and no zone; counts and risk trace as if the
    NaN rows were not there"""
    clean, bad = support.nan_inputs(dtype)
    envs = sorted(NAN_CASES)
    others = np.setdiff1d(np.arange(bad.shape[1]), envs)
    assert clean[:, others].tobytes() == bad[:, others].tobytes()
    signs = np.signbit(bad[np.isnan(bad)])
    assert signs.any() and (~signs).any() and np.isnan(bad[:, 257]).all()
    assert np.isnan(bad[0, 5]) and np.isnan(bad[-1, 64]) and np.isnan(bad).sum() == 4 + bad.shape[0]
    for q in OUT_QS[0]:
        ref, bound = support.percentile_reference(bad, q, dtype)
        assert all(ref[i] is None for i in envs) and all(ref[i] is not None for i in others)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(np.isnan(np.percentile(bad.astype(np.float64), q, axis=0)), np.isin(np.arange(bad.shape[1]), envs))
    zone = O.report_cvga(bad.astype(np.float64))[3]
    assert (zone[envs] == 5).all() and np.array_equal(zone[others], O.report_cvga(clean.astype(np.float64))[3][others])
    cnt = support.outcome_counts(bad)
    terms = support.risk_terms(bad[:, envs])
    for j, env in enumerate(envs):
        keep = ~np.isnan(bad[:, env])
        assert np.array_equal(cnt[:, env], support.outcome_counts(bad[keep][:, env:env + 1])[:, 0])
        assert np.array_equal(np.vectorize(lambda v: v is None)(terms[:, j]), ~(keep & (bad[:, env] >= 1)))
    assert (cnt[:, 257] == 0).all() and (support.risk_reference(terms, 60)[0][:, envs.index(257)] == 0).all()
