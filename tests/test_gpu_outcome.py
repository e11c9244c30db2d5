"""t1d_outcome_stats (outcome_kernel) at every threshold, rank, zone and shape, against references that share no code with it.

What a user quotes from a run -- time in range, the CVGA zones, LBGI and HBGI -- comes out of this one kernel.  Its inputs
and references are built in support.py and shown on the host (test_outcome_host.py) to reach every threshold with the float
on either side, both sides of every comparison of the zones, every kind of row the risk trace skips, and ties exactly at the
rank of a percentile.  Here the device is held to them, in fp64 and fp32:

  percentiles  the exact rational percentile under the rounding bound of support.percentile_reference;
  counts       equal to numpy's comparisons in the batch's own type;
  zones        equal to the oracle's report_cvga on min / max columns (two rows, q = 0 / 100: no interpolation);
  risk trace   NaN exactly where a 50-digit restatement has no usable row, and elsewhere within (cnt + C) u S of its f
               (fp64) and within what that allows for LBGI and HBGI (both types), C = RISK_C below;
  NaN          a column that holds one has NaN percentiles and no zone, and nothing else moves.

Every call goes through run(), the C ABI on buffers of its own: each output and the input are followed by a tail of
sentinel words that must come back intact, the input must come back unchanged, and an output word the kernel leaves
unwritten keeps the sentinel and so fails the comparison it is part of.  The wrapper (analysis/report.py) is held to run()
bit for bit.  The figures the cases print are recorded in profiles/outcome/README.md."""
import ctypes as C
import itertools

import numpy as np
import pytest

import support
from oracle import t1d_oracle as O
from support import NAN_CASES, OUT_KINDS, OUT_NS, OUT_QS, OUT_ROWS, RISK_CHUNKS, gpu_torch as _torch

pytestmark = pytest.mark.gpu

DTYPES = ("f64", "f32")
TAIL = 64                                  # sentinel words behind every buffer
SENTINEL = 0x5A
GROUPS = {"counts": ("counts",), "percentiles": ("pct", "zone"), "risk": ("risk",)}
ALL = ("counts", "pct", "zone", "risk")
# The largest C that |f - f_ref| <= (cnt + C) u S needed on an MI355X over every chunk length of RISK_CHUNKS was 0.21 (fp64,
# chunk = 1; profiles/outcome/README.md): the device's log and pow against correctly rounded ones, and the roundings of
# 10 f^2 that recovering f from the outputs brings in.  Four times that is asserted; support.RISK_C_LIMIT caps it at 64.
RISK_C = 0.84


def run(bg, q=OUT_QS[0], chunk=60, outputs=ALL):
    """One t1d_outcome_stats call on bg [rows, n] (numpy, float64 or float32) with the outputs named, every other output
    pointer NULL -> {"counts" int32 [5, n], "pct" [2, n], "zone" uint8 [n], "lbgi" / "hbgi" [n_chunks, n]} as numpy arrays.
    Asserts the sentinel tails behind the input and behind every output, and that the input is unchanged."""
    torch = _torch()
    from simglucose_amd import _lib
    L = _lib.lib()
    rows, n = bg.shape
    ft = bg.dtype
    word = {8: (torch.int64, np.int64), 4: (torch.int32, np.int32), 1: (torch.uint8, np.uint8)}
    nch = (rows + chunk - 1) // chunk
    shapes = {"counts": ((5, n), np.dtype(np.int32)), "pct": ((2, n), ft), "zone": ((n,), np.dtype(np.uint8)), "risk": ((nch, 2, n), ft)}

    def sentinels(count, size):
        fill = int.from_bytes(bytes([SENTINEL]) * size, "little")
        return torch.full((count,), fill, dtype=word[size][0], device="cuda:0")
    src = np.ascontiguousarray(bg).reshape(-1).view(word[ft.itemsize][1])
    inp = torch.cat([torch.from_numpy(src.copy()).to("cuda:0"), sentinels(TAIL, ft.itemsize)])
    o = _lib.Outcome()
    o.q_lo, o.q_hi, o.chunk = float(q[0]), float(q[1]), int(chunk)
    bufs = {}
    for name in outputs:
        shape, dt = shapes[name]
        bufs[name] = sentinels(int(np.prod(shape)) + TAIL, dt.itemsize)
        setattr(o, {"risk": "risk_trace"}.get(name, name), bufs[name].data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.t1d_outcome_stats(0, 0 if ft == np.float64 else 1, n, rows, C.c_void_p(inp.data_ptr()), C.byref(o), stream)
    assert rc == 0, L.t1d_last_error()
    torch.cuda.synchronize()
    back = inp.cpu().numpy()
    assert np.array_equal(back[:-TAIL], src), "the input changed"
    assert (back[-TAIL:].view(np.uint8) == SENTINEL).all(), "a write behind the input"
    out = {}
    for name, buf in bufs.items():
        shape, dt = shapes[name]
        raw = buf.cpu().numpy()
        assert (raw[-TAIL:].view(np.uint8) == SENTINEL).all(), "a write behind " + name
        out[name] = raw[:-TAIL].view(dt).reshape(shape)
    if "risk" in out:
        risk = out.pop("risk")
        out["lbgi"], out["hbgi"] = risk[:, 0], risk[:, 1]
    return out


def same_bits(a, b, keys=None):
    for k in (keys or a.keys()):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("n", OUT_NS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_percentiles_and_counts_of_every_shape(dtype, n):
    """every kind of column (support.outcome_columns), every row count and pair of percentiles: the percentiles within the
    bound of the exact ones, the counters equal to numpy's, the zone that of the kernel's own percentiles"""
    worst = np.zeros(2)
    for rows in OUT_ROWS:
        for qs in OUT_QS:
            bg = support.outcome_columns(n, rows, dtype, qs)
            r = run(bg, q=qs)
            assert np.array_equal(r["counts"], support.outcome_counts(bg)), (rows, qs)
            for k, q in enumerate(qs):
                ref, bound = support.percentile_reference(bg, q, dtype)
                err = support.percentile_error(r["pct"][k], ref, bound)
                worst = np.maximum(worst, support.worst_by_kind(err))
                assert err.max() <= 1.0, (rows, q, int(err.argmax()), OUT_KINDS[err.argmax() % len(OUT_KINDS)], err.max())
            assert np.array_equal(r["zone"], support.cvga_zone_codes(r["pct"][0], r["pct"][1])), (rows, qs)
    print("percentiles %s n=%d: worst error / bound %.3f, sign_mixed columns %.3f" % (dtype, n, worst[0], worst[1]))


@pytest.mark.parametrize("n", OUT_NS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_counts_at_the_thresholds(dtype, n):
    """50, 70, 180 and 250 themselves and the float on either side of each: exact integer equality"""
    for rows in OUT_ROWS:
        bg = support.outcome_threshold_inputs(n, rows, dtype)
        r = run(bg, outputs=("counts",))
        want = support.outcome_counts(bg)
        assert np.array_equal(r["counts"], want), (rows, np.argwhere(r["counts"] != want)[:4])


@pytest.mark.parametrize("dtype", DTYPES)
def test_zones_on_both_sides_of_every_bound(dtype):
    """support.zone_grid: with two rows and q = (0, 100) the percentiles are the column's min and max as they stand, so the
    zone codes equal the reference's in fp32 as in fp64, one ulp either side of every bound and beyond the clip bounds"""
    bg, mn, mx = support.zone_grid(dtype)
    want = O.report_cvga(bg.astype(np.float64), 0.0, 100.0)[3]
    r = run(bg, q=(0.0, 100.0))
    assert np.array_equal(r["pct"][0], mn) and np.array_equal(r["pct"][1], mx)
    wrong = np.flatnonzero(r["zone"] != want)
    assert not len(wrong), [(float(mn[i]), float(mx[i]), int(r["zone"][i]), int(want[i])) for i in wrong[:6]]
    print("zones %s: %d envs, codes %s" % (dtype, len(want), np.bincount(want, minlength=6).tolist()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrapper_zones_and_cvga_fractions(dtype):
    """the grid with every row twice: the 2.5th and 97.5th percentiles of [mn, mn, mx, mx] fall between equal order
    statistics, so CVGA_analysis with its own percentiles gives the oracle's fractions (B excludes A) and clipped bounds"""
    torch = _torch()
    from simglucose_amd.analysis import report
    bg, mn, mx = support.zone_grid(dtype)
    bg4 = np.concatenate([bg, bg])
    rmn, rmx, frac, zone = O.report_cvga(bg4.astype(np.float64))
    assert np.array_equal(rmn, np.clip(mn, 50, 400)) and np.array_equal(rmx, np.clip(mx, 50, 400))
    t = torch.as_tensor(bg4, device="cuda:0")
    out = report.CVGA_analysis(t)
    assert np.array_equal(out[0].cpu().numpy(), rmn.astype(bg.dtype)) and np.array_equal(out[1].cpu().numpy(), rmx.astype(bg.dtype))
    assert np.abs(np.array(out[2:]) - frac).max() < 1e-15
    s = report.outcome_stats(t, counts=False, risk_trace=False)
    assert np.array_equal(s["zone"].cpu().numpy(), zone)
    s2 = report.outcome_stats(torch.as_tensor(bg.copy(), device="cuda:0"), q_lo=0, q_hi=100)
    assert np.array_equal(s2["zone"].cpu().numpy(), zone)


@pytest.mark.parametrize("chunk", RISK_CHUNKS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_risk_trace_against_fifty_digits(dtype, chunk):
    """support.risk_inputs (rows skipped for BG <= 0, 0 < BG < 1; BG = 1; +Inf; chunks without a usable row; f of either
    sign and around 0) at a chunk of 1, 7, 60, the whole history and past its end.  Measured on an MI355X: the comparison
    needs C = 0.21 at the most (fp64, chunk = 1; 0.09 at 7, below 0 from 60 on), and with RISK_C = 0.84 LBGI / HBGI reach
    0.62 of their bound in fp64 and 0.99 in fp32, where the bound is the half ulp of the final cast."""
    assert RISK_C <= support.RISK_C_LIMIT
    bg = support.risk_inputs(dtype)
    ref = support.risk_reference_of(dtype, chunk)
    r = run(bg, chunk=chunk)
    assert r["lbgi"].shape == ref[0].shape
    res = support.risk_compare(r["lbgi"], r["hbgi"], ref, dtype, RISK_C)
    print("risk %s chunk=%d: C needed %s, LBGI / HBGI worst error / bound %.3f"
          % (dtype, chunk, "%.2f" % res["c_needed"] if dtype == "f64" else "-", res["worst"]))
    assert res["nan_equal"]
    assert res["worst"] <= 1.0
    if dtype == "f64":
        assert res["c_needed"] <= RISK_C


@pytest.mark.parametrize("dtype", DTYPES)
def test_null_outputs_and_repeat_calls_give_the_same_bits(dtype):
    """each non-empty subset of {counts, pct + zone, risk_trace}, and pct without zone and zone without pct, writes what the
    full call writes; a second full call too (run() checks the tails and the input every time)"""
    bg = support.outcome_columns(OUT_NS[-1], 41, dtype)
    full = run(bg, chunk=7)
    same_bits(full, run(bg, chunk=7))
    subsets = [sum((GROUPS[g] for g in c), ()) for k in (1, 2, 3) for c in itertools.combinations(GROUPS, k)]
    assert len(subsets) == 7
    for outputs in subsets + [("pct",), ("zone",)]:
        r = run(bg, chunk=7, outputs=outputs)
        assert set(r) == {k for o in outputs for k in (("lbgi", "hbgi") if o == "risk" else (o,))}
        same_bits(r, full)


@pytest.mark.parametrize("dtype", DTYPES)
def test_wrapper_gives_the_bits_of_the_abi(dtype):
    """analysis/report.py on a tensor against run() on the same values; percent = counts / rows * 100"""
    torch = _torch()
    from simglucose_amd.analysis import report
    rows, n = 41, OUT_NS[-1]
    bg = support.outcome_threshold_inputs(n, rows, dtype)
    t = torch.as_tensor(bg, device="cuda:0")
    full = run(bg, q=OUT_QS[3], chunk=7)
    s = report.outcome_stats(t, chunk=7, q_lo=OUT_QS[3][0], q_hi=OUT_QS[3][1])
    same_bits({k: s[k].cpu().numpy() for k in ("counts", "pct", "zone", "lbgi", "hbgi")}, full)
    want = support.outcome_counts(bg) / float(rows) * 100.0
    assert np.array_equal(s["percent"].cpu().numpy(), want) and np.array_equal(report.percent_stats(t).cpu().numpy(), want)
    for counts, percentiles, risk in itertools.product((False, True), repeat=3):
        if counts or percentiles or risk:
            part = report.outcome_stats(t, chunk=7, q_lo=OUT_QS[3][0], q_hi=OUT_QS[3][1], counts=counts, percentiles=percentiles,
                                        risk_trace=risk)
            keys = [k for k in ("counts", "pct", "zone", "lbgi", "hbgi") if k in part]
            assert len(keys) == counts + 2 * percentiles + 2 * risk
            same_bits({k: part[k].cpu().numpy() for k in keys}, full, keys)
    lb, hb, ri = report.risk_index_trace(t, chunk=60)
    d = run(bg, outputs=("risk",))
    assert lb.cpu().numpy().tobytes() == d["lbgi"].tobytes() and hb.cpu().numpy().tobytes() == d["hbgi"].tobytes()
    assert torch.equal(ri, lb + hb)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_poisons_its_envs_percentiles_and_nothing_else(dtype):
    """support.nan_inputs: a NaN of either sign in the first, the last or an inner row of an env, and an all-NaN column.
    np.percentile of such a column is NaN, and CVGA_analysis then finds no zone; the counters count a NaN in no range and the
    risk mean skips it; every other env reads as in the same call without the NaNs, bit for bit."""
    clean, bad = support.nan_inputs(dtype)
    envs = sorted(NAN_CASES)
    others = np.setdiff1d(np.arange(bad.shape[1]), envs)
    a, b = run(clean, chunk=7), run(bad, chunk=7)
    for k in a:
        assert a[k][..., others].tobytes() == b[k][..., others].tobytes(), k
    print("NaN %s: pct of the poisoned envs %s, zones %s" % (dtype, b["pct"][:, envs].tolist(), b["zone"][envs].tolist()))
    assert np.isnan(b["pct"][:, envs]).all()
    assert (b["zone"][envs] == 5).all()
    assert np.array_equal(b["counts"], support.outcome_counts(bad))
    ref = support.risk_reference(support.risk_terms(bad[:, envs]), 7)
    res = support.risk_compare(b["lbgi"][:, envs], b["hbgi"][:, envs], ref, dtype, RISK_C)
    print("NaN %s: risk trace of the poisoned envs, LBGI / HBGI worst error / bound %.3f" % (dtype, res["worst"]))
    assert res["nan_equal"] and res["worst"] <= 1.0, res
    assert np.isnan(b["lbgi"][:, 257]).all() and not np.isnan(b["lbgi"][:, 5]).any()
