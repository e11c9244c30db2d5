"""Advantages and value targets of a collected batch, K = 32 rows, about 1.5 % of the samples ending an episode, three legs:
  device          controller.gae (t1d_gae): one launch, adv and ret
  device+moments  the same with the per-policy sums of adv and adv^2 (one policy): one more small launch
  torch           the backwards loop over the rows in the call's dtype, r[s] + gamma * where(live, v[s + 1], 0) - v[s] + gamma
                  lam * where(live, adv[s + 1], 0): what a trainer writes by hand
Every leg: one warm-up pass, then `reps` passes timed with device events, the median reported.  bytes: what the scan has to
move -- reward, value and done read, adv and ret written, last_value read once -- and the rate the device leg reaches on
them.  The device's adv is compared with the torch loop's (max |difference| relative to the largest entry).  One JSON line
per (dtype, batch size); --out writes them as a list.

    python tools/gae_bench.py --out profiles/policy/gae_bench.json

--cut: two legs on the same arrays, alternated pass by pass after a warm-up pass of each, timed with device events:
  device          controller.gae (t1d_gae) as above
  device_cut      controller.gae with truncated= (--cut-rate of the samples, never where done is set) and cut_value=
                  (t1d_gae_limit): one more byte read per sample and one more word per env
and nothing else: the median, minimum and maximum of each and their ratio.

    python tools/gae_bench.py --cut --out profiles/policy/gae_limit_bench.json
"""
import argparse

import benchlib


def torch_loop(r, d, v, v_last, gamma, lam):
    import torch
    K = r.shape[0]
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    gl = gamma * lam
    zero = torch.zeros_like(v_last)
    vn, an = v_last, zero
    for s in range(K - 1, -1, -1):
        live = d[s] == 0
        an = r[s] + gamma * torch.where(live, vn, zero) - v[s] + gl * torch.where(live, an, zero)
        adv[s] = an
        ret[s] = an + v[s]
        vn = v[s]
    return adv, ret


def timed(fn, reps):
    out, ms, _ = benchlib.event_timed(fn, reps)
    return out, benchlib.median(ms), ms


def cut_record(gae, r, d, v, v_last, gamma, lam, cut_rate, reps, g):
    """the two legs of --cut on the arrays of one (dtype, batch size) -> the record's fields"""
    import torch
    K, n = r.shape
    t = ((torch.rand(K, n, generator=g, device=r.device) < cut_rate) & (d == 0)).to(torch.uint8)
    v_cut = 3.0 * torch.randn(n, generator=g, dtype=r.dtype, device=r.device)
    legs = {"device": lambda: gae(r, d, v, v_last, gamma=gamma, lam=lam),
            "device_cut": lambda: gae(r, d, v, v_last, gamma=gamma, lam=lam, truncated=t, cut_value=v_cut)}
    for fn in legs.values():
        fn()
    runs = benchlib.alternate(list(legs), reps, lambda leg: benchlib.event_pass(legs[leg])[1])
    word = r.element_size()
    rec = {"cut_rate": float(t.float().mean())}
    for leg, ms in runs.items():
        rec.update({leg + "_" + k: val for k, val in benchlib.summarise(ms, "ms", spread=True).items()})
    rec["cut_over_device"] = rec["device_cut_ms_median"] / rec["device_ms_median"]
    rec["algorithmic_bytes"] = K * n * (4 * word + 1) + n * word
    rec["algorithmic_bytes_cut"] = K * n * (4 * word + 2) + 2 * n * word
    rec["device_GBps"] = rec["algorithmic_bytes"] / rec["device_ms_median"] / 1e6
    rec["device_cut_GBps"] = rec["algorithmic_bytes_cut"] / rec["device_cut_ms_median"] / 1e6
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--done-rate", type=float, default=0.015)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cut", action="store_true", help="t1d_gae_limit against t1d_gae on the same arrays, and nothing else")
    ap.add_argument("--cut-rate", type=float, default=0.01, help="share of the samples that a time limit cut (--cut)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    benchlib.require_gpu("gae_bench.py")
    import torch
    from simglucose_amd.controller import gae
    dev = torch.device("cuda:0")
    K, gamma, lam = args.rows, 0.99, 0.95
    results = []
    for dtype_name in args.dtypes:
        dt = getattr(torch, dtype_name)
        for n in args.n:
            g = torch.Generator(device=dev).manual_seed(1)
            r = torch.randn(K, n, generator=g, dtype=dt, device=dev)
            v = 3.0 * torch.randn(K, n, generator=g, dtype=dt, device=dev)
            v_last = 3.0 * torch.randn(n, generator=g, dtype=dt, device=dev)
            d = (torch.rand(K, n, generator=g, device=dev) < args.done_rate).to(torch.uint8)
            if args.cut:
                rec = {"dtype": dtype_name, "n": n, "rows": K, "done_rate": float(d.float().mean())}
                rec.update(cut_record(gae, r, d, v, v_last, gamma, lam, args.cut_rate, args.reps, g))
                benchlib.emit(results, rec)
                del r, v, v_last, d
                continue
            (adv, ret), ms_dev, all_dev = timed(lambda: gae(r, d, v, v_last, gamma=gamma, lam=lam), args.reps)
            _, ms_mom, all_mom = timed(lambda: gae(r, d, v, v_last, gamma=gamma, lam=lam, moments=True), args.reps)
            (adv_t, ret_t), ms_torch, all_torch = timed(lambda: torch_loop(r, d, v, v_last, gamma, lam), args.reps)
            word = r.element_size()
            nbytes = K * n * (4 * word + 1) + n * word
            rec = {"dtype": dtype_name, "n": n, "rows": K, "done_rate": float(d.float().mean()),
                   "device_ms": ms_dev, "device_moments_ms": ms_mom, "torch_loop_ms": ms_torch,
                   "torch_over_device": ms_torch / ms_dev, "torch_over_device_moments": ms_torch / ms_mom,
                   "algorithmic_bytes": nbytes, "device_GBps": nbytes / ms_dev / 1e6, "device_moments_GBps": nbytes / ms_mom / 1e6,
                   "max_rel_diff_adv": float((adv - adv_t).abs().max() / adv_t.abs().max()),
                   "max_rel_diff_ret": float((ret - ret_t).abs().max() / ret_t.abs().max()),
                   "device_ms_all": all_dev, "device_moments_ms_all": all_mom, "torch_loop_ms_all": all_torch}
            benchlib.emit(results, rec)
            del r, v, v_last, d, adv, ret, adv_t, ret_t
    benchlib.write(results, args.out)


if __name__ == "__main__":
    main()
