"""One training epoch of actor and critic on a collected batch, split into minibatches: per minibatch zero_grad, both fused
losses, backward and two Adam steps.  fp64, H = 4 (F = 11), one weight set each, 32 rows.  Per (widths, batch size, number
of minibatches B) the legs
  tiles    controller.ppo_clip_loss / value_loss with tiles=mb (t1d_mlp_loss_tiles): the batch is read in place
  gather   the loop this replaces: controller.gather_tiles of features, eps, y_old, adv and the value target for every
           minibatch, then the plain fused calls on the copies
  plain    B = 1 only: the plain fused calls without a list, the path a full-batch epoch took before lists existed
The minibatches of an epoch are drawn once by controller.tile_minibatches, outside the timed passes, and all legs walk the
same lists.  With B = 1 the list is a permutation of all tiles.  The legs alternate: after one warm-up epoch of each, `reps`
epochs of each timed with device events, the median reported; every leg starts from the same weights, which move on with
every epoch.  Peak memory is what a leg keeps after its warm-up epoch (gradients, Adam state, its cached workspaces where it
is the first to ask for one of that size) plus torch.cuda.max_memory_allocated over a timed epoch above what was allocated when
it began; the batch, the lists and the other legs' allocations are excluded.  `waves` is the number of waves a minibatch's loss
launch starts, P * ceil(M / T).  One JSON line per (widths, batch size, B); --out writes them as a list.

    python tools/policy_minibatch_bench.py --out profiles/policy/minibatch_bench.json
"""
import argparse

import benchlib


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--history", type=int, default=4)
    ap.add_argument("--widths", nargs="+", default=["16,16,1", "32,32,32,1"])
    ap.add_argument("--minibatches", type=int, nargs="+", default=[1, 4, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    benchlib.require_gpu("policy_minibatch_bench.py")
    import torch
    from simglucose_amd.controller import gather_tiles, mlp_pre_output, ppo_clip_loss, tile_minibatches, value_loss
    dev = torch.device("cuda:0")
    sig, clip = 0.3, 0.2
    results = []
    for ws in args.widths:
        widths = [int(w) for w in ws.split(",")]
        pol = benchlib.random_policy(args.history, widths, hidden="tanh")
        for n in args.n:
            g = torch.Generator(device=dev).manual_seed(1)
            feat = torch.rand(args.rows, pol.n_features, n, generator=g, dtype=torch.float64, device=dev) * 4 - 2
            eps = torch.randn(args.rows, n, generator=g, dtype=torch.float64, device=dev)
            adv = torch.randn(args.rows, n, generator=g, dtype=torch.float64, device=dev)
            ret = torch.randn(args.rows, n, generator=g, dtype=torch.float64, device=dev)
            old = pol.flat_params().to(dev)
            start = old + 0.02 * torch.randn(old.shape, generator=g, dtype=torch.float64, device=dev)   # ratios off 1: the clip acts
            y_old = mlp_pre_output(old, feat, pol)
            for B in args.minibatches:
                mbs = tile_minibatches(args.rows, n, 1, B, generator=torch.Generator(device=dev).manual_seed(2), device=dev)
                M = mbs[0].shape[1]
                names = ("tiles", "gather") + (("plain",) if B == 1 else ())
                legs = {}
                for name in names:
                    params, vparams = start.clone().requires_grad_(True), old.clone().requires_grad_(True)
                    legs[name] = {"params": params, "vparams": vparams, "opt": torch.optim.Adam([params], lr=3e-4),
                                  "vopt": torch.optim.Adam([vparams], lr=1e-3)}

                def step(L, loss):
                    L["opt"].zero_grad(); L["vopt"].zero_grad()
                    loss().backward()
                    L["opt"].step(); L["vopt"].step()

                def tiles_leg(L):
                    for mb in mbs:
                        step(L, lambda: ppo_clip_loss(L["params"], feat, pol, eps, y_old, adv, sig, clip=clip, tiles=mb) +
                             value_loss(L["vparams"], feat, pol, ret, tiles=mb))

                def gather_leg(L):
                    for mb in mbs:
                        f, e, y, a, r = (gather_tiles(t, mb, 1) for t in (feat, eps, y_old, adv, ret))
                        step(L, lambda: ppo_clip_loss(L["params"], f, pol, e, y, a, sig, clip=clip) + value_loss(L["vparams"], f, pol, r))

                def plain_leg(L):
                    step(L, lambda: ppo_clip_loss(L["params"], feat, pol, eps, y_old, adv, sig, clip=clip) + value_loss(L["vparams"], feat, pol, ret))

                fns = {"tiles": tiles_leg, "gather": gather_leg, "plain": plain_leg}
                kept = {name: benchlib.kept_bytes(lambda: fns[name](legs[name])) for name in names}        # warm-up
                runs = benchlib.alternate(names, args.reps, lambda name: benchlib.event_pass(lambda: fns[name](legs[name]))[1:])
                out = {k: {**benchlib.summarise([ms for ms, _ in rr], "ms"), "peak_bytes": kept[k] + max(peak for _, peak in rr),
                           "kept_bytes": kept[k]} for k, rr in runs.items()}
                med = {k: v["ms_median"] for k, v in out.items()}
                T = max(1, -(-M // 2048))
                res = {"widths": widths, "history": args.history, "n_envs": n, "rows": args.rows, "dtype": "float64",
                       "device": torch.cuda.get_device_name(0), "minibatches": B, "tiles_per_minibatch": M, "waves": -(-M // T),
                       "legs": out, "gather_over_tiles": med["gather"] / med["tiles"]}
                if B == 1:
                    res["tiles_over_plain"] = med["tiles"] / med["plain"]
                benchlib.emit(results, res)
                legs = mbs = None
                torch.cuda.empty_cache()
            feat = eps = adv = ret = y_old = None
            torch.cuda.empty_cache()
    benchlib.write(results, args.out)


if __name__ == "__main__":
    main()
