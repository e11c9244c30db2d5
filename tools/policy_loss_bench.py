"""One training epoch of actor and critic on a collected batch (zero_grad, both losses, backward, two Adam steps), fp64,
H = 4 (F = 11), one weight set each, two legs:
  fused    controller.ppo_clip_loss + controller.value_loss (t1d_mlp_loss): the network, the loss, its derivative and the
           weight gradient in one launch per net, one forward pass
  torch    the loop this replaces: controller.mlp_pre_output (t1d_mlp_grad, y only), the loss as a dozen torch elementwise
           kernels with autograd, and a second t1d_mlp_grad call per net that evaluates the network again
The legs alternate (fused, torch, fused, ...): after one warm-up pass of each, `reps` passes of each timed with device events,
the median reported; both legs start from the same weights, which move on with every pass.  Peak memory is what a leg
keeps after its warm-up pass (gradients, Adam state, its cached workspace if this shape is the first to ask for one of that
size) plus torch.cuda.max_memory_allocated over a timed pass above what was allocated when the pass began; the batch and the
other leg's allocations are excluded.  The two legs' actor and critic gradients of the first pass are compared (max |difference|
relative to the largest entry).  One JSON line per (widths, batch size); --out writes them as a list.

    python tools/policy_loss_bench.py --out profiles/policy/policy_loss_bench.json
"""
import argparse

import benchlib


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--history", type=int, default=4)
    ap.add_argument("--widths", nargs="+", default=["16,16,1", "32,32,32,1"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    benchlib.require_gpu("policy_loss_bench.py")
    import torch
    from simglucose_amd.controller import mlp_pre_output, ppo_clip_loss, value_loss
    from simglucose_amd.controller.mlp_ctrller import MLPController
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
            legs, grads = {}, {}
            for name in ("fused", "torch"):
                params, vparams = start.clone().requires_grad_(True), old.clone().requires_grad_(True)
                legs[name] = {"params": params, "vparams": vparams, "opt": torch.optim.Adam([params], lr=3e-4),
                              "vopt": torch.optim.Adam([vparams], lr=1e-3)}

            def fused(L):
                L["opt"].zero_grad(); L["vopt"].zero_grad()
                loss = ppo_clip_loss(L["params"], feat, pol, eps, y_old, adv, sig, clip=clip) + value_loss(L["vparams"], feat, pol, ret)
                loss.backward()
                L["opt"].step(); L["vopt"].step()

            z = y_old + sig * eps
            old_logp = MLPController.log_prob((z - y_old) / sig, sig)

            def torch_leg(L):
                L["opt"].zero_grad(); L["vopt"].zero_grad()
                y_new = mlp_pre_output(L["params"], feat, pol)
                ratio = (MLPController.log_prob((z - y_new) / sig, sig) - old_logp).exp()
                value = 0.5 * ((mlp_pre_output(L["vparams"], feat, pol) - ret) ** 2).mean()
                loss = -torch.minimum(ratio * adv, ratio.clamp(1 - clip, 1 + clip) * adv).mean() + value
                loss.backward()
                L["opt"].step(); L["vopt"].step()

            fns = {"fused": fused, "torch": torch_leg}
            kept = {}
            for name in fns:                                     # warm-up, and the gradients of the same first step
                kept[name] = benchlib.kept_bytes(lambda: fns[name](legs[name]))
                grads[name] = (legs[name]["params"].grad.clone(), legs[name]["vparams"].grad.clone())
            runs = benchlib.alternate(fns, args.reps, lambda name: benchlib.event_pass(lambda: fns[name](legs[name]))[1:])
            out = {k: {**benchlib.summarise([ms for ms, _ in rr], "ms"), "peak_bytes": kept[k] + max(peak for _, peak in rr),
                       "kept_bytes": kept[k]} for k, rr in runs.items()}
            rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
            res = {"widths": widths, "history": args.history, "n_envs": n, "rows": args.rows, "dtype": "float64",
                   "device": torch.cuda.get_device_name(0), "legs": out,
                   "torch_over_fused": out["torch"]["ms_median"] / out["fused"]["ms_median"],
                   "max_rel_grad_difference": {"actor": rel(grads["fused"][0], grads["torch"][0]),
                                               "critic": rel(grads["fused"][1], grads["torch"][1])}}
            benchlib.emit(results, res)
            feat = eps = adv = ret = y_old = z = old_logp = legs = grads = None
            torch.cuda.empty_cache()
    benchlib.write(results, args.out)


if __name__ == "__main__":
    main()
