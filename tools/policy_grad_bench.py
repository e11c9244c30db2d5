"""Forward plus backward of the policy network on a collected batch, fp64, H = 4 (F = 11), one weight set, two legs:
  device    controller.mlp_pre_output (t1d_mlp_grad): y [K, n] from features [K, F, n], then the weight gradient of
            (coef * y).sum() -- the activations are recomputed in LDS, nothing is stored per sample
  autograd  what collect_mlp's docstring used to describe: an nn.Sequential on features.transpose(1, 2) under torch autograd,
            the transpose included
Every leg: one warm-up pass, then `reps` passes timed with device events, the median reported; peak memory is
torch.cuda.max_memory_allocated over a pass minus what was allocated before the leg's first pass (features and coef
excluded, the device leg's cached workspace included).  The two
gradients are compared (max |difference| relative to the largest entry).  One JSON line per (widths, batch size); --out
writes them as a list.

    python tools/policy_grad_bench.py --out profiles/policy/grad_bench.json
"""
import argparse

import benchlib


def sequential_of(pol, device):
    import torch
    from torch import nn
    mods = []
    for k, (W, b) in enumerate(zip(pol.W, pol.b)):
        lin = nn.Linear(W.shape[2], W.shape[1], dtype=torch.float64, device=device)
        with torch.no_grad():
            lin.weight.copy_(W[0]); lin.bias.copy_(b[0])
        mods.append(lin)
        if k + 1 < len(pol.W):
            mods.append(nn.Tanh())
    return nn.Sequential(*mods)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--history", type=int, default=4)
    ap.add_argument("--widths", nargs="+", default=["16,16,1", "32,32,32,1"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    benchlib.require_gpu("policy_grad_bench.py")
    import torch
    from simglucose_amd.controller import mlp_pre_output
    dev = torch.device("cuda:0")
    results = []
    for ws in args.widths:
        widths = [int(w) for w in ws.split(",")]
        pol = benchlib.random_policy(args.history, widths, hidden="tanh")
        for n in args.n:
            g = torch.Generator(device=dev).manual_seed(1)
            feat = torch.rand(args.rows, pol.n_features, n, generator=g, dtype=torch.float64, device=dev) * 4 - 2
            coef = torch.randn(args.rows, n, generator=g, dtype=torch.float64, device=dev)
            params = pol.flat_params().to(dev).requires_grad_(True)
            net = sequential_of(pol, dev)

            def device_leg():
                params.grad = None
                (mlp_pre_output(params, feat, pol) * coef).sum().backward()
                return params.grad

            def autograd_leg():
                net.zero_grad(set_to_none=True)
                (net(feat.transpose(1, 2)).squeeze(-1) * coef).sum().backward()
                return torch.cat([torch.cat([m.weight.grad.reshape(-1), m.bias.grad]) for m in net if hasattr(m, "weight")])

            gd, runs_d, peak_d = benchlib.event_timed(device_leg, args.reps)
            gd = gd.clone()
            ga, runs_a, peak_a = benchlib.event_timed(autograd_leg, args.reps)
            legs = {"device": {**benchlib.summarise(runs_d, "ms"), "peak_bytes": peak_d},
                    "autograd": {**benchlib.summarise(runs_a, "ms"), "peak_bytes": peak_a}}
            res = {"widths": widths, "history": args.history, "n_envs": n, "rows": args.rows, "dtype": "float64",
                   "device": torch.cuda.get_device_name(0), "legs": legs,
                   "autograd_over_device": legs["autograd"]["ms_median"] / legs["device"]["ms_median"],
                   "max_rel_grad_difference": float((gd.reshape(-1) - ga).abs().max() / ga.abs().max())}
            benchlib.emit(results, res)
            feat = coef = net = gd = ga = None
            torch.cuda.empty_cache()
    benchlib.write(results, args.out)


if __name__ == "__main__":
    main()
