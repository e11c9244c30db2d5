"""What the bench tools of this directory share: the GPU check, the two policies and the child / adult env of the collect
benches, the timed pass with its two clocks, alternation of legs, the median, and the JSON output.  Importing it puts the
repository root on sys.path, so a tool imports this module first and the package after it."""
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DAYS = 2


def require_gpu(tool):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("%s measures on the GPU: none found" % tool)


def random_policy(history, widths, **keywords):
    """randn / sqrt(n_in) weights and 0.1 * randn biases, layer by layer from seed 0; `keywords` go to MLPController"""
    import torch
    from simglucose_amd.controller.mlp_ctrller import MLPController
    g = torch.Generator().manual_seed(0)
    layers, n_in = [], 2 * history + 3
    for w in widths:
        layers.append((torch.randn(1, w, n_in, generator=g, dtype=torch.float64) / math.sqrt(n_in),
                       0.1 * torch.randn(1, w, generator=g, dtype=torch.float64)))
        n_in = w
    return MLPController(layers, history=history, **keywords)


def constant_policy(history, basal):
    """all-zero weights: `basal` U/min whatever the features"""
    import torch
    from simglucose_amd.controller.mlp_ctrller import MLPController
    return MLPController([(torch.zeros(1, 2 * history + 3, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))],
                         history=history, output="identity", out_scale=1.0, out_bias=basal)


def mixed_env(n, seed, integrator=None, options=()):
    """fp64 Dexcom, child#001 / adult#001 alternating with random initial glucose, every env restarted onto DAYS days of
    random meals; `options`: (name, value) pairs for set_option"""
    import torch
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    e = BatchedT1DSimEnv(patient=["child#001", "adult#001"] * (n // 2), sensor="Dexcom", dtype=torch.float64, seed=seed,
                         random_init_bg=True, integrator=integrator)
    for name, value in options:
        e.set_option(name, value)
    e.restart_done(mask=torch.ones(n, dtype=torch.uint8, device=e.device), days=DAYS, reset_outputs=True)
    return e


def timed_pass(fn, clock):
    """-> (fn's result, ms).  clock "host": time.perf_counter between two device synchronisations; "events": two events
    on the stream around fn.  A figure is comparable only with figures of the same clock."""
    import torch
    torch.cuda.synchronize()
    if clock == "host":
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)
    assert clock == "events", clock
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def timed_leg(warm, timed, clock):
    """the envelope of a leg: the warm-up pass, then timed_pass(timed, clock) -> ms"""
    warm()
    return timed_pass(timed, clock)[1]


def close_leg(e):
    """-> the env's status word, the env closed.  The caller then drops its reference (`del e`) and empties the cache: only
    it can."""
    status = e.sync(raise_on_status=False)
    e.close()
    return status


def event_pass(fn, base=None):
    """one pass between two events -> (fn's result, ms, peak bytes allocated during the pass above `base`; None: above
    what was allocated when the pass began)"""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    if base is None:
        base = torch.cuda.memory_allocated()
    out, ms = timed_pass(fn, "events")
    return out, ms, torch.cuda.max_memory_allocated() - base


def event_timed(fn, reps):
    """a warm-up pass, then `reps` passes between events -> (the last result, the ms of every pass, peak bytes above what
    was allocated before the warm-up pass: what fn caches in its first pass counts)"""
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    fn()
    ms, peak = [], 0
    for _ in range(reps):
        out, t, p = event_pass(fn, base)
        ms.append(t)
        peak = max(peak, p)
    return out, ms, peak


def kept_bytes(fn):
    """the warm-up pass of a leg that alternates with others -> bytes it leaves allocated"""
    import torch
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.memory_allocated() - base


def alternate(legs, reps, run_one):
    """reps x (every leg once, in order) -> {leg: [run_one(leg), ...]}"""
    runs = {leg: [] for leg in legs}
    for _ in range(reps):
        for leg in legs:
            runs[leg].append(run_one(leg))
    return runs


def median(values):
    """the upper median"""
    return sorted(values)[len(values) // 2]


def summarise(values, key, spread=False):
    """-> {key_median, [key_min, key_max,] key_runs}, in the order the records keep them"""
    out = {key + "_median": median(values)}
    if spread:
        out[key + "_min"], out[key + "_max"] = min(values), max(values)
    out[key + "_runs"] = list(values)
    return out


def emit(results, record):
    print(json.dumps(record), flush=True)
    results.append(record)


def write(results, out):
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
