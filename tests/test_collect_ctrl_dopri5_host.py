"""CPU suite of the controllers' collectors in the exact mode (t1d_collect_pid_dopri5 / t1d_collect_bb_dopri5,
BatchedT1DSimEnv.collect_pid_dopri5 / collect_bb_dopri5): the two symbols, every rejection that needs no device, the methods'
signatures and the texts with which each mode turns the other one's methods away."""
import ctypes as C
import inspect
import os
import re

from support import mode_refusal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("t1d_collect_pid_dopri5", "t1d_collect_bb_dopri5")
N = 70                                      # not a multiple of 64: allowed here


def test_symbols_are_declared_bound_and_exported():
    from simglucose_amd import _lib
    src = open(os.path.join(ROOT, "include", "t1d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    abi = open(os.path.join(ROOT, "simglucose_amd", "csrc", "t1d_abi.hip")).read()
    L = _lib.lib()
    for name, ctl in zip(NAMES, ("t1d_pid", "t1d_bb")):
        assert re.search(r"\bint\s+%s\s*\(\s*t1d_ctx\s*\*[^;]*const\s+t1d_batch\s*\*[^;]*const\s+%s\s*\*[^;]*const\s+t1d_mlp\s*\*[^;]*"
                         r"const\s+t1d_collect\s*\*[^;]*double\s*\*\s*h_carry\s*,\s*int32_t\s*\*\s*nfev\s*,\s*int\s+n_steps\s*,"
                         r"\s*int\s+minutes\s*,\s*void\s*\*\s*\w*\s*\)\s*;" % (name, ctl), code), name
        assert name in _lib.EXPORTS
        assert re.search(r'extern "C" int %s\(' % name, abi)
        fn = getattr(L, name)                                   # AttributeError if the built library does not export it
        assert len(fn.argtypes) == 10 and fn.restype is C.c_int
    assert L.t1d_abi_version() == 4 and re.search(r"#define T1D_ABI_VERSION 4\b", src) and _lib.ABI_VERSION == 4


def _setup():
    """a call that passes every check that needs no device, with on_done = restart: the batch's state pointers stay NULL, so
    a call that gets past the checks under test ends at the batch's own 'a state pointer is NULL', before any HIP call"""
    from simglucose_amd import _lib
    buf = [(C.c_double * N)() for _ in range(13)]
    ptr = lambda a: C.cast(a, C.c_void_p)
    b = _lib.Batch()
    b.n, b.dtype, b.n_meals = N, _lib.T1D_F64, 18
    b.meal_time, b.meal_amt, b.episode = ptr(buf[0]), ptr(buf[1]), ptr(buf[2])
    pid = _lib.Pid(); pid.integ, pid.prev = ptr(buf[3]), ptr(buf[4])
    bb = _lib.Bb(); bb.basal, bb.cr, bb.cf, bb.prev_meal = ptr(buf[5]), ptr(buf[6]), ptr(buf[7]), ptr(buf[8])
    f = _lib.Mlp()                                              # nothing of the network: widths, n_layers, params, n_policies all 0
    f.history = 4
    f.cgm_hist, f.ins_hist, f.prev_meal = ptr((C.c_double * (4 * N))()), ptr((C.c_double * (4 * N))()), ptr(buf[9])
    r = _lib.Restart()
    r.days, r.meal_time, r.meal_amt, r.start_minute = 2, b.meal_time, b.meal_amt, ptr(buf[10])
    g = _lib.Collect()
    g.on_done, g.restart = _lib.T1D_COLLECT_RESTART, C.pointer(r)
    return b, pid, bb, f, g, r, buf, ptr


def test_every_rejection_comes_before_a_device_is_touched():
    from simglucose_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(8)                                        # a ctx nothing may look into
    for name in NAMES:
        fn = getattr(L, name)
        b, pid, bb, f, g, r, buf, ptr = _setup()
        ctl, empty = (pid, _lib.Pid()) if name == "t1d_collect_pid_dopri5" else (bb, _lib.Bb())
        hc = ptr(buf[12])

        def call(ctx=fake, batch=b, c=ctl, feat=f, col=g, h_carry=hc, n_steps=3, minutes=3):
            rc = fn(ctx, C.byref(batch) if batch is not None else None, C.byref(c) if c is not None else None,
                    C.byref(feat) if feat is not None else None, C.byref(col) if col is not None else None, h_carry, None,
                    n_steps, minutes, None)
            return rc, L.t1d_last_error()

        def refused(word, **kw):
            rc, msg = call(**kw)
            assert rc == -1 and msg.startswith(name.encode() + b": ") and word in msg, (name, word, rc, msg)

        # the valid call reaches the batch's own checks, and no further
        refused(b"state pointer")
        # what the exact-mode roll-out entry point rejects
        refused(b"NULL", c=None)
        refused(b"NULL" if name == "t1d_collect_pid_dopri5" else b"not set", c=empty)
        refused(b"ctx is NULL", ctx=None)
        refused(b"batch is NULL", batch=None)
        refused(b"h_carry is NULL", h_carry=None)
        for n_steps in (0, -2):
            refused(b"n_steps", n_steps=n_steps)
        for minutes in (0, 100001):
            refused(b"minutes", minutes=minutes)
        b.cho = ptr(buf[11]); refused(b"dense cho"); b.cho = None
        b.dtype = _lib.T1D_F32; refused(b"fp64 batches only"); b.dtype = _lib.T1D_F64
        b.dtype = 7; refused(b"fp64 batches only"); b.dtype = _lib.T1D_F64
        b.n = 0; refused(b"batch.n"); b.n = N
        # the fields of t1d_mlp that are read
        refused(b"feat is NULL", feat=None)
        for h in (0, 13, -1):
            f.history = h; refused(b"history")
        f.history = 4
        for k in ("cgm_hist", "ins_hist", "prev_meal"):
            keep = getattr(f, k)
            setattr(f, k, None); refused(b"cgm_hist / ins_hist / prev_meal"); setattr(f, k, keep)
        f.start_minute = ptr(buf[11]); refused(b"start_minute"); f.start_minute = None
        f.start_minute = r.start_minute; refused(b"state pointer"); f.start_minute = None        # the restart's own array is fine
        for h in (1, 12):
            f.history = h; refused(b"state pointer")
        f.history = 4
        # ... and the ones that are not: a network's fields may hold anything
        f.n_layers, f.n_policies, f.envs_per_policy, f.n_params, f.out_act = 9, -1, 3, 5, 4
        refused(b"state pointer")
        f.n_layers = f.n_policies = f.envs_per_policy = f.n_params = f.out_act = 0
        # t1d_collect
        refused(b"collect is NULL", col=None)
        g.on_done = 2; refused(b"on_done"); g.on_done = _lib.T1D_COLLECT_RESTART
        g.reserved = 1; refused(b"reserved"); g.reserved = 0
        g.sigma = ptr(buf[11]); refused(b"sigma"); g.sigma = None
        g.eps_trace = ptr(buf[11]); refused(b"eps_trace"); g.eps_trace = None
        g.restart = None; refused(b"needs restart"); g.restart = C.pointer(r)
        # the exact mode's array in the restart: NULL or the call's own, nothing else
        r.h_carry = ptr(buf[11]); refused(b"restart.h_carry"); r.h_carry = None
        r.h_carry = hc; refused(b"state pointer"); r.h_carry = None
        # what t1d_restart_done rejects
        r.days = 0; refused(b"days"); r.days = 2
        r.reserved = 1; refused(b"reserved"); r.reserved = 0
        b.n_meals = 12; refused(b"n_meals"); b.n_meals = 18
        b.episode = None; refused(b"episode"); b.episode = ptr(buf[2])
        b.n_normals = 5; refused(b"host-normals"); b.n_normals = 0
        b.x0_override = ptr(buf[11]); refused(b"x0_override"); b.x0_override = None
        r.meal_amt = ptr(buf[11]); refused(b"tables the batch names"); r.meal_amt = b.meal_amt
        r.start_minute = None; refused(b"start_minute"); r.start_minute = ptr(buf[10])
        r.ep_return = ptr(buf[11]); refused(b"ep_return and ep_length"); r.ep_return = None
        r.last_return = ptr(buf[11]); refused(b"last_return"); r.last_return = None
        # without restarts the restart struct is not looked at
        g.on_done, g.restart = _lib.T1D_COLLECT_CONTINUE, None
        refused(b"state pointer")


def test_env_has_the_methods():
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    for fixed, exact in ((BatchedT1DSimEnv.collect_pid, BatchedT1DSimEnv.collect_pid_dopri5),
                         (BatchedT1DSimEnv.collect_bb, BatchedT1DSimEnv.collect_bb_dopri5)):
        a, b = inspect.signature(fixed), inspect.signature(exact)
        assert list(b.parameters) == list(a.parameters) + ["max_minutes_per_launch"]
        for k, v in a.parameters.items():
            assert b.parameters[k].default == v.default, k
        assert b.parameters["max_minutes_per_launch"].default == 240
    sig = inspect.signature(BatchedT1DSimEnv.collect_pid_dopri5)
    assert list(sig.parameters)[1:8] == ["n_steps", "P", "I", "D", "target", "features", "pid_state"]
    sig_bb = inspect.signature(BatchedT1DSimEnv.collect_bb_dopri5)
    assert list(sig_bb.parameters)[1:5] == ["n_steps", "target", "features", "bb_state"]
    assert sig.parameters["target"].default == 140.0 and sig.parameters["on_done"].default == "continue"


def test_the_committed_measurements_are_what_the_tool_computes():
    """profiles/collect/exact_ctrl_collect_bench.json: every median and ratio from its own runs, by benchlib.summarise and the
    tool's expressions; fp64 Dexcom, 32 steps, 5 runs, 64 Ki and 1 Mi envs, both workloads, every status 0"""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from benchlib import summarise
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    records = json.load(open(os.path.join(ROOT, "profiles", "collect", "exact_ctrl_collect_bench.json")))
    assert sorted((r["workload"], r["n_envs"]) for r in records) == [("hot", 1 << 16), ("hot", 1 << 20), ("stock", 1 << 16), ("stock", 1 << 20)]
    for rec in records:
        assert (rec["dtype"], rec["sensor"], rec["steps"], rec["integrator"]) == ("float64", "Dexcom", 32, "dopri5")
        med = {}
        for leg, v in rec["legs"].items():
            got = summarise(v["ms_runs"], "ms", spread=True)
            assert got == {k: v[k] for k in got} and len(v["ms_runs"]) == 5 and v["status"] == 0, leg
            med[leg] = v["ms_median"]
        assert rec["loop_over_collect"] == med["loop"] / med["collect"]
        assert rec["plain_over_rollout"] == med["plain"] / med["rollout"]
        assert rec["plain_minus_rollout_ms"] == med["plain"] - med["rollout"]


def test_each_mode_turns_the_other_ones_methods_away_first():
    for method in ("collect_pid", "collect_bb"):
        msg = mode_refusal(method + "_dopri5", None)
        assert msg.startswith(method + "_dopri5 needs") and msg.endswith("(the fixed-step envs take %s)" % method), method
        msg = mode_refusal(method, "dopri5")
        assert method + "_dopri5" in msg, method
        assert "collect_pid and collect_bb have no exact-mode form" in msg, method
