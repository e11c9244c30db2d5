"""CPU suite of the controllers' collectors (t1d_collect_pid / t1d_collect_bb, BatchedT1DSimEnv.collect_pid / collect_bb): the
two symbols, every rejection that needs no device, the ctypes mirrors left as they were and the methods' signatures."""
import ctypes as C
import inspect
import os
import re

from support import CLOSED_LOOP, CLOSED_LOOP_EXACT, header_fields, mode_refusal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("t1d_collect_pid", "t1d_collect_bb")
N = 70                                      # not a multiple of 64: allowed here


def test_symbols_are_declared_bound_and_exported():
    from simglucose_amd import _lib
    src = open(os.path.join(ROOT, "include", "t1d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    abi = open(os.path.join(ROOT, "simglucose_amd", "csrc", "t1d_abi.hip")).read()
    L = _lib.lib()
    for name, ctl in zip(NAMES, ("t1d_pid", "t1d_bb")):
        assert re.search(r"\bint\s+%s\s*\(\s*t1d_ctx\s*\*[^;]*const\s+t1d_batch\s*\*[^;]*const\s+%s\s*\*[^;]*const\s+t1d_mlp\s*\*[^;]*"
                         r"const\s+t1d_collect\s*\*[^;]*int\s+n_steps\s*,\s*int\s+minutes\s*,\s*int\s+n_sub\s*,\s*void\s*\*\s*\w*\s*\)\s*;"
                         % (name, ctl), code), name
        assert name in _lib.EXPORTS
        assert re.search(r'extern "C" int %s\(' % name, abi)
        fn = getattr(L, name)                                   # AttributeError if the built library does not export it
        assert len(fn.argtypes) == 9 and fn.restype is C.c_int
    assert L.t1d_abi_version() == 4 and re.search(r"#define T1D_ABI_VERSION 4\b", src) and _lib.ABI_VERSION == 4


def test_lib_mirrors_are_untouched():
    """the ABI version stays 4 because no struct moved: every mirror the two calls take has the header's fields, in its
    order, at the sizes they had"""
    from simglucose_amd import _lib
    for name, mirror, size in (("t1d_pid", _lib.Pid, 4 * 8 + 11 * 8 + 8), ("t1d_bb", _lib.Bb, 8 + 13 * 8 + 8),
                               ("t1d_mlp", _lib.Mlp, 8 * 4 + 3 * 8 + 6 * 8 + 15 * 8 + 8), ("t1d_collect", _lib.Collect, 64),
                               ("t1d_restart", _lib.Restart, 4 * 4 + 9 * 8)):
        assert [f[0] for f in header_fields(name)] == [f[0] for f in mirror._fields_], name
        assert C.sizeof(mirror) == size, name


def _setup():
    """a call that passes every check that needs no device, with on_done = restart: the batch's state pointers stay NULL, so
    a call that gets past the checks under test ends at check_batch's 'a state pointer is NULL', before any HIP call"""
    from simglucose_amd import _lib
    buf = [(C.c_double * N)() for _ in range(12)]
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
        ctl, empty = (pid, _lib.Pid()) if name == "t1d_collect_pid" else (bb, _lib.Bb())

        def call(ctx=fake, batch=b, c=ctl, feat=f, col=g, n_steps=3, minutes=3, n_sub=4):
            rc = fn(ctx, C.byref(batch) if batch is not None else None, C.byref(c) if c is not None else None,
                    C.byref(feat) if feat is not None else None, C.byref(col) if col is not None else None, n_steps, minutes, n_sub, None)
            return rc, L.t1d_last_error()

        def refused(word, **kw):
            rc, msg = call(**kw)
            assert rc == -1 and msg.startswith(name.encode()) and word in msg, (name, word, rc, msg)

        # the valid call reaches the batch's own checks, and no further
        refused(b"state pointer")
        # what the roll-out entry point rejects
        refused(b"NULL" if name == "t1d_collect_pid" else b"must be set", c=None)
        refused(b"NULL" if name == "t1d_collect_pid" else b"must be set", c=empty)
        refused(b"ctx is NULL", ctx=None)
        refused(b"batch is NULL", batch=None)
        for n_steps in (0, -2):
            refused(b"n_steps", n_steps=n_steps)
        for minutes in (0, 100001):
            refused(b"minutes", minutes=minutes)
        for n_sub in (0, 4097):
            refused(b"n_sub", n_sub=n_sub)
        b.cho = ptr(buf[11]); refused(b"dense cho"); b.cho = None
        b.dtype = 7; refused(b"dtype"); b.dtype = _lib.T1D_F64
        b.n = 0; refused(b"batch.n"); b.n = N
        # the fields of t1d_mlp that are read
        refused(b"feat is NULL", feat=None)
        for h in (0, 13):
            f.history = h; refused(b"history")
        f.history = 4
        for k in ("cgm_hist", "ins_hist", "prev_meal"):
            keep = getattr(f, k)
            setattr(f, k, None); refused(b"cgm_hist / ins_hist / prev_meal"); setattr(f, k, keep)
        f.start_minute = ptr(buf[11]); refused(b"start_minute"); f.start_minute = None
        f.start_minute = r.start_minute; refused(b"state pointer"); f.start_minute = None        # the restart's own array is fine
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
        # what t1d_restart_done rejects, and the exact mode's array
        r.h_carry = ptr(buf[11]); refused(b"h_carry"); r.h_carry = None
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
    tail = ["policy_state", "stats", "trace", "on_done", "days", "terminal_obs", "episode_stats", "reset_outputs"]
    sig = inspect.signature(BatchedT1DSimEnv.collect_pid)
    assert list(sig.parameters)[1:] == ["n_steps", "P", "I", "D", "target", "features", "pid_state"] + tail
    sig_bb = inspect.signature(BatchedT1DSimEnv.collect_bb)
    assert list(sig_bb.parameters)[1:] == ["n_steps", "target", "features", "bb_state"] + tail
    mlp = inspect.signature(BatchedT1DSimEnv.collect_mlp)
    for s in (sig, sig_bb):
        d = {k: v.default for k, v in s.parameters.items()}
        assert d["target"] == 140.0 and d["on_done"] == "continue"
        for k in tail[1:]:
            assert d[k] == mlp.parameters[k].default, k


def test_every_closed_loop_method_turns_the_other_mode_away_first():
    """an exact-mode env is turned away by the six fixed-step methods, which name the exact-mode sibling or say that there is
    none, and a fixed-step env by the four exact-mode methods, which name theirs -- before anything else of the env is read"""
    for method in CLOSED_LOOP:
        msg = mode_refusal(method, "dopri5")
        if method in CLOSED_LOOP_EXACT:
            assert method + "_dopri5" in msg, method
        else:
            assert "collect_pid and collect_bb have no exact-mode form" in msg, method
    for method in CLOSED_LOOP_EXACT:
        msg = mode_refusal(method + "_dopri5", None)
        assert msg.startswith(method + "_dopri5 needs") and msg.endswith("(the fixed-step envs take %s)" % method), method
