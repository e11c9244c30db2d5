"""The exact mode's closed-loop roll-outs (t1d_rollout_pid_dopri5 / t1d_rollout_bb_dopri5) without a GPU: the symbols, the
argument checks that need no device, the count model of tools/dopri5_bench.py and the kernel's registers."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np

from support import kernel_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("t1d_rollout_pid_dopri5", "t1d_rollout_bb_dopri5")


def test_symbols_are_declared_exported_and_loadable():
    from simglucose_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "t1d.h")).read(), flags=re.S)
    for name, ctl in zip(NAMES, ("t1d_pid", "t1d_bb")):
        assert re.search(r"int\s+%s\s*\(\s*t1d_ctx\s*\*\s*\w*\s*,\s*const\s+t1d_batch\s*\*\s*\w*\s*,\s*const\s+%s\s*\*\s*\w*\s*,"
                         r"\s*double\s*\*\s*h_carry\s*,\s*int32_t\s*\*\s*nfev\s*,\s*int\s+n_steps\s*,\s*int\s+minutes\s*,"
                         r"\s*void\s*\*\s*\w*\s*\)" % (name, ctl), src), name
        assert name in _lib.EXPORTS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().t1d_abi_version() == 4
    assert "T1D_ABI_VERSION 4" in src


def test_null_and_range_arguments_are_rejected_without_a_device():
    """NULL ctx, batch, controller or h_carry, a wrong dtype, n_steps or minutes out of range -> T1D_E_INVALID with a message;
    none of these paths looks at the ctx (a dummy pointer stands in)."""
    from simglucose_amd import _lib
    L = _lib.lib()
    b = _lib.Batch()
    b.n, b.dtype = 4, _lib.T1D_F64
    buf = [(C.c_double * 4)() for _ in range(6)]
    ptr = lambda a: C.cast(a, C.c_void_p)
    pid = _lib.Pid(); pid.integ, pid.prev = ptr(buf[0]), ptr(buf[1])
    bb = _lib.Bb(); bb.basal, bb.cr, bb.cf, bb.prev_meal = ptr(buf[2]), ptr(buf[3]), ptr(buf[4]), ptr(buf[5])
    hc = ptr((C.c_double * 4)())
    fake = C.c_void_p(8)
    for fn, ctl, empty in ((L.t1d_rollout_pid_dopri5, pid, _lib.Pid()), (L.t1d_rollout_bb_dopri5, bb, _lib.Bb())):
        assert fn(None, C.byref(b), C.byref(ctl), hc, None, 1, 3, None) == -1 and b"ctx" in L.t1d_last_error()
        assert fn(fake, None, C.byref(ctl), hc, None, 1, 3, None) == -1 and b"batch" in L.t1d_last_error()
        assert fn(fake, C.byref(b), None, hc, None, 1, 3, None) == -1 and b"NULL" in L.t1d_last_error()
        assert fn(fake, C.byref(b), C.byref(empty), hc, None, 1, 3, None) == -1          # controller arrays not set
        assert fn(fake, C.byref(b), C.byref(ctl), None, None, 1, 3, None) == -1 and b"h_carry" in L.t1d_last_error()
        b.dtype = _lib.T1D_F32
        assert fn(fake, C.byref(b), C.byref(ctl), hc, None, 1, 3, None) == -1 and b"fp64" in L.t1d_last_error()
        b.dtype = _lib.T1D_F64
        for n_steps in (0, -2):
            assert fn(fake, C.byref(b), C.byref(ctl), hc, None, n_steps, 3, None) == -1 and b"n_steps" in L.t1d_last_error()
        for minutes in (0, -3, 100001):
            assert fn(fake, C.byref(b), C.byref(ctl), hc, None, 1, minutes, None) == -1 and b"minutes" in L.t1d_last_error()


def _tool():
    spec = importlib.util.spec_from_file_location("dopri5_counts", os.path.join(ROOT, "tools", "dopri5_counts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wave_cost_model_on_a_hand_made_array():
    """4 minutes, 2 waves of 2 lanes.  Wave 0: lanes (7, 1, 1, 1) and (1, 7, 1, 1); wave 1: (2, 2, 2, 2) and (4, 4, 4, 4)."""
    wave_costs = _tool().wave_costs
    nf = np.array([[7, 1, 2, 4],
                   [1, 7, 2, 4],
                   [1, 1, 2, 4],
                   [1, 1, 2, 4]])
    r = wave_costs(nf, launch_minutes=4, wave=2)
    assert r["rhs_per_env_minute"] == (10 + 10 + 8 + 16) / 16.0 == 2.75
    # lock step: wave 0 pays 7 + 7 + 1 + 1 = 16 over 4 minutes, wave 1 pays 4 x 4 = 16 -> 4 per env-minute
    assert r["lockstep_wave_cost"] == 4.0
    # free running, one launch of 4 minutes: wave 0 pays max(10, 10) = 10, wave 1 max(8, 16) = 16 -> 13 / 4
    assert r["free_running_wave_cost"] == 3.25
    # launches of 2 minutes: wave 0 pays max(8, 8) + max(2, 2) = 10, wave 1 8 + 8 = 16
    assert wave_costs(nf, launch_minutes=2, wave=2)["free_running_wave_cost"] == 3.25
    # launches of 1 minute are the lock step
    assert wave_costs(nf, launch_minutes=1, wave=2)["free_running_wave_cost"] == 4.0
    # a last wave that is not full, and a last launch that is shorter: 3 lanes, launches of 3 minutes
    r = wave_costs(nf[:, :3], launch_minutes=3, wave=2)
    assert r["rhs_per_env_minute"] == 28 / 12.0
    assert r["lockstep_wave_cost"] == (16 + 8) / 2 / 4.0
    assert r["free_running_wave_cost"] == ((9 + 1) + (6 + 2)) / 2 / 4.0


def test_the_free_running_solver_loop_is_written_once():
    """Every closed-loop kernel of the exact mode includes one text for its loop (t1d_dopri5_loop.inc): over the device
    sources, dopri5_attempt( stands at its definition, in dopri5_minute and in that text; dopri5_enter( at its definition, in
    dopri5_minute and in that text.  Nine includes, one per kernel, and the text is a source of the library."""
    from simglucose_amd import _lib
    csrc = os.path.join(ROOT, "simglucose_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp", ".inc"))}
    loop = "t1d_dopri5_loop.inc"
    for call in ("dopri5_attempt(", "dopri5_enter("):
        counts = {f: t.count(call) for f, t in text.items() if call in t}
        assert counts == {"t1d_dopri5.hpp": 2, loop: 1}, (call, counts)
    assert text["t1d_dopri5.hpp"].count('#include "%s"' % loop) == 9
    assert os.path.join(csrc, loop) in _lib.SOURCES


def test_rollout_kernel_needs_no_scratch_and_the_step_kernel_still_none():
    """Both exact-mode kernels keep the stage vectors in the unified VGPR + AGPR file: the roll-out's per-minute words wait
    in LDS between the minute boundaries instead of being spilled inside the step-attempt loop."""
    ks = kernel_asm().kernels(kernel_asm().device_asm()).values()
    for prefix in ("_ZN3t1d21dopri5_rollout_kernel", "_ZN3t1d18dopri5_step_kernel"):
        mine = [k for k in ks if k.name.startswith(prefix)]
        assert len(mine) == 1, (prefix, mine)
        assert mine[0].figures["scratch_bytes_per_lane"] == 0, mine[0].figures
