"""CPU suite of the per-env PID gains (t1d_rollout_pid_gains / t1d_rollout_pid_dopri5_gains, BatchedT1DSimEnv.pid_gains): the
header against the binding, the two signatures against their siblings', what pid_gains makes of its arguments, which entry
point rollout_pid / rollout_pid_dopri5 pick, the collectors' refusal, and every rejection of the library that needs no
device."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from support import header_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 70                                      # not a multiple of 64
NAMES = {"t1d_rollout_pid_gains": "t1d_rollout_pid", "t1d_rollout_pid_dopri5_gains": "t1d_rollout_pid_dopri5"}


def _header_code():
    src = open(os.path.join(ROOT, "include", "t1d.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_functions_are_the_exports():
    from simglucose_amd import _lib
    declared = re.findall(r"^\s*(?:const\s+char\s*\*|int64_t|int)\s+(t1d_\w+)\s*\(", _header_code(), re.M)
    assert len(declared) == len(set(declared))
    assert set(declared) == set(_lib.EXPORTS), set(declared) ^ set(_lib.EXPORTS)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS))
    for name in NAMES:
        assert name in declared
    src = open(os.path.join(ROOT, "include", "t1d.h")).read()
    assert re.search(r"#define T1D_ABI_VERSION 4\b", src) and _lib.ABI_VERSION == 4


def test_mirror_matches_the_header_and_t1d_pid_kept_its_layout():
    from simglucose_amd import _lib
    fields = header_fields("t1d_pid_gains")
    assert [f[0] for f in fields] == [f[0] for f in _lib.PidGains._fields_] == ["P", "I", "D", "target"]
    assert all(f[2] for f in fields)                            # four pointers
    assert all(t is C.c_void_p for _, t in _lib.PidGains._fields_) and C.sizeof(_lib.PidGains) == 32
    assert [f[0] for f in header_fields("t1d_pid")] == [f[0] for f in _lib.Pid._fields_]
    assert C.sizeof(_lib.Pid) == 4 * 8 + 11 * 8 + 8


def test_signatures_are_the_siblings_with_one_pointer_inserted():
    from simglucose_amd import _lib
    L = _lib.lib()
    code = _header_code()
    for name, sibling in NAMES.items():
        fn, sib = getattr(L, name), getattr(L, sibling)         # AttributeError if the built library does not export it
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == list(sib.argtypes[:3]) + [C.POINTER(_lib.PidGains)] + list(sib.argtypes[3:]), name
        args = lambda f: [re.sub(r"\s*\w+$", "", a.strip()) for a in
                          re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % f, code).group(1).split(",")]
        a, s = args(name), args(sibling)
        assert a == s[:3] + ["const t1d_pid_gains*"] + s[3:], (name, a, s)


def _bare(dtype_name="float32", n=5, integrator=None):
    """an env that has what pid_gains and the dispatch read, and nothing else: no context, no library, no device"""
    import torch
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    e = object.__new__(BatchedT1DSimEnv)
    e.n, e.dtype, e.device, e.integrator = n, getattr(torch, dtype_name), torch.device("cpu"), integrator
    return e


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
def test_pid_gains_broadcasts_and_rounds_once(dtype_name):
    import torch
    e = _bare(dtype_name)
    dt = e.dtype
    third = np.arange(1, 6) / 3.0                               # not representable in fp32
    own = torch.arange(5, dtype=dt) * 0.1
    g = e.pid_gains(1.0 / 3.0, third, torch.as_tensor(third, dtype=torch.float64) * 2, own)
    assert sorted(g) == ["D", "I", "P", "target"]
    for k in g:
        assert g[k].shape == (5,) and g[k].dtype == dt and g[k].is_contiguous() and g[k].device == e.device, k
    # a number: what (T)p->P gives; an array: float64 first, then one rounding
    assert torch.equal(g["P"], torch.full((5,), 1.0 / 3.0, dtype=torch.float64).to(dt))
    assert torch.equal(g["I"], torch.as_tensor(third, dtype=torch.float64).to(dt))
    assert torch.equal(g["D"], (torch.as_tensor(third, dtype=torch.float64) * 2).to(dt))
    assert g["target"] is own                                    # in place
    assert e.pid_gains(1, 2, 3)["target"].tolist() == [140.0] * 5
    # lists, integer arrays, the other dtype, a strided view: all formed anew
    other = torch.float32 if dt == torch.float64 else torch.float64
    g = e.pid_gains([1, 2, 3, 4, 5], np.arange(5), torch.ones(5, dtype=other), torch.arange(10, dtype=dt)[::2])
    assert g["P"].tolist() == [1, 2, 3, 4, 5] and g["I"].tolist() == [0, 1, 2, 3, 4] and g["D"].dtype == dt
    assert g["target"].tolist() == [0, 2, 4, 6, 8] and g["target"].is_contiguous()


def test_pid_gains_refuses_a_wrong_length_before_any_library_call():
    import torch
    e = _bare()                                                  # has no _L and no _ctx: touching either is an AttributeError
    for k, name in enumerate(("P", "I", "D", "target")):
        for bad in (torch.zeros(4), np.zeros(6), [1.0, 2.0], torch.zeros(5, 1), np.zeros((2, 5))):
            args = [0.0, 0.0, 0.0, 140.0]
            args[k] = bad
            with pytest.raises(ValueError) as err:
                e.pid_gains(*args)
            assert re.search(r"\b%s\b" % name, str(err.value)), (name, str(err.value))
            for method in ("rollout_pid", "rollout_pid_dopri5"):
                e.integrator = "dopri5" if method.endswith("dopri5") else None
                with pytest.raises(ValueError) as err:
                    getattr(e, method)(3, *args)
                assert re.search(r"\b%s\b" % name, str(err.value)), (method, name, str(err.value))
    e.integrator = None
    with pytest.raises(ValueError):
        e.rollout_pid(3, {"P": torch.zeros(5), "I": torch.zeros(5), "D": torch.zeros(5)})        # no target
    with pytest.raises(ValueError):
        e.rollout_pid(3, e.pid_gains(1, 2, 3), 2.0, 3.0)


def _recording(e):
    """stubs where the launch would be: -> the list of (entry point's name, the structs behind the batch)"""
    from simglucose_amd import _lib
    calls = []
    names = ("t1d_rollout_pid", "t1d_rollout_pid_gains", "t1d_rollout_pid_dopri5", "t1d_rollout_pid_dopri5_gains")
    e._L = types.SimpleNamespace(**{k: k for k in names})
    e._rollout = lambda fn, structs, n_steps, trace: calls.append((fn, structs))
    e._rollout_dopri5 = lambda fn, p, n_steps, trace, mm, extra=(): calls.append((fn, (p,) + tuple(x._obj for x in extra)))
    return calls, _lib


@pytest.mark.parametrize("exact", [False, True])
def test_scalars_take_the_old_entry_point_and_arrays_the_new(exact):
    import torch
    e = _bare("float64", integrator="dopri5" if exact else None)
    calls, _lib = _recording(e)
    method = e.rollout_pid_dopri5 if exact else e.rollout_pid
    old = "t1d_rollout_pid_dopri5" if exact else "t1d_rollout_pid"
    state = method(3, 1.5e-4, 4e-7, 5e-4, 120.0)
    assert sorted(state) == ["integ", "prev"]
    fn, structs = calls.pop()
    assert fn == old and len(structs) == 1 and isinstance(structs[0], _lib.Pid)
    assert (structs[0].P, structs[0].I, structs[0].D, structs[0].target) == (1.5e-4, 4e-7, 5e-4, 120.0)
    method(3, np.float64(1.0), np.float32(2.0), 3, target=np.int64(100))        # numpy numbers are numbers
    assert calls.pop()[0] == old
    P = torch.arange(5, dtype=torch.float64)
    for args, kw in (((P, 0.0, 0.0), {}), ((0.0, np.zeros(5), 0.0), {}), ((0.0, 0.0, [0.0] * 5), {}),
                     ((0.0, 0.0, 0.0), {"target": P}), ((e.pid_gains(P, 1.0, 2.0, 3.0),), {})):
        got = method(3, *args, pid_state=state, **kw)
        assert got is state
        fn, structs = calls.pop()
        assert fn == old + "_gains" and isinstance(structs[0], _lib.Pid) and isinstance(structs[1], _lib.PidGains)
        assert structs[0].integ == state["integ"].data_ptr() and structs[0].prev == state["prev"].data_ptr()
        assert all(getattr(structs[1], k) for k in ("P", "I", "D", "target"))
    assert structs[1].P == P.data_ptr()                          # the last call: the caller's tensor, in place
    assert not calls


@pytest.mark.parametrize("method", ["collect_pid", "collect_pid_limit", "collect_pid_dopri5", "collect_pid_dopri5_limit"])
def test_collectors_say_that_per_env_gains_are_a_rollout_feature(method):
    import torch
    from simglucose_amd import _lib
    e = _bare("float64", integrator="dopri5" if "dopri5" in method else None)
    extra = (7,) if method.endswith("_limit") else ()
    for args in ((torch.zeros(5), 0.0, 0.0), (0.0, np.zeros(5), 0.0), (0.0, 0.0, torch.zeros(150)), (e.pid_gains(1, 2, 3), None, None)):
        with pytest.raises(_lib.T1DError) as err:
            getattr(e, method)(3, *args, *extra)
        assert "per-env gains are a roll-out feature" in str(err.value) and "rollout_pid" in str(err.value)
        assert str(err.value).startswith(method + " ")


def test_library_refuses_null_gains_before_a_device_is_touched():
    from simglucose_amd import _lib
    L = _lib.lib()
    fake = C.c_void_p(8)                                        # a ctx nothing may look into
    buf = [(C.c_double * N)() for _ in range(9)]
    ptr = lambda a: C.cast(a, C.c_void_p)
    b = _lib.Batch()                                            # the state pointers stay NULL: a call that gets past the checks
    b.n, b.dtype, b.n_meals = N, _lib.T1D_F64, 4                # under test ends at the batch's own, before any HIP call
    b.meal_time, b.meal_amt = ptr(buf[0]), ptr(buf[1])
    pid = _lib.Pid(); pid.integ, pid.prev = ptr(buf[2]), ptr(buf[3])
    for name in NAMES:
        fn = getattr(L, name)
        g = _lib.PidGains(); g.P, g.I, g.D, g.target = (ptr(buf[4 + k]) for k in range(4))

        def call(gains=g, p=pid, ctx=fake):
            tail = (ptr(buf[8]), None, 3, 3, None) if "dopri5" in name else (3, 3, 4, None)
            rc = fn(ctx, C.byref(b), C.byref(p) if p is not None else None, C.byref(gains) if gains is not None else None, *tail)
            return rc, L.t1d_last_error()

        def refused(word, **kw):
            rc, msg = call(**kw)
            assert rc == -1 and msg.startswith(name.encode() + b":") and word in msg, (name, word, rc, msg)

        refused(b"state pointer")                               # the valid call reaches the batch's checks, and no further
        refused(b"gains is NULL", gains=None)
        for k in ("P", "I", "D", "target"):
            keep = getattr(g, k)
            setattr(g, k, None)
            refused(b"gains.%s is NULL" % k.encode())
            setattr(g, k, keep)
        refused(b"state pointer")
        # the sibling's own checks, under this call's name
        refused(b"pid state is NULL", p=None)
        refused(b"pid state is NULL", p=_lib.Pid())
        refused(b"ctx is NULL", ctx=None)
        # the four scalars of t1d_pid are not read: anything goes
        pid.P, pid.I, pid.D, pid.target = float("nan"), float("inf"), -1e300, float("nan")
        refused(b"state pointer")
        pid.P = pid.I = pid.D = pid.target = 0.0
