"""CPU suite: the surface of the exact-mode trajectory collector (t1d_collect_mlp_dopri5) -- declared, bound, exported by the
built library, refusing a NULL context without a device, and reachable as BatchedT1DSimEnv.collect_mlp_dopri5."""
import ctypes as C
import os
import re

from support import mode_refusal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "t1d_collect_mlp_dopri5"


def test_symbol_is_declared_bound_and_exported():
    from simglucose_amd import _lib
    src = open(os.path.join(ROOT, "include", "t1d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, code)
    assert NAME in _lib.EXPORTS
    fn = getattr(L, NAME)                                       # AttributeError if the built library does not export it
    assert fn.argtypes is not None and len(fn.argtypes) == 9 and fn.restype is C.c_int
    assert L.t1d_abi_version() == 4                             # a function only: the structs did not move
    # the header no longer says that the exact mode has no collector, and points here from t1d_collect_mlp
    assert "the exact mode has no collector" not in src
    assert src.count(NAME) >= 3


def test_null_ctx_is_refused_without_a_device():
    from simglucose_amd import _lib
    L = _lib.lib()
    b, m, g = _lib.Batch(), _lib.Mlp(), _lib.Collect()
    assert L.t1d_collect_mlp_dopri5(None, C.byref(b), C.byref(m), C.byref(g), None, None, 1, 3, None) == -1
    assert L.t1d_last_error().startswith(b"t1d_collect_mlp_dopri5") and b"ctx is NULL" in L.t1d_last_error()


def test_env_has_the_method():
    import inspect
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    sig = inspect.signature(BatchedT1DSimEnv.collect_mlp_dopri5)
    assert list(sig.parameters)[1:] == ["n_steps", "policy", "sigma", "explore_seed", "policy_state", "stats", "trace", "on_done",
                                        "days", "terminal_obs", "episode_stats", "reset_outputs", "max_minutes_per_launch"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["sigma"] is None and d["explore_seed"] is None and d["policy_state"] is None and d["stats"] is None
    assert d["trace"] is None and d["on_done"] == "continue" and d["days"] == 2 and d["terminal_obs"] is None
    assert d["episode_stats"] is None and d["reset_outputs"] is False and d["max_minutes_per_launch"] == 240
    # collect_mlp keeps its signature, still refuses exact-mode envs, and now says where to go
    old = inspect.signature(BatchedT1DSimEnv.collect_mlp)
    assert list(old.parameters)[1:] == list(sig.parameters)[1:-1]
    assert "collect_mlp_dopri5" in mode_refusal("collect_mlp", "dopri5")
    assert "(the fixed-step envs take collect_mlp)" in mode_refusal("collect_mlp_dopri5", None)
