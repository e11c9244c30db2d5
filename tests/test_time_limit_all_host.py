"""CPU suite: the time limit in the five collectors behind collect_mlp_limit -- t1d_collect_pid_limit, t1d_collect_bb_limit,
t1d_collect_mlp_dopri5_limit, t1d_collect_pid_dopri5_limit, t1d_collect_bb_dopri5_limit -- without a GPU: the exports and their
argtypes, the five signatures against their siblings', and what every method refuses before anything is launched."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import support
import support_ctrl
import support_limit
from support_limit import ENTRY_POINTS, METHODS, call_limit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_exported_with_argtypes():
    from simglucose_amd import _lib
    L = _lib.lib()
    tl = C.POINTER(_lib.TimeLimit)
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        fn, sib = getattr(L, name), getattr(L, name[:-len("_limit")])
        assert fn.restype is C.c_int and fn.argtypes is not None, name
        # the sibling's arguments with the limit behind the t1d_collect
        k = list(sib.argtypes).index(C.POINTER(_lib.Collect))
        assert list(fn.argtypes) == list(sib.argtypes[:k + 1]) + [tl] + list(sib.argtypes[k + 1:]), name
    assert L.t1d_abi_version() == 4 == _lib.ABI_VERSION


def test_header_declares_the_five_and_no_longer_says_no_time_limit():
    src = open(os.path.join(ROOT, "include", "t1d.h")).read()
    for name in ENTRY_POINTS:
        m = re.search(r"^int %s\((.*?)\);" % name, src, flags=re.S | re.M)
        assert m, name
        assert "const t1d_collect* collect, const t1d_time_limit* limit" in re.sub(r"\s+", " ", m.group(1)), name
    for doc in ("include/t1d.h", "README.md", "INTEGRATION.md", "simglucose_amd/batch_env.py"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, doc)).read())
        assert "have no time limit" not in text, doc


@pytest.mark.parametrize("method", list(METHODS))
def test_signature_is_the_siblings_with_the_limit_inserted(method):
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    sibling, head, behind, _ = METHODS[method]
    sig, old = inspect.signature(getattr(BatchedT1DSimEnv, method)), inspect.signature(getattr(BatchedT1DSimEnv, sibling))
    names, old_names = list(sig.parameters), list(old.parameters)
    k = 1 + len(head)
    assert names[1:k] == list(head) == old_names[1:k]
    assert names[k:k + 2] == ["max_episode_steps", "cut_features"]
    assert old_names[k] == behind and names[k + 2:] == old_names[k:]
    for name in old_names[k:]:                                   # the sibling's defaults, but for on_done
        want = "restart" if name == "on_done" else old.parameters[name].default
        assert sig.parameters[name].default == want, name
    assert sig.parameters["cut_features"].default is None
    assert sig.parameters["max_episode_steps"].default is inspect.Parameter.empty
    assert "max_episode_steps" not in old.parameters and "cut_features" not in old.parameters


def test_the_siblings_signatures_are_unchanged():
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    tail = ["on_done", "days", "terminal_obs", "episode_stats", "reset_outputs"]
    want = {"collect_pid": ["n_steps", "P", "I", "D", "target", "features", "pid_state", "policy_state", "stats", "trace"] + tail,
            "collect_bb": ["n_steps", "target", "features", "bb_state", "policy_state", "stats", "trace"] + tail,
            "collect_mlp_dopri5": ["n_steps", "policy", "sigma", "explore_seed", "policy_state", "stats", "trace"] + tail
            + ["max_minutes_per_launch"],
            "collect_mlp_limit": ["n_steps", "policy", "max_episode_steps", "cut_features", "sigma", "explore_seed", "policy_state",
                                  "stats", "trace"] + tail}
    want["collect_pid_dopri5"] = want["collect_pid"] + ["max_minutes_per_launch"]
    want["collect_bb_dopri5"] = want["collect_bb"] + ["max_minutes_per_launch"]
    for name, params in want.items():
        sig = inspect.signature(getattr(BatchedT1DSimEnv, name))
        assert list(sig.parameters)[1:] == params, name
        assert sig.parameters["on_done"].default == ("restart" if name == "collect_mlp_limit" else "continue"), name


def _bare_env(exact, n=128, dtype=torch.float64):
    """tests/test_time_limit_host.py's: a BatchedT1DSimEnv that has what a collector reads before its first launch, and nothing
    else: a call that gets past its argument checks ends in an AttributeError, not in a launch"""
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    e = object.__new__(BatchedT1DSimEnv)
    e.integrator, e.n, e.dtype, e.device, e.minutes_per_step = ("dopri5" if exact else None), n, dtype, torch.device("cpu"), 3
    return e


@pytest.mark.parametrize("method", list(METHODS))
def test_refusals_before_anything_is_launched(method):
    exact = METHODS[method][3]
    e = _bare_env(exact)
    pol = support.constant_policy(0.05) if "mlp" in method else support_ctrl.feature_policy()
    F = 2 * pol.history + 3
    with pytest.raises(ValueError, match=r"^%s: .*on_done='restart'" % method):
        call_limit(e, method, 4, 10, pol=pol, on_done="continue")
    with pytest.raises(ValueError, match=r"^%s: n_steps must not exceed" % method):
        call_limit(e, method, 11, 10, pol=pol)
    with pytest.raises(ValueError, match=r"^%s: .*at least 1" % method):
        call_limit(e, method, 1, 0, pol=pol)
    for bad in (torch.zeros(F, e.n + 1, dtype=torch.float64), torch.zeros(F + 1, e.n, dtype=torch.float64),
                torch.zeros(e.n, F, dtype=torch.float64), torch.zeros(F, e.n, dtype=torch.float32),
                torch.zeros(e.n, F, dtype=torch.float64).t(), [[0.0] * e.n] * F):
        with pytest.raises(ValueError, match=r"^%s: cut_features" % method):
            call_limit(e, method, 4, 10, bad, pol=pol)
    with pytest.raises(ValueError, match="truncated"):
        call_limit(e, method, 4, 10, pol=pol, trace={"row": 1, "truncated": torch.zeros(4, e.n, dtype=torch.uint8)})   # five rows needed
    # a good limit gets past the checks (and then misses what a real env has)
    with pytest.raises(AttributeError):
        call_limit(e, method, 10, 10, torch.zeros(F, e.n, dtype=torch.float64), pol=pol)
    # the other mode, in the words of the sibling's refusal
    msg, sib = support_limit.limit_mode_refusal(method), METHODS[method][0]
    if exact:
        assert msg.startswith(method + " needs") and msg.endswith("(the fixed-step envs take %s)" % method.replace("_dopri5", "")), msg
        assert msg.replace(method, sib).replace(method.replace("_dopri5", ""), sib.replace("_dopri5", "")) == support.mode_refusal(sib, None)
    else:
        assert msg == support.mode_refusal(sib, "dopri5") and "fixed-step" in msg and sib + "_dopri5" in msg


def test_collect_mlp_limit_keeps_its_messages():
    e, pol = _bare_env(False), support.constant_policy(0.05)
    with pytest.raises(ValueError, match=r"^collect_mlp_limit: max_episode_steps needs on_done='restart' \(a cut env starts its next episode\)$"):
        e.collect_mlp_limit(4, pol, 10, on_done="continue")
    with pytest.raises(ValueError, match=r"^collect_mlp_limit: n_steps must not exceed max_episode_steps \(an env is cut at most once per call\); "
                                         r"take the batch in several calls$"):
        e.collect_mlp_limit(11, pol, 10)
    with pytest.raises(ValueError, match=r"^collect_mlp_limit: max_episode_steps must be at least 1$"):
        e.collect_mlp_limit(1, pol, 0)
    with pytest.raises(ValueError, match=r"^collect_mlp_limit: cut_features must be a contiguous \[11, 128\] tensor of torch.float64 on the env's device$"):
        e.collect_mlp_limit(4, pol, 10, cut_features=torch.zeros(3, 3))


def test_the_exact_mlp_collector_refuses_a_bolus_and_a_relative_policy():
    from simglucose_amd import _lib
    e, pol = _bare_env(True), support.constant_policy(0.05)
    bolus = type(pol)(list(zip(pol.W, pol.b)), history=pol.history, output="identity", out_scale=1.0, out_bias=0.05, meal_bolus=140)
    rel = support.random_policy(widths=(8, 1), seed=6, output="identity", out_scale=1.0, out_bias=6.0, relative_to="basal")
    with pytest.raises(_lib.T1DError, match=r"^collect_mlp_dopri5_limit: the exact-mode collector has no meal bolus"):
        e.collect_mlp_dopri5_limit(4, bolus, 10)
    with pytest.raises(_lib.T1DError, match=r"^collect_mlp_dopri5_limit: the exact-mode collector has no patient-relative output"):
        e.collect_mlp_dopri5_limit(4, rel, 10)
    # collect_mlp_dopri5 as it was
    with pytest.raises(_lib.T1DError, match=r"^collect_mlp_dopri5: the exact-mode collector has no meal bolus"):
        e.collect_mlp_dopri5(4, bolus)
    with pytest.raises(_lib.T1DError, match=r"^collect_mlp_dopri5: the exact-mode collector has no patient-relative output"):
        e.collect_mlp_dopri5(4, rel)
