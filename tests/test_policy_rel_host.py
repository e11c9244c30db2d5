"""CPU suite of the patient-relative policy output (the *_rel entry points of include/t1d.h, MLPController(relative_to=)):
exports and the ctypes mirror of t1d_env_output, the refusals that need no device, the constructor, the host form of the policy
against BBController for every patient, and the refusal of the exact-mode collector."""
import ctypes as C
import os
import re
from collections import namedtuple

import pytest
import torch

import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t1d_rollout_mlp_rel", "t1d_collect_mlp_rel", "t1d_rollout_mlp_dopri5_rel", "t1d_mlp_action_rel")
Observation = namedtuple("Observation", ["CGM"])


def test_every_rel_symbol_is_declared_and_exported():
    from simglucose_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "t1d.h")).read(), flags=re.S)
    abi = open(os.path.join(ROOT, "simglucose_amd", "csrc", "t1d_abi.hip")).read()
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint %s\(t1d_ctx\*[^;]*const t1d_env_output\*[^;]*\);" % name, src), name
        assert re.search(r'extern "C" int %s\(' % name, abi), name
        assert hasattr(L, name), name
    assert re.search(r"#define T1D_ABI_VERSION 4\b", src) and _lib.ABI_VERSION == 4          # functions are only added


def test_env_output_struct_layout_matches_header():
    from simglucose_amd import _lib
    fields = support.header_fields("t1d_env_output")
    assert [f[0] for f in fields] == [f[0] for f in _lib.EnvOutput._fields_] == ["scale", "bias"]
    assert [f[2] for f in fields] == [True, True]
    assert C.sizeof(_lib.EnvOutput) == 16 and _lib.EnvOutput.bias.offset == 8


def _calls(L, mlp, g, eo, mb):
    """the four entry points with a NULL ctx and a NULL batch; `eo` / `mb`: the struct, None for NULL"""
    from simglucose_amd import _lib
    o = C.byref(eo) if eo is not None else C.POINTER(_lib.EnvOutput)()
    m = C.byref(mb) if mb is not None else C.POINTER(_lib.MealBolus)()
    return {"t1d_rollout_mlp_rel": lambda: L.t1d_rollout_mlp_rel(None, None, C.byref(mlp), o, m, 1, 3, 4, None),
            "t1d_collect_mlp_rel": lambda: L.t1d_collect_mlp_rel(None, None, C.byref(mlp), C.byref(g), o, m, 1, 3, 4, None),
            "t1d_rollout_mlp_dopri5_rel": lambda: L.t1d_rollout_mlp_dopri5_rel(None, None, C.byref(mlp), o, m, None, None, 1, 3, None),
            "t1d_mlp_action_rel": lambda: L.t1d_mlp_action_rel(None, None, C.byref(mlp), o, None, None)}


def test_rel_entry_points_refuse_without_a_device():
    """a NULL ctx under the call's own name, with and without a meal bolus; a NULL env_output, scale or bias is T1D_E_INVALID
    ahead of everything else, and so is a meal bolus without cr or cf in the three calls that take one"""
    from simglucose_amd import _lib
    L = _lib.lib()
    mlp, g = support.mlp_struct(), _lib.Collect()
    good, bolus = _lib.EnvOutput(0x1000, 0x2000), _lib.MealBolus(140.0, 0x3000, 0x4000, None)
    for mb in (None, bolus):
        for name, call in _calls(L, mlp, g, good, mb).items():
            assert call() == -1, name
            err = L.t1d_last_error().decode()
            assert err.startswith(name + ":") and "ctx is NULL" in err, (name, err)
    for label, eo in (("NULL", None), ("scale", _lib.EnvOutput(None, 0x2000)), ("bias", _lib.EnvOutput(0x1000, None))):
        for name, call in _calls(L, mlp, g, eo, bolus).items():
            assert call() == -1, (name, label)                   # T1D_E_INVALID
            err = L.t1d_last_error().decode()
            assert err.startswith(name + ":") and "env_output" in err and "ctx" not in err, (name, label, err)
            assert ("is NULL" in err) == (eo is None) and ("scale / bias" in err) == (eo is not None), (name, label, err)
    for label, mb in (("cr", _lib.MealBolus(140.0, None, 0x4000, None)), ("cf", _lib.MealBolus(140.0, 0x3000, None, None))):
        for name, call in _calls(L, mlp, g, good, mb).items():
            if name == "t1d_mlp_action_rel":                     # takes no meal bolus: t1d_mlp_bolus is the bolus half of a step loop
                continue
            assert call() == -1, (name, label)
            err = L.t1d_last_error().decode()
            assert err.startswith(name + ":") and "cr / cf" in err and "ctx" not in err, (name, label, err)


def test_wrong_policy_split_is_refused_before_anything_is_read():
    """192 envs under two weight sets: 96 envs each is no multiple of 64.  The three launches turn the relative policy away as
    they turn away a plain one, on a bare env that has its size and nothing else (the library's own check of the split,
    T1D_E_INVALID, needs a ctx: tests/test_gpu_policy_rel.py)"""
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    pol = support.random_policy(widths=(8, 1), n_policies=2, relative_to="basal", meal_bolus=140.0)
    for method, integrator in (("rollout_mlp", None), ("collect_mlp", None), ("rollout_mlp_dopri5", "dopri5")):
        e = object.__new__(BatchedT1DSimEnv)
        e.integrator, e.n = integrator, 192
        with pytest.raises(ValueError) as err:
            getattr(e, method)(1, pol, policy_state={})
        assert "do not split" in str(err.value) and method in str(err.value), method


def _zero_net(bias=1.0, **kw):
    F = 2 * 4 + 3
    from simglucose_amd.controller.mlp_ctrller import MLPController
    return MLPController([(torch.zeros(1, F, dtype=torch.float64), torch.full((1,), float(bias), dtype=torch.float64))], history=4,
                         output="identity", out_scale=1.0, out_bias=0.0, **kw)


def test_constructor_validation_and_pass_through():
    from simglucose_amd.controller.mlp_ctrller import MLPController
    assert _zero_net().relative_to is None and _zero_net(relative_to=None).relative_to is None
    assert _zero_net(relative_to="basal").relative_to == "basal"
    for bad in ("Basal", "tdi", 1, True, 0.5):
        with pytest.raises(ValueError):
            _zero_net(relative_to=bad)
    flat = _zero_net().flat_params()
    assert MLPController.from_flat(flat, [1], history=4, relative_to="basal").relative_to == "basal"
    assert MLPController.from_flat(flat, [1], history=4).relative_to is None
    net = torch.nn.Sequential(torch.nn.Linear(11, 4), torch.nn.Tanh(), torch.nn.Linear(4, 1))
    both = MLPController.from_torch(net, history=4, relative_to="basal", meal_bolus=120)
    assert both.relative_to == "basal" and both.meal_bolus.target == 120
    assert MLPController.from_torch(net, history=4).relative_to is None


def test_forward_multiplies_by_ref_when_given():
    pol = support.random_policy(widths=(8, 1), seed=2, out_scale=1.5, out_bias=0.25, relative_to="basal")
    feat = torch.randn(11, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    ref = torch.tensor([0.005, 0.01, 0.02, 0.03, 0.0, 1.0], dtype=torch.float64)
    for ordered in (False, True):
        plain = pol.forward(feat, ordered=ordered)
        assert torch.equal(pol.forward(feat, ordered=ordered, ref=ref), plain * ref)
        assert torch.equal(pol.forward(feat, ordered=ordered, ref=None), plain)


def _patients():
    from simglucose_amd import params
    return params.patient_table()[0]


# (CGM, announced meal g/min, sample time): no meal, a meal below and at the correction threshold, a meal above it
POINTS = ((120.0, 0.0, 3), (120.0, 15.0, 3), (150.0, 20.0, 5), (150.5, 20.0, 5), (230.0, 15.0, 3))


@pytest.mark.parametrize("name", _patients() + ["nobody#000"])
def test_one_relative_policy_is_bbcontroller_for_every_patient(name):
    """the zero network with last bias 1, relative_to="basal" and meal_bolus=140: Action for Action what BBController(140)
    returns for the patient -- one policy object for all 30 (and for the reference's 'Average' row)"""
    from simglucose_amd.controller.basal_bolus_ctrller import BBController
    bb = BBController(target=140)
    pol = _zero_net(relative_to="basal", meal_bolus=140)
    for cgm, meal, st in POINTS:
        info = dict(patient_name=name, meal=meal, sample_time=st)
        want = bb.policy(Observation(CGM=cgm), 0.0, False, **info)
        pol.reset()
        got = pol.policy(Observation(CGM=cgm), 0.0, False, **info)
        assert got == want, (name, cgm, meal, got, want)
        assert want.basal > 0 and (got.bolus > 0) == (meal > 0)
    # without meal_bolus the basal is still the patient's, and a multiple of it under another out_scale
    info = dict(patient_name=name, meal=15.0, sample_time=3)
    want = bb.policy(Observation(CGM=120.0), 0.0, False, **info)
    a = _zero_net(relative_to="basal").policy(Observation(CGM=120.0), 0.0, False, **info)
    assert a.basal == want.basal and a.bolus == 0
    assert _zero_net(bias=0.5, relative_to="basal").policy(Observation(CGM=120.0), 0.0, False, **info).basal == 0.5 * want.basal


def test_the_cohorts_basal_rates_span_a_factor_of_four():
    """what the feature is for: no single out_scale in U/min fits children and adults"""
    from simglucose_amd.controller.basal_bolus_ctrller import BBController
    bb = BBController()
    basal = [bb._bb_policy(n, 0.0, 100.0, 3).basal for n in _patients()]
    assert max(basal) / min(basal) > 4.0


def test_exact_mode_collector_refuses_a_relative_policy_on_a_bare_env():
    """collect_mlp_dopri5 names what is missing before it reads anything of the env; its mode check still comes first"""
    from simglucose_amd import _lib
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    e = object.__new__(BatchedT1DSimEnv)
    e.integrator = "dopri5"
    for kw in ({}, {"meal_bolus": 140.0}):
        with pytest.raises(_lib.T1DError) as err:
            e.collect_mlp_dopri5(1, _zero_net(relative_to="basal", **kw))
        assert "collect_mlp_dopri5" in str(err.value)
        if not kw:
            assert "relative_to" in str(err.value) and "t1d_collect_mlp_dopri5_rel" in str(err.value)
    e.integrator = None
    with pytest.raises(_lib.T1DError) as err:
        e.collect_mlp_dopri5(1, _zero_net(relative_to="basal"))
    assert "integrator='dopri5'" in str(err.value)
    for method in ("rollout_mlp", "collect_mlp", "rollout_mlp_dopri5", "collect_mlp_dopri5"):       # policy=None, as the mode tests call them
        assert support.mode_refusal(method, "dopri5" if not method.endswith("_dopri5") else None)
