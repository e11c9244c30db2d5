"""CPU suite of the hybrid closed loop (the *_bolus entry points of include/t1d.h, MLPController(meal_bolus=)): exports and
the ctypes mirror of t1d_meal_bolus, the refusals that need no device, the host form of the policy against BBController, and
the refusal of the exact-mode collector."""
import ctypes as C
import os
import re
from collections import namedtuple

import pytest
import torch

import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t1d_rollout_mlp_bolus", "t1d_collect_mlp_bolus", "t1d_rollout_mlp_dopri5_bolus", "t1d_mlp_bolus")
Observation = namedtuple("Observation", ["CGM"])


def test_every_bolus_symbol_is_declared_and_exported():
    from simglucose_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "t1d.h")).read(), flags=re.S)
    abi = open(os.path.join(ROOT, "simglucose_amd", "csrc", "t1d_abi.hip")).read()
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint %s\(t1d_ctx\*[^;]*const t1d_meal_bolus\*[^;]*\);" % name, src), name
        assert re.search(r'extern "C" int %s\(' % name, abi), name
        assert hasattr(L, name), name
    assert re.search(r"#define T1D_ABI_VERSION 4\b", src) and _lib.ABI_VERSION == 4          # functions are only added


def test_meal_bolus_struct_layout_matches_header():
    from simglucose_amd import _lib
    fields = support.header_fields("t1d_meal_bolus")
    assert [f[0] for f in fields] == [f[0] for f in _lib.MealBolus._fields_] == ["target", "cr", "cf", "bolus_trace"]
    assert [f[2] for f in fields] == [False, True, True, True] and fields[0][1] == "double"
    assert C.sizeof(_lib.MealBolus) == 32 and _lib.MealBolus.bolus_trace.offset == 24


def _calls(L, mlp, g, mb):
    """the four entry points with a NULL ctx and a NULL batch, the meal-bolus struct `mb` (None: NULL)"""
    from simglucose_amd import _lib
    m = C.byref(mb) if mb is not None else C.POINTER(_lib.MealBolus)()
    return {"t1d_rollout_mlp_bolus": lambda: L.t1d_rollout_mlp_bolus(None, None, C.byref(mlp), m, 1, 3, 4, None),
            "t1d_collect_mlp_bolus": lambda: L.t1d_collect_mlp_bolus(None, None, C.byref(mlp), C.byref(g), m, 1, 3, 4, None),
            "t1d_rollout_mlp_dopri5_bolus": lambda: L.t1d_rollout_mlp_dopri5_bolus(None, None, C.byref(mlp), m, None, None, 1, 3, None),
            "t1d_mlp_bolus": lambda: L.t1d_mlp_bolus(None, None, C.byref(mlp), m, None, None)}


def test_bolus_entry_points_refuse_without_a_device():
    """a NULL ctx under the call's own name; a NULL meal_bolus, cr or cf is T1D_E_INVALID ahead of everything else"""
    from simglucose_amd import _lib
    L = _lib.lib()
    mlp, g = support.mlp_struct(), _lib.Collect()
    good = _lib.MealBolus(140.0, 0x1000, 0x2000, None)
    for name, call in _calls(L, mlp, g, good).items():
        assert call() == -1, name
        err = L.t1d_last_error().decode()
        assert err.startswith(name + ":") and "ctx is NULL" in err, (name, err)
    for label, mb in (("NULL", None), ("cr", _lib.MealBolus(140.0, None, 0x2000, None)), ("cf", _lib.MealBolus(140.0, 0x1000, None, None))):
        for name, call in _calls(L, mlp, g, mb).items():
            assert call() == -1, (name, label)                   # T1D_E_INVALID
            err = L.t1d_last_error().decode()
            assert err.startswith(name + ":") and "meal_bolus" in err and "ctx" not in err, (name, label, err)
            assert ("is NULL" in err) == (mb is None) and ("cr / cf" in err) == (mb is not None), (name, label, err)


# (patient, in Quest.csv?): one the table lists and one it does not (BBController's "Average" row)
PATIENTS = (("adult#003", True), ("nobody#000", False))
CASES = [(name, meal, cgm, st) for name, _ in PATIENTS for meal in (0.0, 15.0) for cgm in (120.0, 150.0, 150.5, 230.0) for st in (3, 5)]


def _zero_net(basal, **kw):
    F = 2 * 4 + 3
    from simglucose_amd.controller.mlp_ctrller import MLPController
    return MLPController([(torch.zeros(1, F, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))], history=4, output="identity",
                         out_scale=1.0, out_bias=basal, **kw)


def test_patient_table_of_the_cases():
    from simglucose_amd import params
    quest = params.quest_table()
    for name, listed in PATIENTS:
        assert (name in quest) == listed, name


@pytest.mark.parametrize("name,meal,cgm,st", CASES)
def test_hybrid_policy_is_bbcontroller_under_a_constant_basal_net(name, meal, cgm, st):
    """a zero-weight net whose out_bias is the patient's basal rate + meal_bolus=140: Action for Action what BBController
    returns from the same observation and info"""
    from simglucose_amd.controller.basal_bolus_ctrller import BBController
    bb = BBController(target=140)
    info = dict(patient_name=name, meal=meal, sample_time=st)
    want = bb.policy(Observation(CGM=cgm), 0.0, False, **info)
    pol = _zero_net(want.basal, meal_bolus=140)
    got = pol.policy(Observation(CGM=cgm), 0.0, False, **info)
    assert isinstance(pol.meal_bolus, BBController) and pol.meal_bolus.target == 140
    assert got == want, (got, want)
    assert (got.bolus > 0) == (meal > 0)
    if meal > 0:                       # the correction term is there above 150 mg/dL and nowhere else
        carbs = bb.policy(Observation(CGM=100.0), 0.0, False, **info).bolus
        assert (got.bolus > carbs) == (cgm > 150)
    # a BBController instance is taken as it is, its target included
    other = _zero_net(want.basal, meal_bolus=BBController(target=110))
    assert other.meal_bolus.target == 110
    assert other.policy(Observation(CGM=cgm), 0.0, False, **info) == BBController(target=110).policy(Observation(CGM=cgm), 0.0, False, **info)


def test_without_meal_bolus_the_policy_commands_no_bolus():
    from simglucose_amd.controller.mlp_ctrller import MLPController
    for pol in (_zero_net(0.02), _zero_net(0.02, meal_bolus=None)):
        assert pol.meal_bolus is None
        a = pol.policy(Observation(CGM=230.0), 0.0, False, patient_name="adult#003", meal=15.0, sample_time=3)
        assert a.basal == 0.02 and a.bolus == 0
    with pytest.raises(ValueError):
        _zero_net(0.02, meal_bolus="140")
    # the keyword reaches the two other constructors through their **kw
    flat = _zero_net(0.02).flat_params()
    assert MLPController.from_flat(flat, [1], history=4, meal_bolus=140.0).meal_bolus.target == 140.0
    net = torch.nn.Sequential(torch.nn.Linear(11, 4), torch.nn.Tanh(), torch.nn.Linear(4, 1))
    assert MLPController.from_torch(net, history=4, meal_bolus=120).meal_bolus.target == 120
    assert MLPController.from_torch(net, history=4).meal_bolus is None


def test_exact_mode_collector_refuses_a_bolus_policy_on_a_bare_env():
    """collect_mlp_dopri5 names what is missing before it reads anything of the env; its mode check still comes first"""
    from simglucose_amd import _lib
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    e = object.__new__(BatchedT1DSimEnv)
    e.integrator = "dopri5"
    with pytest.raises(_lib.T1DError) as err:
        e.collect_mlp_dopri5(1, _zero_net(0.02, meal_bolus=140.0))
    assert "collect_mlp_dopri5" in str(err.value) and "meal bolus" in str(err.value) and "t1d_collect_mlp_dopri5_bolus" in str(err.value)
    e.integrator = None
    with pytest.raises(_lib.T1DError) as err:
        e.collect_mlp_dopri5(1, _zero_net(0.02, meal_bolus=140.0))
    assert "integrator='dopri5'" in str(err.value)
    for method in ("rollout_mlp", "collect_mlp", "rollout_mlp_dopri5", "collect_mlp_dopri5"):       # policy=None, as the mode tests call them
        assert support.mode_refusal(method, "dopri5" if not method.endswith("_dopri5") else None)
