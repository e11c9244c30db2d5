"""CPU suite: the host form of the in-kernel policy (controller/mlp_ctrller.py) and the ctypes mirror of t1d_mlp."""
import ctypes as C
import math

import pytest
import torch

from simglucose_amd.controller.mlp_ctrller import MLPController
from support import header_fields as _header_fields


def _net(history=3, widths=(8, 5, 1), act=torch.nn.Tanh, sigmoid=True, seed=0):
    torch.manual_seed(seed)
    mods, n_in = [], 2 * history + 3
    for k, w in enumerate(widths):
        mods.append(torch.nn.Linear(n_in, w))
        if k + 1 < len(widths):
            mods.append(act())
        n_in = w
    if sigmoid:
        mods.append(torch.nn.Sigmoid())
    return torch.nn.Sequential(*mods).double()


@pytest.mark.parametrize("act,sigmoid", [(torch.nn.Tanh, True), (torch.nn.ReLU, False)])
def test_forward_equals_sequential(act, sigmoid):
    net = _net(act=act, sigmoid=sigmoid)
    c = MLPController.from_torch(net, history=3, out_scale=0.05, out_bias=0.001)
    assert c.hidden == ("tanh" if act is torch.nn.Tanh else "relu") and c.output == ("logistic" if sigmoid else "identity")
    feat = torch.randn(9, 200, dtype=torch.float64)
    want = 0.05 * net(feat.T).reshape(-1) + 0.001
    for ordered in (False, True):
        assert (c.forward(feat, ordered=ordered) - want).abs().max() < 1e-12


def test_stack_of_weight_sets_uses_one_set_per_block_of_envs():
    nets = [_net(seed=s) for s in range(4)]
    singles = [MLPController.from_torch(nn_, history=3) for nn_ in nets]
    stack = MLPController([(torch.stack([s.W[k][0] for s in singles]), torch.stack([s.b[k][0] for s in singles])) for k in range(3)],
                          history=3, output="logistic")
    assert stack.n_policies == 4
    feat = torch.randn(9, 4 * 64, dtype=torch.float64)
    got = stack.forward(feat, ordered=True)
    for k, s in enumerate(singles):
        assert torch.equal(got[k * 64:(k + 1) * 64], s.forward(feat[:, k * 64:(k + 1) * 64], ordered=True))
    assert torch.equal(stack.flat_params(), torch.cat([s.flat_params() for s in singles]))


def test_feature_order_and_window_shift():
    H, n = 3, 5
    c = MLPController.from_torch(_net(history=H), history=H, cgm_mean=120.0, cgm_scale=0.5, ins_scale=3.0, cho_scale=0.25)
    cgm = torch.arange(H * n, dtype=torch.float64).reshape(H, n) + 100.0
    ins = torch.arange(H * n, dtype=torch.float64).reshape(H, n) * 0.01
    meal = torch.full((n,), 2.0, dtype=torch.float64)
    minute = torch.tensor([0, 360, 720, 1080, 1440 + 360])
    f = c.features(cgm, ins, meal, minute)
    assert f.shape == (2 * H + 3, n)
    assert torch.equal(f[:H], (cgm - 120.0) * 0.5)
    assert torch.equal(f[H:2 * H], ins * 3.0)
    assert torch.equal(f[2 * H], meal * 0.25)
    assert (f[2 * H + 1] - torch.tensor([0.0, 1.0, 0.0, -1.0, 1.0], dtype=torch.float64)).abs().max() < 1e-15
    assert (f[2 * H + 2] - torch.tensor([1.0, 0.0, -1.0, 0.0, 0.0], dtype=torch.float64)).abs().max() < 1e-15
    new_cgm, new_ins = torch.full((n,), 7.0, dtype=torch.float64), torch.full((n,), 0.5, dtype=torch.float64)
    c0, i0 = cgm.clone(), ins.clone()
    c.shift(cgm, ins, new_cgm, new_ins)
    assert torch.equal(cgm[0], new_cgm) and torch.equal(cgm[1:], c0[:-1])
    assert torch.equal(ins[0], new_ins) and torch.equal(ins[1:], i0[:-1])


def test_flat_params_round_trip_and_layout():
    c = MLPController.from_torch(_net(history=2, widths=(4, 1)), history=2)
    flat = c.flat_params()
    assert flat.shape == (1, MLPController.count_params(2, [4, 1])) == (1, 4 * 8 + 5)
    assert torch.equal(flat[0, :28], c.W[0][0].reshape(-1)) and torch.equal(flat[0, 28:32], c.b[0][0])
    assert torch.equal(flat[0, 32:36], c.W[1][0].reshape(-1)) and torch.equal(flat[0, 36:], c.b[1][0])
    back = MLPController.from_flat(flat, [4, 1], history=2)
    assert all(torch.equal(a, b) for a, b in zip(back.W + back.b, c.W + c.b))
    assert torch.equal(back.flat_params(), flat)


def test_policy_surface_for_one_env():
    from collections import namedtuple
    from datetime import datetime
    Obs = namedtuple("Obs", ["CGM"])
    H = 2
    c = MLPController.from_torch(_net(history=H, widths=(4, 1), sigmoid=False), history=H)
    a0 = c.policy(Obs(150.0), 0, False, sample_time=3, meal=0, time=datetime(2020, 1, 1, 6, 0))
    f0 = c.features(torch.full((H, 1), 150.0, dtype=torch.float64), torch.zeros(H, 1, dtype=torch.float64),
                    torch.zeros(1, dtype=torch.float64), torch.tensor([360]))
    assert a0.bolus == 0 and a0.basal == float(c.forward(f0, ordered=True)[0])
    a1 = c.policy(Obs(160.0), 0, False, sample_time=3, meal=1.5, insulin=0.02, time=datetime(2020, 1, 1, 6, 3))
    f1 = c.features(torch.tensor([[160.0], [150.0]], dtype=torch.float64), torch.tensor([[0.02], [0.0]], dtype=torch.float64),
                    torch.tensor([1.5], dtype=torch.float64), torch.tensor([363]))
    assert a1.basal == float(c.forward(f1, ordered=True)[0])
    c.reset()
    assert c.policy(Obs(150.0), 0, False, sample_time=3, meal=0, time=datetime(2020, 1, 1, 6, 0)).basal == a0.basal


def test_argument_checks_raise():
    lin = lambda i, o: (torch.zeros(o, i), torch.zeros(o))
    with pytest.raises(ValueError):
        MLPController([lin(11, 1)], history=0)
    with pytest.raises(ValueError):
        MLPController([lin(29, 1)], history=13)
    with pytest.raises(ValueError):
        MLPController([lin(11, 33), lin(33, 1)], history=4)              # too wide
    with pytest.raises(ValueError):
        MLPController([lin(11, 4)], history=4)                            # last width not 1
    with pytest.raises(ValueError):
        MLPController([lin(10, 1)], history=4)                            # wrong number of inputs
    with pytest.raises(ValueError):
        MLPController([lin(11, 4), lin(5, 1)], history=4)                 # layers do not chain
    with pytest.raises(ValueError):
        MLPController([lin(11, 2), lin(2, 2), lin(2, 2), lin(2, 2), lin(2, 1)], history=4)   # five layers
    with pytest.raises(ValueError):
        MLPController([lin(11, 1)], history=4, hidden="gelu")
    with pytest.raises(ValueError):
        MLPController([lin(11, 1)], history=4, output="softmax")
    with pytest.raises(ValueError):
        MLPController.from_flat(torch.zeros(5), [1], history=4)
    with pytest.raises(ValueError):
        MLPController.from_torch(torch.nn.Sequential(torch.nn.Linear(11, 1), torch.nn.GELU()), history=4)
    two = MLPController([(torch.zeros(2, 1, 11), torch.zeros(2, 1))], history=4)
    with pytest.raises(ValueError):
        two.forward(torch.zeros(11, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        two.policy(None, 0, False)


def test_mlp_struct_matches_header():
    from simglucose_amd import _lib
    fields = _header_fields("t1d_mlp")
    assert [f[0] for f in fields] == [f[0] for f in _lib.Mlp._fields_]
    size = {"int32_t": 4, "int64_t": 8, "double": 8}
    total = 0
    for (name, ctype, ptr, count), (_, ct) in zip(fields, _lib.Mlp._fields_):
        want = 8 if ptr else size[ctype] * count
        assert C.sizeof(ct) == want, name
        total += want
    assert C.sizeof(_lib.Mlp) == total == 8 * 4 + 3 * 8 + 6 * 8 + 15 * 8 + 8      # no padding: the 32-bit fields come in pairs
    assert "t1d_rollout_mlp" in _lib.EXPORTS
    assert (_lib.MLP_MAX_HISTORY, _lib.MLP_MAX_LAYERS, _lib.MLP_MAX_WIDTH) == (12, 4, 32)
    assert math.isclose(MLPController.count_params(12, [32, 32, 32, 1]), 27 * 32 + 32 + 2 * (32 * 32 + 32) + 33)
