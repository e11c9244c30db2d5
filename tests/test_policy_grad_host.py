"""CPU suite: t1d_mlp_grad without a GPU -- the exports, the struct mirror, the workspace size, every argument check
(validation comes before any HIP call), and the host restatements MLPController.pre_output / grad_reference."""
import ctypes as C

import pytest
import torch

from support import header_fields, mlp_struct as _mlp

U = 2.0 ** -53


def test_symbols_are_exported():
    from simglucose_amd import _lib
    L = _lib.lib()
    for name in ("t1d_mlp_grad_workspace", "t1d_mlp_grad"):
        assert name in _lib.EXPORTS and hasattr(L, name)


def test_mlp_batch_struct_layout_matches_header():
    from simglucose_amd import _lib
    fields = [f[0] for f in header_fields("t1d_mlp_batch")]
    assert fields == [f[0] for f in _lib.MlpBatch._fields_]
    assert C.sizeof(_lib.MlpBatch) == 8 * len(fields)


def test_workspace_size():
    from simglucose_amd import _lib
    L = _lib.lib()
    p = _mlp()
    # 2 policies x 1 chunk x 3 rows: one partial per tile
    assert L.t1d_mlp_grad_workspace(C.byref(p), _lib.T1D_F64, 128, 3) == 2 * 3 * p.n_params * 8
    assert L.t1d_mlp_grad_workspace(C.byref(p), _lib.T1D_F32, 128, 3) == 2 * 3 * p.n_params * 4
    p.params = None                                                   # the weights are not needed for the size
    assert L.t1d_mlp_grad_workspace(C.byref(p), _lib.T1D_F64, 128, 3) > 0
    # many tiles: about 2048 partials in all, whatever the number of rows
    big = L.t1d_mlp_grad_workspace(C.byref(p), _lib.T1D_F64, 128, 100000)
    assert 0 < big <= 2 * 1025 * p.n_params * 8
    bad = _mlp(widths=(33, 1))
    assert L.t1d_mlp_grad_workspace(C.byref(bad), _lib.T1D_F64, 128, 3) < 0
    assert L.t1d_mlp_grad_workspace(C.byref(p), _lib.T1D_F64, 128, 0) < 0
    assert L.t1d_mlp_grad_workspace(C.byref(p), 7, 128, 3) < 0


def test_every_invalid_argument_is_rejected_without_a_gpu():
    """-1 (T1D_E_INVALID) whether or not a device is present: nothing is launched, the device is not touched."""
    from simglucose_amd import _lib
    L = _lib.lib()
    F64 = _lib.T1D_F64

    def io(n_rows=3, feat=0x2000, coef=0x3000, y=0x4000, grad=0x5000, workspace=0x6000, workspace_bytes=1 << 30):
        b = _lib.MlpBatch()
        b.n_rows, b.feat, b.coef, b.y, b.grad = n_rows, feat, coef, y, grad
        b.workspace, b.workspace_bytes = workspace, workspace_bytes
        return b

    def call(p, b, n=128, dtype=F64):
        return L.t1d_mlp_grad(0, dtype, n, C.byref(p) if p is not None else None, C.byref(b) if b is not None else None, None)

    ok = _mlp()
    # what t1d_rollout_mlp rejects of the network's fields
    assert call(_mlp(history=0), io()) == -1 and b"history" in L.t1d_last_error()
    assert call(_mlp(history=13), io()) == -1
    assert call(_mlp(widths=(33, 1)), io()) == -1 and b"width" in L.t1d_last_error()
    assert call(_mlp(widths=(8, 2)), io()) == -1 and b"last layer" in L.t1d_last_error()
    p = _mlp(); p.n_layers = 5
    assert call(p, io()) == -1
    p = _mlp(); p.n_params += 1
    assert call(p, io()) == -1 and b"n_params" in L.t1d_last_error()
    p = _mlp(); p.hidden_act = 2
    assert call(p, io()) == -1 and b"hidden_act" in L.t1d_last_error()
    assert call(_mlp(params=None), io()) == -1 and b"params" in L.t1d_last_error()
    assert call(_mlp(n_policies=0), io()) == -1
    assert call(None, io()) == -1
    assert call(ok, None) == -1
    assert call(ok, io(), dtype=5) == -1
    # n and the split into policies
    assert call(ok, io(), n=192) == -1 and b"n_policies * envs_per_policy" in L.t1d_last_error()
    assert call(_mlp(envs_per_policy=96), io(), n=192) == -1 and b"multiple of 64" in L.t1d_last_error()
    # the batch
    assert call(ok, io(n_rows=0)) == -1 and b"n_rows" in L.t1d_last_error()
    assert call(ok, io(feat=None)) == -1 and b"feat" in L.t1d_last_error()
    assert call(ok, io(y=None, grad=None)) == -1 and b"both NULL" in L.t1d_last_error()
    assert call(ok, io(coef=None)) == -1 and b"coef" in L.t1d_last_error()
    assert call(ok, io(workspace=None)) == -1 and b"workspace" in L.t1d_last_error()
    need = L.t1d_mlp_grad_workspace(C.byref(ok), F64, 128, 3)
    assert call(ok, io(workspace_bytes=need - 1)) == -1 and b"workspace" in L.t1d_last_error()
    # the ignored fields may be anything: out_act, scales and state pointers are not looked at (a valid call would go on to
    # the device, so this is only checked through the workspace size)
    p = _mlp(); p.out_act = 9
    assert L.t1d_mlp_grad_workspace(C.byref(p), F64, 128, 3) == need


def _policy(widths, history, hidden, P, seed):
    from simglucose_amd.controller.mlp_ctrller import MLPController
    g = torch.Generator().manual_seed(seed)
    n_params = MLPController.count_params(history, widths)
    flat = (torch.rand(P, n_params, generator=g, dtype=torch.float64) - 0.5) * 1.2
    return MLPController.from_flat(flat, list(widths), history=history, hidden=hidden, output="logistic", out_scale=0.05,
                                   out_bias=0.01)


@pytest.mark.parametrize("ordered", [False, True])
def test_pre_output_then_output_function_is_forward(ordered):
    pol = _policy((8, 8, 1), 4, "tanh", 2, 1)
    feat = torch.rand(11, 128, generator=torch.Generator().manual_seed(2), dtype=torch.float64) * 4 - 2
    y = pol.pre_output(feat, ordered=ordered)
    assert y.shape == (128,)
    assert torch.equal(pol.out_scale * torch.sigmoid(y) + pol.out_bias, pol.forward(feat, ordered=ordered))
    ident = _policy((1,), 2, "relu", 1, 3)
    ident.output, ident.out_scale, ident.out_bias = "identity", 1.0, 0.0
    f2 = torch.rand(7, 64, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    assert torch.equal(ident.pre_output(f2, ordered=ordered), ident.forward(f2, ordered=ordered))


@pytest.mark.parametrize("hidden", ["tanh", "relu"])
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("widths", [(1,), (8, 1), (8, 5, 1), (32, 32, 32, 1)])
def test_grad_reference_is_autograd(widths, P, hidden):
    """grad_reference against torch autograd of (coef * pre_output(feat)).sum(), fp64 on the CPU.  Both add N terms of total
    size S per parameter in some order: |difference| <= 8 (N + 200) 2^-53 S (N u S the worst case of a recursive sum, 200 u
    the per-term rounding through three layers of width 32, 8 margin)."""
    K, n, H = 3, 64 * P, 4
    pol = _policy(widths, H, hidden, P, 10 + len(widths))
    g = torch.Generator().manual_seed(20 + P)
    feat = torch.rand(K, 2 * H + 3, n, generator=g, dtype=torch.float64) * 4 - 2
    coef = torch.randn(K, n, generator=g, dtype=torch.float64)
    grad, info = pol.grad_reference(feat, coef, info=True)
    S = info["scale"]
    assert grad.shape == S.shape == (P, pol.count_params(H, widths))
    if hidden == "relu" and len(widths) > 1:
        assert info["min_abs_pre"] > 1e-8                              # no unit on the kink
    for W, b in zip(pol.W, pol.b):
        W.requires_grad_(True); b.requires_grad_(True)
    loss = sum((coef[s] * pol.pre_output(feat[s])).sum() for s in range(K))
    loss.backward()
    want = torch.cat([torch.cat([W.grad.reshape(P, -1), b.grad], dim=1) for W, b in zip(pol.W, pol.b)], dim=1)
    N = K * (n // P)
    err = (grad - want).abs()
    bound = 8 * (N + 200) * U * S
    assert (err <= bound).all(), float((err / S.clamp_min(1e-300)).max())
    if hidden == "tanh":
        assert float(S.min()) > 0                                      # every parameter takes part (a relu unit may be dead)
    # params= overrides the controller's weights
    other = pol.flat_params().detach() * 0.5
    g2 = pol.grad_reference(feat, coef, params=other)
    pol2 = type(pol).from_flat(other, list(widths), history=H, hidden=hidden)
    assert torch.equal(g2, pol2.grad_reference(feat, coef))
