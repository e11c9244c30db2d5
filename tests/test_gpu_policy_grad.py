"""GPU suite: t1d_mlp_grad / controller.mlp_pre_output -- the network on recorded features and its weight gradient.

Largest measured |grad - grad_reference| / S on an MI355X over the cases of test_gradient_against_the_reference (the
test prints it): fp64 2.76e-14 where the bound 8 (N + 200) u is 3.48e-13, fp32 2.29e-07 where it is 1.87e-04
(profiles/policy/README.md)."""
import ctypes as C

import pytest

from support import gpu_torch as _torch, identity_policy as _policy

pytestmark = pytest.mark.gpu


def _inputs(pol, K, n, dtype, seed):
    """random features in [-2, 2] and random coef on the device, rounded to dtype; the weights likewise"""
    torch = _torch()
    g = torch.Generator().manual_seed(seed)
    feat = (torch.rand(K, pol.n_features, n, generator=g, dtype=torch.float64) * 4 - 2).to(dtype).cuda().contiguous()
    coef = torch.randn(K, n, generator=g, dtype=torch.float64).to(dtype).cuda().contiguous()
    params = pol.flat_params().to(dtype).cuda().contiguous()
    return params, feat, coef


def _grad(pol, params, feat, coef, y=False, workspace=None):
    torch = _torch()
    from simglucose_amd.controller.mlp_grad import mlp_grad_call
    grad = torch.full_like(params, float("nan"))                       # overwritten, not accumulated
    yy = torch.empty(feat.shape[0], feat.shape[2], dtype=feat.dtype, device=feat.device) if y else None
    mlp_grad_call(pol, params, feat, coef=coef, y=yy, grad=grad, workspace=workspace)
    return (grad, yy) if y else grad


# ------------------------------------------------------------------------------------------------ 1: y is the collector's word
@pytest.mark.parametrize("history,widths,hidden,f64,exact", [
    (4, (8, 8, 1), "tanh", True, False), (4, (8, 8, 1), "tanh", False, False),
    (12, (32, 32, 32, 1), "relu", True, False), (12, (32, 32, 32, 1), "relu", False, False),
    (4, (8, 8, 1), "tanh", True, True)])
def test_y_is_the_collectors_word(history, widths, hidden, f64, exact):
    torch = _torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    from simglucose_amd.controller import mlp_pre_output
    dtype = torch.float64 if f64 else torch.float32
    n, P, K = 128, 2, 5
    pol = _policy(history, widths, P, hidden=hidden, seed=5, gain=0.3)
    env = BatchedT1DSimEnv(patient=["child#001", "adult#001"] * (n // 2), sensor="Dexcom", dtype=dtype, seed=3,
                           integrator="dopri5" if exact else None)
    env.reset()
    tr = env.new_trace(K, columns=("action", "features"), history=history)
    collect = env.collect_mlp_dopri5 if exact else env.collect_mlp
    collect(K, pol, sigma=None, on_done="continue", trace=tr)
    assert env.sync() == 0
    params = pol.device_params(env.device, dtype)
    y = mlp_pre_output(params, tr["features"][1:], pol)
    assert y.shape == (K, n) and bool(torch.isfinite(y).all())
    assert torch.equal(y, tr["action"][1:])
    assert float(y.std()) > 0                                          # not a constant that would match anything


# ------------------------------------------------------------------------------------------------ 2: the gradient
GRAD_CASES = [  # history, widths, n, K
    (4, (8, 8, 1), 128, 3), (4, (8, 8, 1), 256, 5),
    (12, (32, 32, 32, 1), 128, 3), (12, (32, 32, 32, 1), 256, 5),
    (4, (1,), 128, 3), (4, (1,), 256, 5),
    (2, (5, 1), 256, 1100),         # 4400 tiles in all, more than 2048: a wave takes three, across chunks and rows
]


@pytest.mark.parametrize("hidden,f64", [("tanh", True), ("relu", True), ("tanh", False)])
@pytest.mark.parametrize("history,widths,n,K", GRAD_CASES)
def test_gradient_against_the_reference(history, widths, n, K, hidden, f64):
    """|grad - grad_reference| <= 8 (N + 200) u S + 1e-300 per parameter, N samples per policy, S = sum |coef dy/dparam|,
    u = 2^-53 (fp64) or 2^-24 (fp32; the reference is fp64 on the fp32-rounded inputs).  N u S is the worst case of the
    recursive sums, about 200 u covers the per-term rounding through three layers of width 32, 8 is margin; a wrong index or
    a missing term is off by the order of S."""
    torch = _torch()
    P = 2
    dtype = torch.float64 if f64 else torch.float32
    pol = _policy(history, widths, P, hidden=hidden, seed=7)
    params, feat, coef = _inputs(pol, K, n, dtype, seed=11)
    ref, info = pol.grad_reference(feat, coef, params=params, info=True)
    if hidden == "relu" and len(widths) > 1:
        assert info["min_abs_pre"] > 1e-8, info["min_abs_pre"]        # no unit can sit on the other side of the kink
    grad = _grad(pol, params, feat, coef)
    assert grad.dtype == dtype and bool(torch.isfinite(grad).all())
    S = info["scale"]
    N = K * (n // P)
    u = 2.0 ** -53 if f64 else 2.0 ** -24
    err = (grad.double() - ref).abs()
    print("max error / S = %.3e (bound %.3e) %s %s" % (float((err / S.clamp_min(1e-300)).max()), 8 * (N + 200) * u, widths, dtype))
    assert bool((err <= 8 * (N + 200) * u * S + 1e-300).all())
    assert float(S.max()) > 0 and float(ref.abs().max()) > 0


def test_relu_seed_keeps_clear_of_the_kink_on_the_cpu():
    """the same margin as above, from the reference on the CPU: the seeds of the relu cases are chosen so that it holds"""
    torch = _torch()
    for history, widths, n, K in GRAD_CASES:
        if len(widths) == 1:
            continue
        pol = _policy(history, widths, 2, hidden="relu", seed=7)
        g = torch.Generator().manual_seed(11)
        feat = torch.rand(K, pol.n_features, n, generator=g, dtype=torch.float64) * 4 - 2
        coef = torch.randn(K, n, generator=g, dtype=torch.float64)
        assert pol.grad_reference(feat, coef, info=True)[1]["min_abs_pre"] > 1e-8


# ------------------------------------------------------------------------------------------------ 3: determinism, independence
def test_determinism_and_independence():
    torch = _torch()
    from simglucose_amd.controller import mlp_pre_output
    pol = _policy(4, (8, 8, 1), 2, hidden="tanh", seed=9)
    n, K = 256, 5
    params, feat, coef = _inputs(pol, K, n, torch.float64, seed=13)
    g1, y1 = _grad(pol, params, feat, coef, y=True)
    g2, y2 = _grad(pol, params, feat, coef, y=True)
    assert torch.equal(g1, g2) and torch.equal(y1, y2)
    # policy 1's samples do not show in policy 0's gradient
    feat2, coef2 = feat.clone(), coef.clone()
    feat2[:, :, n // 2:] = feat2[:, :, n // 2:] * 0.5 + 0.25
    coef2[:, n // 2:] = -3.0 * coef2[:, n // 2:]
    g3 = _grad(pol, params, feat2, coef2)
    assert torch.equal(g3[0], g1[0]) and not torch.equal(g3[1], g1[1])
    # y of a row does not depend on which rows go with it
    perm = torch.tensor([3, 0, 4, 1, 2], device=feat.device)
    yp = mlp_pre_output(params, feat[perm].contiguous(), pol)
    assert torch.equal(yp, y1[perm])
    assert torch.equal(mlp_pre_output(params, feat[2:3].contiguous(), pol), y1[2:3])


# ------------------------------------------------------------------------------------------------ 4: autograd plumbing
def test_autograd_plumbing():
    torch = _torch()
    from simglucose_amd.controller import mlp_pre_output
    from simglucose_amd.controller.mlp_ctrller import MLPController
    pol = _policy(4, (8, 8, 1), 2, hidden="tanh", seed=15)
    n, K = 128, 3
    old_params, feat, adv = _inputs(pol, K, n, torch.float64, seed=17)
    g = torch.Generator().manual_seed(19)
    eps = torch.randn(K, n, generator=g, dtype=torch.float64).cuda()
    sig = 0.3
    y_old = mlp_pre_output(old_params, feat, pol)
    assert not y_old.requires_grad
    z = y_old + sig * eps
    old = MLPController.log_prob((z - y_old) / sig, sig)

    def ppo(params):
        y_new = mlp_pre_output(params, feat, pol)
        ratio = (MLPController.log_prob((z - y_new) / sig, sig) - old).exp()
        return ratio, y_new, -torch.minimum(ratio * adv, ratio.clamp(0.8, 1.2) * adv).mean()

    same = old_params.clone().requires_grad_(True)
    ratio, _, _ = ppo(same)
    assert bool((ratio == 1.0).all())                                  # unchanged weights: exactly 1
    new_params = (old_params + 0.05 * torch.randn(old_params.shape, generator=g, dtype=torch.float64).cuda()).requires_grad_(True)
    ratio, y_new, loss = ppo(new_params)
    assert y_new.requires_grad and float((ratio.detach() - 1).abs().max()) > 1e-3
    got, = torch.autograd.grad(loss, new_params)
    # the same coefficient by hand: dloss / dy_new through a detached copy, then one t1d_mlp_grad call
    y_leaf = y_new.detach().clone().requires_grad_(True)
    r2 = (MLPController.log_prob((z - y_leaf) / sig, sig) - old).exp()
    loss2 = -torch.minimum(r2 * adv, r2.clamp(0.8, 1.2) * adv).mean()
    coef, = torch.autograd.grad(loss2, y_leaf)
    assert torch.equal(got, _grad(pol, new_params.detach(), feat, coef.contiguous()))
    assert float(got.abs().max()) > 0
    # the features get no gradient, bad input raises
    with pytest.raises(ValueError):
        mlp_pre_output(new_params, feat.transpose(0, 1).contiguous().transpose(0, 1), pol)
    with pytest.raises(ValueError):
        mlp_pre_output(new_params.float(), feat, pol)
    with pytest.raises(ValueError):
        mlp_pre_output(new_params.cpu(), feat, pol)
    # one SGD step lowers a quadratic loss on fixed features
    params = old_params.clone().requires_grad_(True)
    target = torch.randn(K, n, generator=g, dtype=torch.float64).cuda()
    opt = torch.optim.SGD([params], lr=0.05)
    before = ((mlp_pre_output(params, feat, pol) - target) ** 2).mean()
    opt.zero_grad(); before.backward(); opt.step()
    after = ((mlp_pre_output(params, feat, pol) - target) ** 2).mean()
    assert float(after.detach()) < float(before.detach())
    # the trained weights go back into the roll-outs' controller
    pol2 = MLPController.from_flat(params, pol.widths, history=pol.history, hidden=pol.hidden)
    assert torch.equal(pol2.device_params(feat.device, torch.float64), params.detach())


# ------------------------------------------------------------------------------------------------ 5: buffers
def test_buffers():
    torch = _torch()
    from simglucose_amd import _lib
    from simglucose_amd.controller.mlp_grad import mlp_grad_call, _struct
    pol = _policy(4, (8, 8, 1), 2, hidden="tanh", seed=21)
    n, K = 256, 5
    params, feat, coef = _inputs(pol, K, n, torch.float64, seed=23)
    both, y_both = _grad(pol, params, feat, coef, y=True)
    # y only
    y = torch.full((K, n), float("nan"), dtype=torch.float64, device=feat.device)
    mlp_grad_call(pol, params, feat, y=y)
    assert torch.equal(y, y_both)
    # grad only, into a buffer full of NaN
    assert torch.equal(_grad(pol, params, feat, coef), both)
    # a workspace of exactly the stated size in front of a sentinel tail
    need = _lib.lib().t1d_mlp_grad_workspace(C.byref(_struct(pol, params, n)), _lib.T1D_F64, n, K)
    assert need > 0 and need % 8 == 0
    buf = torch.full((need // 8 + 512,), -7.25, dtype=torch.float64, device=feat.device)
    grad = torch.full_like(params, float("nan"))
    io_ws = buf[:need // 8]
    mlp_grad_call(pol, params, feat, coef=coef, grad=grad, workspace=io_ws)
    torch.cuda.synchronize()
    assert torch.equal(grad, both)
    assert bool((buf[need // 8:] == -7.25).all())
    assert not bool((buf[:need // 8] == -7.25).any())                  # and all of it is used
