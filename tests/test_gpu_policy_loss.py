"""GPU suite: t1d_mlp_loss / controller.ppo_clip_loss, value_loss -- the PPO-clip and value losses inside the gradient launch.

The inputs are tests/test_policy_loss_host.py's recipe (checked there, on the CPU, to be clear of the clip boundaries and to
run both branches of the select).  The bounds of test_against_the_reference for T1D_LOSS_PPO_CLIP are 4 x the largest error
measured on an MI355X over all its cases (the test prints the figures; profiles/policy/README.md has them); those of
T1D_LOSS_VALUE_MSE follow from the number formats and are derived in the test."""
import ctypes as C

import pytest

from support import gpu_torch as _torch
from test_policy_loss_host import CLIP, LOSS_CASES, recipe

pytestmark = pytest.mark.gpu

# 4 x the largest error measured on an MI355X over all cases of test_against_the_reference (True: fp64, False: fp32):
# per sample |coef - ref| relative to |scale adv r e_new / sigma|; |sum - ref| of the loss, dsig and KL sums relative to the
# sum of the terms' magnitudes.  Where each largest error sits: profiles/policy/README.md.
COEF_RTOL = {True: 4 * 4.53e-14, False: 4 * 1.20e-05}
LOSS_RTOL = {True: 4 * 2.32e-16, False: 4 * 4.85e-08}
DSIG_RTOL = {True: 4 * 2.14e-16, False: 4 * 1.14e-07}
KL_RTOL = {True: 4 * 1.97e-15, False: 4 * 3.47e-07}      # sum of expm1(logr) - logr, formed in double from the call's logr


def _dev(c):
    """the recipe's arrays on the device in the case's dtype (they were rounded to it on the CPU)"""
    return {k: (v.to(c["dtype"]).cuda().contiguous() if hasattr(v, "dtype") and k not in ("y", "y_old") else v) for k, v in c.items()}


def _call(d, kind, params, y_old=None, sigma=None, grad=True, y=True, coef=True, stats=True, workspace=None, scale=None):
    """one t1d_mlp_loss call -> dict of the outputs asked for, every buffer NaN before the call"""
    torch = _torch()
    from simglucose_amd import _lib
    from simglucose_amd.controller.policy_loss import mlp_loss_call
    feat = d["feat"]
    K, n = feat.shape[0], feat.shape[2]
    nan = lambda *shape, dt=feat.dtype: torch.full(shape, float("nan"), dtype=dt, device=feat.device)
    out = {"y": nan(K, n) if y else None, "coef": nan(K, n) if coef else None,
           "grad": torch.full_like(params, float("nan")) if grad else None, "stats": nan(d["P"], 4, dt=torch.float64) if stats else None}
    scale = 1.0 / (K * n) if scale is None else scale
    if kind == "ppo":
        mlp_loss_call(d["pol"], params, feat, _lib.T1D_LOSS_PPO_CLIP, scale, eps=d["eps"], y_old=y_old, adv=d["adv"],
                      sigma_old=d["sigma_old"], sigma=d["sigma"] if sigma is None else sigma, clip=CLIP, y=out["y"],
                      coef_out=out["coef"], grad=out["grad"], stats=out["stats"], workspace=workspace)
    else:
        mlp_loss_call(d["pol"], params, feat, _lib.T1D_LOSS_VALUE_MSE, scale, target=d["target"], y=out["y"], coef_out=out["coef"],
                      grad=out["grad"], stats=out["stats"], workspace=workspace)
    return out


def _y(d, params):
    torch = _torch()
    from simglucose_amd.controller.mlp_grad import mlp_grad_call
    y = torch.empty(d["feat"].shape[0], d["feat"].shape[2], dtype=d["feat"].dtype, device=d["feat"].device)
    mlp_grad_call(d["pol"], params, d["feat"], y=y)
    return y


def _grad(d, params, coef):
    torch = _torch()
    from simglucose_amd.controller.mlp_grad import mlp_grad_call
    grad = torch.full_like(params, float("nan"))
    mlp_grad_call(d["pol"], params, d["feat"], coef=coef, grad=grad)
    return grad


MODES = [("tanh", True), ("relu", True), ("tanh", False)]


# ------------------------------------------------------------------------------------------------ 6, 7: y and grad
@pytest.mark.parametrize("hidden,f64", MODES)
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("history,widths,n,K", LOSS_CASES)
def test_y_and_grad_are_those_of_mlp_grad_bit_for_bit(history, widths, n, K, P, hidden, f64):
    torch = _torch()
    d = _dev(recipe(history, widths, n, K, P, hidden, f64))
    y_old, y_new = _y(d, d["old"]), _y(d, d["new"])
    for kind in ("ppo", "mse"):
        o = _call(d, kind, d["new"], y_old=y_old)
        assert torch.equal(o["y"], y_new)
        assert bool(torch.isfinite(o["coef"]).all()) and float(o["coef"].abs().max()) > 0
        assert torch.equal(o["grad"], _grad(d, d["new"], o["coef"]))
        assert bool(torch.isfinite(o["grad"]).all()) and float(o["grad"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 8, 9: the reference
@pytest.mark.parametrize("hidden,f64", MODES)
@pytest.mark.parametrize("history,widths,n,K", LOSS_CASES)
def test_against_the_reference(history, widths, n, K, hidden, f64):
    """coef_out, the four sums and dsig against the fp64 closed form evaluated on the device's own y (for fp32 on the
    fp32-rounded inputs).  PPO: the bounds are the measured ones above, the not-active count is exact.  MSE: scale converted
    to the call's type, d = y - target and their product are three roundings: 4 u |coef|; a loss term is three roundings and the sum is in double:
    (8 u + N 2^-53) sum |loss_i|, u = 2^-53 or 2^-24.  A wrong branch or sign is an error of order 1."""
    torch = _torch()
    from simglucose_amd.controller import ppo_clip_loss_reference, value_loss_reference
    P = 2
    c = recipe(history, widths, n, K, P, hidden, f64)
    d = _dev(c)
    y_old = _y(d, d["old"])
    N = K * n // P
    u = 2.0 ** -53 if f64 else 2.0 ** -24
    tiny = torch.finfo(c["dtype"]).tiny
    o = _call(d, "ppo", d["new"], y_old=y_old)
    loss, coef, stats, dsig, info = ppo_clip_loss_reference(o["y"].double().cpu(), c["eps"], y_old.double().cpu(), c["adv"], c["sigma"],
                                                          c["sigma_old"], CLIP, P)
    got, st = o["coef"].double().cpu(), o["stats"].cpu()
    e_coef = float(((got - coef).abs() / info["coef_mag"]).max())
    e_loss = float(((st[:, 0] - stats[:, 0]).abs() / info["loss_mag"]).max())
    e_kl = float(((st[:, 2] - stats[:, 2]).abs() / stats[:, 2]).max())
    e_dsig = float(((st[:, 3] - stats[:, 3]).abs() / info["dsig_mag"]).max())
    print("ppo %s %s %s: coef %.3e loss %.3e kl %.3e dsig %.3e" % (widths, hidden, c["dtype"], e_coef, e_loss, e_kl, e_dsig))
    assert torch.equal(st[:, 1], stats[:, 1]) and float(stats[:, 1].min()) > 0          # the not-active count, exactly
    assert torch.equal(got != 0, info["active"])                                         # g is SELECTED: 0 where clipped
    assert bool(((got - coef).abs() <= COEF_RTOL[f64] * info["coef_mag"] + tiny).all())
    assert bool(((st[:, 0] - stats[:, 0]).abs() <= LOSS_RTOL[f64] * info["loss_mag"]).all())
    assert bool(((st[:, 2] - stats[:, 2]).abs() <= KL_RTOL[f64] * stats[:, 2]).all())
    assert bool(((st[:, 3] - stats[:, 3]).abs() <= DSIG_RTOL[f64] * info["dsig_mag"]).all())
    o = _call(d, "mse", d["new"])
    loss, coef, stats, _ = value_loss_reference(o["y"].double().cpu(), c["target"], P)
    got, st = o["coef"].double().cpu(), o["stats"].cpu()
    print("mse %s %s %s: coef %.3e loss %.3e" % (widths, hidden, c["dtype"], float(((got - coef).abs() / coef.abs().clamp_min(tiny)).max()),
                                                 float(((st[:, 0] - stats[:, 0]).abs() / stats[:, 0]).max())))
    assert bool(((got - coef).abs() <= 4 * u * coef.abs() + tiny).all())
    assert bool(((st[:, 0] - stats[:, 0]).abs() <= (8 * u + N * 2.0 ** -53) * stats[:, 0]).all())
    assert bool((st[:, 1:] == 0).all()) and float(stats[:, 0].min()) > 0


# ------------------------------------------------------------------------------------------------ 10: unchanged weights
@pytest.mark.parametrize("hidden,f64", MODES)
@pytest.mark.parametrize("history,widths,n,K", [LOSS_CASES[1], LOSS_CASES[3], LOSS_CASES[6]])
def test_unchanged_weights(history, widths, n, K, hidden, f64):
    torch = _torch()
    from simglucose_amd.controller import ppo_clip_loss
    P = 2
    c = recipe(history, widths, n, K, P, hidden, f64)
    d = _dev(c)
    y_old = _y(d, d["old"])
    o = _call(d, "ppo", d["old"], y_old=y_old, sigma=d["sigma_old"])
    assert torch.equal(o["y"], y_old)
    st = o["stats"].cpu()
    assert bool((st[:, 1] == 0).all()) and bool((st[:, 2] == 0.0).all())               # r is exactly 1 everywhere
    E = n // P
    so = c["sigma_old"].repeat_interleave(E)
    e_new = (so * c["eps"] + y_old.double().cpu() - y_old.double().cpu()) / so
    want = -(1.0 / (K * n)) * c["adv"] * e_new / so
    got = o["coef"].double().cpu()
    per = c["adv"].reshape(K, P, E)
    print("unchanged %s %s %s: coef %.3e loss %.3e" % (widths, hidden, c["dtype"], float(((got - want).abs() / want.abs()).max()),
                                                       float(((st[:, 0] + per.sum(dim=(0, 2))).abs() / per.abs().sum(dim=(0, 2))).max())))
    assert bool(((got - want).abs() <= COEF_RTOL[f64] * want.abs() + torch.finfo(c["dtype"]).tiny).all())
    assert bool(((st[:, 0] + per.sum(dim=(0, 2))).abs() <= LOSS_RTOL[f64] * per.abs().sum(dim=(0, 2))).all())
    params = d["old"].clone().requires_grad_(True)
    loss = ppo_clip_loss(params, d["feat"], d["pol"], d["eps"], y_old, d["adv"], d["sigma_old"], clip=CLIP)
    assert abs(float(loss.detach()) + float(c["adv"].mean())) <= LOSS_RTOL[f64] * float(c["adv"].abs().mean())


# ------------------------------------------------------------------------------------------------ 11: determinism, swap
@pytest.mark.parametrize("f64", [True, False])
def test_determinism_and_policy_swap(f64):
    torch = _torch()
    history, widths, n, K = LOSS_CASES[1]
    d = _dev(recipe(history, widths, n, K, 2, "tanh", f64))
    y_old = _y(d, d["old"])
    half = torch.cat([torch.arange(n // 2, n), torch.arange(0, n // 2)]).cuda()
    s = dict(d)
    for k in ("feat", "eps", "adv", "target"):
        s[k] = d[k][..., half].contiguous()
    for k in ("sigma", "sigma_old"):
        s[k] = d[k].flip(0).contiguous()
    for kind in ("ppo", "mse"):
        a, b = _call(d, kind, d["new"], y_old=y_old), _call(d, kind, d["new"], y_old=y_old)
        assert torch.equal(a["grad"], b["grad"]) and torch.equal(a["stats"], b["stats"]) and torch.equal(a["coef"], b["coef"])
        w = _call(s, kind, d["new"].flip(0).contiguous(), y_old=y_old[:, half].contiguous())
        assert torch.equal(w["grad"], a["grad"].flip(0)) and torch.equal(w["stats"], a["stats"].flip(0))
        assert not torch.equal(a["grad"][0], a["grad"][1]) and not torch.equal(a["stats"][0], a["stats"][1])


# ------------------------------------------------------------------------------------------------ 12: buffers
@pytest.mark.parametrize("kind", ["ppo", "mse"])
def test_buffers(kind):
    torch = _torch()
    from simglucose_amd import _lib
    from simglucose_amd.controller.mlp_grad import _struct
    history, widths, n, K = LOSS_CASES[1]
    d = _dev(recipe(history, widths, n, K, 2, "tanh", True))
    y_old = _y(d, d["old"])
    inputs = {k: d[k].clone() for k in ("feat", "eps", "adv", "target", "sigma", "sigma_old", "new")}
    inputs["y_old"] = y_old.clone()
    full = _call(d, kind, d["new"], y_old=y_old)
    # a workspace of exactly the stated size in front of a sentinel tail
    need = _lib.lib().t1d_mlp_loss_workspace(C.byref(_struct(d["pol"], d["new"], n)), _lib.T1D_F64, n, K)
    assert need > 0 and need % 8 == 0
    buf = torch.full((need // 8 + 512,), -7.25, dtype=torch.float64, device="cuda")
    o = _call(d, kind, d["new"], y_old=y_old, workspace=buf[:need // 8])
    torch.cuda.synchronize()
    assert all(torch.equal(o[k], full[k]) for k in full)
    assert bool((buf[need // 8:] == -7.25).all())
    assert not bool((buf[:need // 8] == -7.25).any())                  # and all of it is used
    # the inputs are unchanged
    assert all(torch.equal(inputs[k], d[k]) for k in inputs if k != "y_old") and torch.equal(inputs["y_old"], y_old)
    # no grad: the back-propagation is skipped, the rest is still written
    o = _call(d, kind, d["new"], y_old=y_old, grad=False)
    assert o["grad"] is None and all(torch.equal(o[k], full[k]) for k in ("y", "coef", "stats"))
    # any one output alone
    for only in ("y", "coef", "grad", "stats"):
        o = _call(d, kind, d["new"], y_old=y_old, **{k: k == only for k in ("y", "coef", "grad", "stats")})
        assert torch.equal(o[only], full[only]), only


# ------------------------------------------------------------------------------------------------ 13: autograd plumbing
def test_autograd_plumbing():
    torch = _torch()
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    from simglucose_amd.controller import ppo_clip_loss, value_loss
    from simglucose_amd.controller.mlp_ctrller import MLPController
    history, widths, n, K = LOSS_CASES[0]
    P = 2
    d = _dev(recipe(history, widths, n, K, P, "tanh", True))
    y_old = _y(d, d["old"])
    want = _call(d, "ppo", d["new"], y_old=y_old)
    params = d["new"].clone().requires_grad_(True)
    sigma = d["sigma"].clone().requires_grad_(True)
    loss, st = ppo_clip_loss(params, d["feat"], d["pol"], d["eps"], y_old, d["adv"], sigma, sigma_old=d["sigma_old"], clip=CLIP,
                             return_stats=True)
    assert loss.dim() == 0 and loss.requires_grad and float(loss.detach()) == float(want["stats"][:, 0].sum() / (K * n))
    N = K * n // P
    assert torch.equal(st["loss"], want["stats"][:, 0] / N) and torch.equal(st["clip_frac"], want["stats"][:, 1] / N)
    assert torch.equal(st["approx_kl"], want["stats"][:, 2] / N) and not st["loss"].requires_grad
    opt = torch.optim.Adam([params, sigma], lr=1e-2)
    opt.zero_grad(); loss.backward()
    assert torch.equal(params.grad, want["grad"])
    assert torch.equal(sigma.grad, (1.0 / (K * n)) * want["stats"][:, 3]) and float(sigma.grad.abs().min()) > 0
    opt.step()
    assert not torch.equal(params.detach(), d["new"]) and not torch.equal(sigma.detach(), d["sigma"])
    # a float sigma gets no grad and is every policy's; grad_output scales the stored gradient
    p2 = d["new"].clone().requires_grad_(True)
    s2 = torch.full((P,), 0.33, dtype=torch.float64, device="cuda")
    (2.0 * ppo_clip_loss(p2, d["feat"], d["pol"], d["eps"], y_old, d["adv"], 0.33, sigma_old=0.3)).backward()
    assert torch.equal(p2.grad, 2.0 * _call(d, "ppo", d["new"], y_old=y_old, sigma=s2)["grad"])
    # the critic
    vwant = _call(d, "mse", d["new"])
    vparams = d["new"].clone().requires_grad_(True)
    vopt = torch.optim.Adam([vparams], lr=1e-2)
    vl = value_loss(vparams, d["feat"], d["pol"], d["target"])
    vopt.zero_grad(); vl.backward()
    assert torch.equal(vparams.grad, vwant["grad"]) and float(vl) == float(vwant["stats"][:, 0].sum() / (K * n))
    vopt.step()
    assert float(value_loss(vparams, d["feat"], d["pol"], d["target"])) < float(vl)
    # without grad nothing is recorded; bad input raises
    with torch.no_grad():
        assert not ppo_clip_loss(params, d["feat"], d["pol"], d["eps"], y_old, d["adv"], sigma).requires_grad
    with pytest.raises(ValueError):
        ppo_clip_loss(params, d["feat"], d["pol"], d["eps"].t().contiguous().t(), y_old, d["adv"], 0.3)
    with pytest.raises(ValueError):
        ppo_clip_loss(params, d["feat"], d["pol"], d["eps"].float(), y_old, d["adv"], 0.3)
    with pytest.raises(ValueError):
        ppo_clip_loss(params, d["feat"], d["pol"], d["eps"], y_old, d["adv"], 0.3, clip=1.0)
    with pytest.raises(ValueError):
        value_loss(vparams, d["feat"], d["pol"], d["target"][:-1])
    # the trained weights go back into the collector
    pol2 = MLPController.from_flat(params, d["pol"].widths, history=history, hidden="tanh")
    assert torch.equal(pol2.device_params(params.device, torch.float64), params.detach())
    env = BatchedT1DSimEnv(patient=["child#001", "adult#001"] * (n // 2), sensor="Dexcom", dtype=torch.float64, seed=3)
    env.reset()
    tr = env.new_trace(2, columns=("action", "features", "eps"), history=history)
    env.collect_mlp(2, pol2, sigma=sigma.detach(), on_done="continue", trace=tr)
    assert env.sync() == 0 and bool(torch.isfinite(tr["action"][1:]).all())
