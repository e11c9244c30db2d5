"""CPU suite: t1d_mlp_loss without a GPU -- the exports, the struct mirror, the workspace size, every argument check
(validation comes before any HIP call), the closed-form references against autograd on the torch form of the loss, and the
input recipe of the GPU suite (tests/test_gpu_policy_loss.py imports it from here)."""
import ctypes as C
import functools
import os
import re

import pytest
import torch

from support import identity_policy as _policy, mlp_struct as _mlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP = 0.2

# the shapes of GRAD_CASES in tests/test_gpu_policy_grad.py: history, widths, n, K
LOSS_CASES = [
    (4, (8, 8, 1), 128, 3), (4, (8, 8, 1), 256, 5),                     # one chunk per policy (P = 2), two chunks
    (12, (32, 32, 32, 1), 128, 3), (12, (32, 32, 32, 1), 256, 5),
    (4, (1,), 128, 3), (4, (1,), 256, 5),
    (2, (5, 1), 256, 1100),         # 4400 tiles in all, more than 2048: a wave takes three, across chunks and rows
]


# ------------------------------------------------------------------------------------------------ the GPU suite's inputs
def host_y(pol, params, feat):
    """y [K, n] in fp64 on the CPU under params [P, n_params]: MLPController.pre_output(ordered=True), the kernel's order, on
    all K rows at once (the envs regrouped so that policy p still owns one contiguous block)"""
    from simglucose_amd.controller.mlp_ctrller import MLPController
    K, F, n = feat.shape
    P = params.shape[0]
    net = MLPController.from_flat(params.double(), pol.widths, history=pol.history, hidden=pol.hidden)
    cols = feat.double().reshape(K, F, P, n // P).permute(1, 2, 0, 3).reshape(F, P * K * (n // P))
    return net.pre_output(cols, ordered=True).reshape(P, K, n // P).permute(1, 0, 2).reshape(K, n)


@functools.lru_cache(maxsize=None)
def recipe(history, widths, n, K, P, hidden, f64):
    """The inputs of one GPU case, on the CPU, every array rounded to the case's dtype: the collector's weights and the new
    ones (old + 0.05 randn), features in [-2, 2], eps and adv standard normal, a value target, sigma_old = 0.3 and sigma !=
    sigma_old per policy.  Then, on the fp64 reference alone, eps of a sample is moved up by 1/64 until the sample is clear of
    everything a rounding error could tip: r at least 1e-3 (relative) from both clip boundaries, and |e_new| and |eps| at least
    1/32 -- z - y cancels near 0 and no tolerance relative to coef means anything there.  Computed once per case."""
    from simglucose_amd.controller.policy_loss import ppo_clip_loss_reference
    dtype = torch.float64 if f64 else torch.float32
    rd = lambda t: t.to(dtype).double()
    pol = _policy(history, widths, P, hidden=hidden, seed=7)
    g = torch.Generator().manual_seed(11)
    feat = rd(torch.rand(K, pol.n_features, n, generator=g, dtype=torch.float64) * 4 - 2)
    eps = rd(torch.randn(K, n, generator=g, dtype=torch.float64))
    adv = rd(torch.randn(K, n, generator=g, dtype=torch.float64))
    old = rd(pol.flat_params())
    new = rd(old + 0.05 * torch.randn(old.shape, generator=g, dtype=torch.float64))
    target = rd(torch.randn(K, n, generator=g, dtype=torch.float64))
    sigma_old = rd(torch.full((P,), 0.3, dtype=torch.float64))
    sigma = rd(torch.tensor([0.33, 0.28], dtype=torch.float64)[:P])
    y_old, y = host_y(pol, old, feat), host_y(pol, new, feat)
    for _ in range(64):
        r = ppo_clip_loss_reference(y, eps, y_old, adv, sigma, sigma_old, CLIP, P)[4]["r"]
        E = n // P
        e_new = (sigma_old.repeat_interleave(E) * eps + y_old - y) / sigma.repeat_interleave(E)
        bad = ((r - (1 - CLIP)).abs() <= 1e-3 * (1 - CLIP)) | ((r - (1 + CLIP)).abs() <= 1e-3 * (1 + CLIP))
        bad |= (e_new.abs() < 1 / 32) | (eps.abs() < 1 / 32)
        if not bool(bad.any()):
            break
        eps = rd(eps + bad.double() / 64)
    else:
        raise AssertionError("the recipe does not settle")
    return dict(pol=pol, dtype=dtype, P=P, feat=feat, eps=eps, adv=adv, old=old, new=new, target=target, sigma_old=sigma_old,
                sigma=sigma, y_old=y_old, y=y)


# ------------------------------------------------------------------------------------------------ 1: exports, struct
def test_symbols_are_exported():
    from simglucose_amd import _lib
    L = _lib.lib()
    for name in ("t1d_mlp_loss_workspace", "t1d_mlp_loss"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.t1d_abi_version() == 4


def test_mlp_loss_struct_layout_matches_header():
    from simglucose_amd import _lib
    src = open(os.path.join(ROOT, "include", "t1d.h")).read()
    body = src[src.index("struct t1d_mlp_loss {"):]
    body = body[:body.index("};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("struct t1d_mlp_loss {", "")
    fields, sizes = [], []
    for stmt in body.split(";"):
        for k, part in enumerate(stmt.split(",")):
            m = re.findall(r"([A-Za-z_0-9]+)\s*$", part.strip())
            if m and part.strip():
                fields.append(m[0])
                sizes.append(4 if "int32_t" in stmt else 8)
    assert fields == [f[0] for f in _lib.MlpLoss._fields_]
    assert [C.sizeof(f[1]) for f in _lib.MlpLoss._fields_] == sizes
    assert C.sizeof(_lib.MlpLoss) == sum(sizes)                        # no padding: the two int32 share a word
    assert (_lib.T1D_LOSS_PPO_CLIP, _lib.T1D_LOSS_VALUE_MSE) == (1, 2)
    assert "T1D_LOSS_PPO_CLIP = 1, T1D_LOSS_VALUE_MSE = 2" in src


# ------------------------------------------------------------------------------------------------ 2: workspace
def test_workspace_size():
    """the header's formula: t1d_mlp_grad_workspace rounded up to 8, plus 32 bytes for every partial"""
    from simglucose_amd import _lib
    L = _lib.lib()
    p = _mlp()
    for dtype in (_lib.T1D_F64, _lib.T1D_F32):
        for n, K, P in ((128, 3, 2), (64, 3, 1), (256, 1100, 2), (128, 100000, 2)):
            p.n_policies, p.envs_per_policy = P, n // P
            W = L.t1d_mlp_grad_workspace(C.byref(p), dtype, n, K)
            C_, T = n // P // 64, max(1, -(-P * (n // P // 64) * K // 2048))
            partials = P * -(-C_ * K // T)
            assert W == partials * p.n_params * (8 if dtype == _lib.T1D_F64 else 4)
            assert L.t1d_mlp_loss_workspace(C.byref(p), dtype, n, K) == (W + 7) // 8 * 8 + 32 * partials
    p = _mlp(n_policies=1)
    assert L.t1d_mlp_grad_workspace(C.byref(p), _lib.T1D_F32, 64, 3) % 8 == 4       # the rounding is exercised
    assert L.t1d_mlp_loss_workspace(C.byref(p), _lib.T1D_F32, 64, 3) % 8 == 0
    p.params = None                                                   # the weights are not needed for the size
    assert L.t1d_mlp_loss_workspace(C.byref(p), _lib.T1D_F64, 64, 3) > 0
    assert L.t1d_mlp_loss_workspace(C.byref(_mlp(widths=(33, 1))), _lib.T1D_F64, 128, 3) < 0
    assert L.t1d_mlp_loss_workspace(C.byref(_mlp()), _lib.T1D_F64, 128, 0) < 0
    assert L.t1d_mlp_loss_workspace(C.byref(_mlp()), 7, 128, 3) < 0
    assert L.t1d_mlp_loss_workspace(None, _lib.T1D_F64, 128, 3) < 0


# ------------------------------------------------------------------------------------------------ 3: argument checks
def test_every_invalid_argument_is_rejected_without_a_gpu():
    """-1 (T1D_E_INVALID) whether or not a device is present: nothing is launched, the device is not touched."""
    from simglucose_amd import _lib
    L = _lib.lib()
    F64 = _lib.T1D_F64
    PPO, MSE = _lib.T1D_LOSS_PPO_CLIP, _lib.T1D_LOSS_VALUE_MSE

    def io(kind=PPO, **kw):
        b = _lib.MlpLoss()
        d = dict(n_rows=3, feat=0x2000, eps=0x3000, y_old=0x4000, adv=0x5000, sigma_old=0x6000, sigma=0x7000, target=0x8000,
                 clip=0.2, scale=1.0 / 384, y=0x9000, coef_out=0xa000, grad=0xb000, stats=0xc000, workspace=0xd000,
                 workspace_bytes=1 << 30)
        d.update(kw)
        b.kind = kind
        for k, v in d.items():
            setattr(b, k, v)
        return b

    def call(p, b, n=128, dtype=F64):
        return L.t1d_mlp_loss(0, dtype, n, C.byref(p) if p is not None else None, C.byref(b) if b is not None else None, None)

    ok = _mlp()
    # everything t1d_mlp_grad rejects
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
    assert call(ok, io(), n=192) == -1 and b"n_policies * envs_per_policy" in L.t1d_last_error()
    assert call(_mlp(envs_per_policy=96), io(), n=192) == -1 and b"multiple of 64" in L.t1d_last_error()
    assert call(ok, io(n_rows=0)) == -1 and b"n_rows" in L.t1d_last_error()
    assert call(ok, io(feat=None)) == -1 and b"feat" in L.t1d_last_error()
    # the kind and the inputs it needs
    for kind in (0, 3, -1):
        assert call(ok, io(kind=kind)) == -1 and b"kind" in L.t1d_last_error()
    for name in ("eps", "y_old", "adv", "sigma_old", "sigma"):
        assert call(ok, io(**{name: None})) == -1 and b"T1D_LOSS_PPO_CLIP needs" in L.t1d_last_error(), name
    assert call(ok, io(kind=MSE, target=None)) == -1 and b"target" in L.t1d_last_error()
    # clip and scale
    for clip in (0.0, 1.0, -0.2, 1.5, float("nan"), float("inf")):
        assert call(ok, io(clip=clip)) == -1 and b"clip" in L.t1d_last_error(), clip
    for scale in (float("nan"), float("inf"), float("-inf")):
        assert call(ok, io(scale=scale)) == -1 and b"scale" in L.t1d_last_error()
        assert call(ok, io(kind=MSE, scale=scale)) == -1 and b"scale" in L.t1d_last_error()
    # the outputs and the workspace
    assert call(ok, io(y=None, coef_out=None, grad=None, stats=None)) == -1 and b"all NULL" in L.t1d_last_error()
    need = L.t1d_mlp_loss_workspace(C.byref(ok), F64, 128, 3)
    for kind in (PPO, MSE):
        for out in (dict(stats=None), dict(grad=None), dict()):
            assert call(ok, io(kind=kind, workspace=None, **out)) == -1 and b"workspace" in L.t1d_last_error()
            assert call(ok, io(kind=kind, workspace_bytes=need - 1, **out)) == -1 and b"workspace" in L.t1d_last_error()


def test_python_argument_checks_raise_value_error():
    """what can be refused before the device is needed: tensors on the CPU are refused like mlp_pre_output refuses them"""
    from simglucose_amd.controller import ppo_clip_loss, value_loss
    pol = _policy(4, (8, 8, 1), 2, hidden="tanh", seed=1)
    feat = torch.zeros(3, pol.n_features, 128, dtype=torch.float64)
    a = torch.zeros(3, 128, dtype=torch.float64)
    with pytest.raises(ValueError, match="ppo_clip_loss"):
        ppo_clip_loss(pol.flat_params(), feat, pol, a, a, a, 0.3)
    with pytest.raises(ValueError, match="value_loss"):
        value_loss(pol.flat_params(), feat, pol, a)
    with pytest.raises(ValueError):
        ppo_clip_loss(pol.flat_params().float(), feat, pol, a, a, a, 0.3)


# ------------------------------------------------------------------------------------------------ 4: the references
@pytest.mark.parametrize("hidden", ["tanh", "relu"])
@pytest.mark.parametrize("P", [1, 2])
def test_references_are_autograd_of_the_torch_form(P, hidden):
    """loss, d loss / d y and d loss / d sigma of the closed forms against autograd on the expression INTEGRATION.md gives
    (log_prob, exp, clamp, torch.minimum, .mean()), fp64 on the CPU, y from pre_output(ordered=True).  Both are a handful of
    fp64 operations per sample on words of order 1 to 10: 1e-12 relative to the largest term is a thousand roundings."""
    from simglucose_amd.controller import ppo_clip_loss_reference, value_loss_reference
    from simglucose_amd.controller.mlp_ctrller import MLPController
    c = recipe(4, (8, 8, 1), 64 * P * 2, 3, P, hidden, True)
    E = c["feat"].shape[2] // P
    y = c["y"].clone().requires_grad_(True)
    sg = c["sigma"].clone().requires_grad_(True)
    so_e, sg_e = c["sigma_old"].repeat_interleave(E), sg.repeat_interleave(E)
    z = c["y_old"] + so_e * c["eps"]
    old_logp = MLPController.log_prob((z - c["y_old"]) / so_e, so_e)
    ratio = (MLPController.log_prob((z - y) / sg_e, sg_e) - old_logp).exp()
    loss = -torch.minimum(ratio * c["adv"], ratio.clamp(1 - CLIP, 1 + CLIP) * c["adv"]).mean()
    dy, ds = torch.autograd.grad(loss, (y, sg))
    ref_loss, coef, stats, dsig, info = ppo_clip_loss_reference(c["y"], c["eps"], c["y_old"], c["adv"], c["sigma"], c["sigma_old"],
                                                              CLIP, P)
    assert abs(float(ref_loss) - float(loss.detach())) <= 1e-12 * float(info["loss_mag"].sum()) / y.numel()
    assert bool(((coef - dy).abs() <= 1e-12 * info["coef_mag"] + 1e-300).all()) and float(dy.abs().max()) > 0
    assert bool(((dsig - ds).abs() <= 1e-12 * info["dsig_mag"] / y.numel()).all()) and float(ds.abs().min()) > 0
    assert torch.equal(ratio.detach() > 0, torch.ones_like(ratio, dtype=torch.bool))
    assert bool(((info["r"] - ratio.detach()).abs() <= 1e-12 * info["r"]).all())
    # clip fraction and approximate KL as a trainer forms them by hand
    n_s = 3 * E
    clipped = ((ratio.detach() - 1).abs() > CLIP) & (torch.where(c["adv"] >= 0, ratio.detach() > 1, ratio.detach() < 1))
    assert torch.equal(stats[:, 1], clipped.reshape(3, P, E).sum(dim=(0, 2)).double())
    kl = ((ratio.detach() - 1) - ratio.detach().log()).reshape(3, P, E).sum(dim=(0, 2))
    assert bool(((stats[:, 2] - kl).abs() <= 1e-9 * kl).all()) and float(kl.min()) > 1e-3 * n_s
    # the value loss
    y2 = c["y"].clone().requires_grad_(True)
    vl = 0.5 * ((y2 - c["target"]) ** 2).mean()
    dv, = torch.autograd.grad(vl, y2)
    ref_vl, vcoef, vstats, none = value_loss_reference(c["y"], c["target"], P)
    assert none is None and abs(float(ref_vl) - float(vl.detach())) <= 1e-12 * float(vl.detach())
    assert bool(((vcoef - dv).abs() <= 1e-12 * dv.abs() + 1e-300).all())
    assert bool((vstats[:, 1:] == 0).all()) and abs(float(vstats[:, 0].sum()) / y.numel() - float(vl.detach())) <= 1e-12 * float(vl.detach())


def test_reference_at_unchanged_weights():
    """y == y_old and sigma == sigma_old: r is exactly 1, nothing is clipped, the KL term is exactly 0.0"""
    from simglucose_amd.controller import ppo_clip_loss_reference
    c = recipe(4, (8, 8, 1), 128, 3, 2, "tanh", True)
    loss, coef, stats, dsig, info = ppo_clip_loss_reference(c["y_old"], c["eps"], c["y_old"], c["adv"], c["sigma_old"], None, CLIP, 2)
    assert bool((info["r"] == 1.0).all()) and bool((stats[:, 1] == 0).all()) and bool((stats[:, 2] == 0.0).all())
    assert abs(float(loss) + float(c["adv"].mean())) <= 1e-15 * float(c["adv"].abs().mean())


# ------------------------------------------------------------------------------------------------ 5: the GPU suite's recipe
@pytest.mark.parametrize("hidden,f64", [("tanh", True), ("relu", True), ("tanh", False)])
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("history,widths,n,K", LOSS_CASES)
def test_gpu_recipe_is_clear_of_the_clip_boundaries_and_runs_both_branches(history, widths, n, K, P, hidden, f64):
    from simglucose_amd.controller import ppo_clip_loss_reference
    c = recipe(history, widths, n, K, P, hidden, f64)
    info = ppo_clip_loss_reference(c["y"], c["eps"], c["y_old"], c["adv"], c["sigma"], c["sigma_old"], CLIP, P)[4]
    r, active = info["r"], info["active"]
    for edge in (1 - CLIP, 1 + CLIP):
        assert not bool(((r - edge).abs() <= 1e-4 * edge).any())      # fp32 cannot land on the other side
    assert not torch.equal(c["sigma"], c["sigma_old"])
    for pos in (True, False):
        for act in (True, False):
            share = float((((c["adv"] >= 0) == pos) & (active == act)).double().mean())
            assert share >= 0.02, (pos, act, share)
    # relu: no hidden unit sits on the kink, so fp32 and fp64 take the same side (as test_gpu_policy_grad.py asks)
    if hidden == "relu" and len(widths) > 1:
        for params in (c["old"], c["new"]):
            assert c["pol"].grad_reference(c["feat"], c["adv"], params=params, info=True)[1]["min_abs_pre"] > 1e-8
