"""The PPO-clip and value losses of the in-kernel policy network with the loss inside the gradient launch:
``ppo_clip_loss`` and ``value_loss`` (t1d_mlp_loss in ``include/t1d.h``, ``csrc/t1d_policy_grad.hpp``), one forward pass of
the network per call, and ``ppo_clip_loss_reference`` / ``value_loss_reference``, the same arithmetic in plain torch and
fp64.  With ``tiles=`` either loss runs on a minibatch, a list of 64-env tiles of the batch read in place
(t1d_mlp_loss_tiles); ``tile_minibatches`` draws the lists of an epoch and ``gather_tiles`` restates one as a copy."""
import ctypes as C

import torch

from .. import _lib
from .mlp_grad import _check as _check_net, _struct, _T1D_DTYPE, check_tiles, tile_list

_workspaces = {}                          # (device, bytes) -> tensor: one per shape, reused by every call


def _check(who, params, features, policy, arrays):
    """mlp_grad._check under this function's name, then every [K, n] array of the loss"""
    try:
        _check_net(params, features, policy)
    except ValueError as e:
        raise ValueError(str(e).replace("mlp_pre_output", who)) from None
    K, n = features.shape[0], features.shape[2]
    for name, t in arrays:
        if not isinstance(t, torch.Tensor) or t.dtype != features.dtype:
            raise ValueError("%s: %s must be a %s tensor" % (who, name, features.dtype))
        if t.device != features.device:
            raise ValueError("%s: %s must be on the features' device" % (who, name))
        if tuple(t.shape) != (K, n):
            raise ValueError("%s: %s must be [%d, %d]" % (who, name, K, n))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (who, name))


def _sigma(who, sigma, name, P, like):
    """a float or a [P] tensor -> a contiguous [P] tensor of features' dtype on its device (detached)"""
    if isinstance(sigma, torch.Tensor):
        if sigma.dim() != 1 or sigma.shape[0] != P:
            raise ValueError("%s: %s must be a float or a [%d] tensor" % (who, name, P))
        if sigma.device != like.device or sigma.dtype != like.dtype:
            raise ValueError("%s: %s must have the features' device and dtype" % (who, name))
        return sigma.detach().contiguous()
    if not float(sigma) > 0.0:
        raise ValueError("%s: %s must be > 0" % (who, name))
    return torch.full((P,), float(sigma), dtype=like.dtype, device=like.device)


def mlp_loss_call(policy, params, features, kind, scale, eps=None, y_old=None, adv=None, sigma_old=None, sigma=None,
                  target=None, clip=0.2, y=None, coef_out=None, grad=None, stats=None, workspace=None, tiles=None):
    """One t1d_mlp_loss call on the current stream of the features' device.  kind: _lib.T1D_LOSS_PPO_CLIP (eps, y_old, adv
    [K, n], sigma_old, sigma [P]) or _lib.T1D_LOSS_VALUE_MSE (target [K, n]).  y, coef_out [K, n], grad [P, n_params] and
    stats [P, 4] (float64) are written where given.  workspace: a tensor of at least t1d_mlp_loss_workspace bytes
    (default: the cached one of this shape).  tiles (int32 [P, M] on the device, or [M] with P == 1): t1d_mlp_loss_tiles
    on the listed 64-env tiles u = row * C + chunk of every policy instead; y and coef_out are then written at those tiles
    alone, and the workspace is that of t1d_mlp_loss_tiles_workspace."""
    L = _lib.lib()
    K, _, n = features.shape
    p = _struct(policy, params, n)
    dt = _T1D_DTYPE[features.dtype]
    if tiles is not None:
        tiles = check_tiles("mlp_loss_call", tiles, features, params.shape[0])
    io = _lib.MlpLoss()
    io.n_rows, io.kind, io.feat, io.clip, io.scale = K, int(kind), features.data_ptr(), float(clip), float(scale)
    for name, t in (("eps", eps), ("y_old", y_old), ("adv", adv), ("sigma_old", sigma_old), ("sigma", sigma), ("target", target),
                    ("y", y), ("coef_out", coef_out), ("grad", grad), ("stats", stats)):
        setattr(io, name, t.data_ptr() if t is not None else None)
    if grad is not None or stats is not None:
        if workspace is None:
            need = L.t1d_mlp_loss_workspace(C.byref(p), dt, n, K) if tiles is None else \
                L.t1d_mlp_loss_tiles_workspace(C.byref(p), dt, n, tiles.shape[1])
            if need < 0:
                _lib.check(int(need))
            key = (str(features.device), need)
            if key not in _workspaces:
                _workspaces[key] = torch.empty(need, dtype=torch.uint8, device=features.device)
            workspace = _workspaces[key]
        io.workspace, io.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    with torch.cuda.device(features.device):
        stream = C.c_void_p(torch.cuda.current_stream(features.device).cuda_stream)
        if tiles is None:
            _lib.check(L.t1d_mlp_loss(features.device.index, dt, n, C.byref(p), C.byref(io), stream))
        else:
            _lib.check(L.t1d_mlp_loss_tiles(features.device.index, dt, n, C.byref(p), C.byref(io), C.byref(tile_list(tiles)), stream))


class _Loss(torch.autograd.Function):
    """forward: the one fused call, which also gives grad and sum dsig; backward: those times grad_output"""

    @staticmethod
    def forward(ctx, params, sigma, features, policy, kind, inputs):
        K, n = features.shape[0], features.shape[2]
        tiles = inputs.get("tiles")
        scale = 1.0 / (K * n) if tiles is None else 1.0 / (64 * tiles.shape[1] * params.shape[0])
        want_grad = ctx.needs_input_grad[0]
        grad = torch.empty_like(params) if want_grad else None
        stats = torch.empty(params.shape[0], 4, dtype=torch.float64, device=features.device)
        mlp_loss_call(policy, params.detach(), features, kind, scale, grad=grad, stats=stats, **inputs)
        ctx.grad, ctx.scale = grad, scale
        ctx.dsig = stats[:, 3] if ctx.needs_input_grad[1] else None
        ctx.sigma_dtype = sigma.dtype if isinstance(sigma, torch.Tensor) else None
        ctx.mark_non_differentiable(stats)
        return (stats[:, 0].sum() * scale).to(params.dtype), stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        g_params = g_loss.to(ctx.grad.dtype) * ctx.grad if ctx.grad is not None else None
        g_sigma = (g_loss.double() * ctx.scale * ctx.dsig).to(ctx.sigma_dtype) if ctx.dsig is not None else None
        return g_params, g_sigma, None, None, None, None


def ppo_clip_loss(params, features, policy, eps, y_old, adv, sigma, sigma_old=None, clip=0.2, return_stats=False, tiles=None):
    """The clipped PPO surrogate -mean(min(r adv, clamp(r, 1 - clip, 1 + clip) adv)) over all K * n samples, r the ratio of
    the Gaussian densities N(y, sigma^2) / N(y_old, sigma_old^2) at the action the collector took, with the network, the
    loss, its derivative and the weight gradient in ONE launch that evaluates the network once (t1d_mlp_loss; the arithmetic
    is in include/t1d.h).  params [P, n_params] and features [K, F, n] as for mlp_pre_output; eps = tr["eps"][1:], y_old =
    mlp_pre_output under the collector's weights, adv [K, n]: contiguous, the features' dtype and device.  sigma: a float, or
    a [P] tensor that may require grad; sigma_old: what the collector used (default: sigma's current value).  A float is
    checked to be > 0; a tensor is device data and is not read on the host, so its positivity is the caller's responsibility,
    as in the C call.  -> a scalar,
    differentiable in params and in a tensor sigma: backward only scales what the forward call already computed.  With
    return_stats=True -> (loss, {"loss", "clip_frac", "approx_kl"}), each [P] float64: per policy the mean loss, the share
    of samples whose gradient the clip removed, and the mean of (r - 1) - log r.  The sums have an order fixed by the shapes:
    two calls give identical bits.  Raises ValueError for non-contiguous input, a wrong dtype, device or shape.

    tiles (default None: all samples): a minibatch as an int32 [P, M] contiguous tensor on the features' device ([M] is also
    taken with P == 1), one of tile_minibatches' lists: per policy M ids u = row * C + chunk (C = n / P / 64) of 64-env
    tiles of the batch.  Every array keeps its full shape and is read in place; nothing is gathered.  The loss is then the
    mean over the 64 * M * P listed samples and the statistics are divided by 64 * M.  A tile listed twice counts twice.
    An id < 0 or >= C * K is skipped by the kernel (-1 pads a list) and still counts in 64 * M: skipped ids dilute the
    mean.  The result equals, bit for bit, the call without tiles on gather_tiles of every array.

        y_old = mlp_pre_output(pol.device_params(env.device, env.dtype), f, pol)
        for epoch in range(epochs):
            for mb in tile_minibatches(K, n, pol.n_policies, 4, device=f.device):
                loss = ppo_clip_loss(params, f, pol, eps, y_old, adv, sig, tiles=mb)
                opt.zero_grad(); loss.backward(); opt.step()
    """
    who = "ppo_clip_loss"
    if tiles is not None:
        tiles = check_tiles(who, tiles, features, policy.n_policies)
    _check(who, params, features, policy, (("eps", eps), ("y_old", y_old), ("adv", adv)))
    if not 0.0 < float(clip) < 1.0:
        raise ValueError("ppo_clip_loss: clip must be in (0, 1)")
    P = policy.n_policies
    sg = _sigma(who, sigma, "sigma", P, features)
    so = sg if sigma_old is None else _sigma(who, sigma_old, "sigma_old", P, features)
    inputs = dict(eps=eps.detach(), y_old=y_old.detach(), adv=adv.detach(), sigma_old=so, sigma=sg, clip=float(clip))
    if tiles is not None:
        inputs["tiles"] = tiles
    loss, stats = _Loss.apply(params, sigma, features.detach(), policy, _lib.T1D_LOSS_PPO_CLIP, inputs)
    if not return_stats:
        return loss
    count = features.shape[0] * (features.shape[2] // P) if tiles is None else 64 * tiles.shape[1]
    return loss, {"loss": stats[:, 0] / count, "clip_frac": stats[:, 1] / count, "approx_kl": stats[:, 2] / count}


def value_loss(params, features, policy, target, tiles=None):
    """The critic's regression loss 0.5 * mean((y - target)^2) over all K * n samples, with the network, the loss and the
    weight gradient in one launch (t1d_mlp_loss, T1D_LOSS_VALUE_MSE).  target [K, n] (gae's ret): contiguous, the features'
    dtype and device.  -> a scalar, differentiable in params.  tiles: a minibatch as for ppo_clip_loss -- the mean is then
    over the 64 * M * P listed samples, and skipped ids dilute it."""
    if tiles is not None:
        tiles = check_tiles("value_loss", tiles, features, policy.n_policies)
    _check("value_loss", params, features, policy, (("target", target),))
    inputs = dict(target=target.detach())
    if tiles is not None:
        inputs["tiles"] = tiles
    loss, _ = _Loss.apply(params, None, features.detach(), policy, _lib.T1D_LOSS_VALUE_MSE, inputs)
    return loss


def tile_minibatches(n_rows, n, n_policies, n_minibatches, generator=None, device=None):
    """The minibatches of one epoch over a batch of n_rows rows of n envs: a list of n_minibatches int32 [P, M] tensors for
    tiles=, M = (C * n_rows) // n_minibatches with C = n / P / 64.  Every policy gets its own random permutation of its tile
    ids 0 .. C * n_rows - 1, cut into the lists; the (C * n_rows) % n_minibatches tiles left over are left out of this
    epoch (no padding).  Pure torch, on `device` (default: the CPU) with `generator`.  Raises ValueError when M == 0 or n
    is not a multiple of 64 * n_policies."""
    P, B = int(n_policies), int(n_minibatches)
    if P < 1 or B < 1 or n_rows < 1 or n < 1 or n % (64 * P):
        raise ValueError("tile_minibatches: %d envs do not split into %d policies of a multiple of 64 envs each" % (n, P))
    total = n // P // 64 * int(n_rows)
    M = total // B
    if M == 0:
        raise ValueError("tile_minibatches: %d tiles per policy do not fill %d minibatches" % (total, B))
    perm = torch.stack([torch.randperm(total, generator=generator, device=device) for _ in range(P)]).to(torch.int32)
    return [perm[:, b * M:(b + 1) * M].contiguous() for b in range(B)]


def gather_tiles(t, tiles, n_policies):
    """The listed tiles of t ([K, n] or [K, F, n]) as a batch of their own: [M, 64 P] or [M, F, 64 P] with row j of policy p
    (envs 64 p .. 64 p + 63) holding tile tiles[p][j] of t -- what a call with tiles= reads in place, as a copy.  tiles: an
    integer [P, M] tensor ([M] with P == 1) of ids in [0, C * K); the gathered batch has no place for skipped ids."""
    P = int(n_policies)
    if tiles.dim() == 1:
        tiles = tiles.unsqueeze(0)
    K, n = t.shape[0], t.shape[-1]
    Cn = n // P // 64
    idx = tiles.long()
    pol = torch.arange(P, device=idx.device).unsqueeze(1)
    row, chunk = idx // Cn, idx % Cn
    if t.dim() == 2:
        g = t.view(K, P, Cn, 64).permute(1, 0, 2, 3)[pol, row, chunk]              # [P, M, 64]
        return g.permute(1, 0, 2).reshape(idx.shape[1], 64 * P).contiguous()
    F = t.shape[1]
    g = t.view(K, F, P, Cn, 64).permute(2, 0, 3, 1, 4)[pol, row, chunk]            # [P, M, F, 64]
    return g.permute(1, 2, 0, 3).reshape(idx.shape[1], F, 64 * P).contiguous()


def _per_env(sigma, P, n, device):
    s = torch.as_tensor(sigma, dtype=torch.float64, device=device).detach()
    return (s.expand(P) if s.dim() == 0 else s).repeat_interleave(n // P)


def ppo_clip_loss_reference(y, eps, y_old, adv, sigma, sigma_old=None, clip=0.2, n_policies=1, scale=None):
    """T1D_LOSS_PPO_CLIP of include/t1d.h in plain torch and fp64, in closed form (no autograd): y, eps, y_old, adv [K, n],
    sigma and sigma_old a float or [P] -> (loss, coef [K, n], stats [P, 4], dsig [P], info) with loss = scale * sum loss_i,
    coef = d loss / d y, dsig = d loss / d sigma (both scaled; scale defaults to 1 / (K n)), stats the unscaled sums of
    t1d_mlp_loss, and info a dict of what a tolerance is stated in: "r" [K, n], "active" [K, n], "coef_mag" [K, n] = |scale
    adv r e_new / sigma|, "loss_mag" and "dsig_mag" [P] = the per-policy sums of |loss_i| and |dsig_i|."""
    y, eps, y_old, adv = (t.detach().to(torch.float64) for t in (y, eps, y_old, adv))
    K, n = y.shape
    P = int(n_policies)
    k = 1.0 / (K * n) if scale is None else float(scale)
    sg = _per_env(sigma, P, n, y.device)
    so = sg if sigma_old is None else _per_env(sigma_old, P, n, y.device)
    z = so * eps + y_old
    e_old, e_new = (z - y_old) / so, (z - y) / sg
    logr = 0.5 * ((e_old - e_new) * (e_old + e_new)) + (so.log() - sg.log())
    r = logr.exp()
    lo, hi = 1.0 - float(clip), 1.0 + float(clip)
    active = torch.where(adv >= 0, r <= hi, r >= lo)
    ra = r * adv
    loss_i = -torch.where(ra <= r.clamp(lo, hi) * adv, ra, r.clamp(lo, hi) * adv)
    g = torch.where(active, -ra, torch.zeros_like(ra))
    coef = k * g * e_new / sg
    dsig_i = g * (e_new * e_new - 1.0) / sg
    per = lambda t: t.reshape(K, P, n // P).sum(dim=(0, 2))
    stats = torch.stack([per(loss_i), per((~active).double()), per(torch.expm1(logr) - logr), per(dsig_i)], dim=1)
    info = {"r": r, "active": active, "coef_mag": (k * adv * r * e_new / sg).abs(), "loss_mag": per(loss_i.abs()),
            "dsig_mag": per(dsig_i.abs())}
    return k * loss_i.sum(), coef, stats, k * stats[:, 3], info


def value_loss_reference(y, target, n_policies=1, scale=None):
    """T1D_LOSS_VALUE_MSE in plain torch and fp64: -> (loss, coef [K, n], stats [P, 4], None), as ppo_clip_loss_reference"""
    y, target = y.detach().to(torch.float64), target.detach().to(torch.float64)
    K, n = y.shape
    P = int(n_policies)
    k = 1.0 / (K * n) if scale is None else float(scale)
    d = y - target
    loss_i = 0.5 * d * d
    stats = torch.zeros(P, 4, dtype=torch.float64, device=y.device)
    stats[:, 0] = loss_i.reshape(K, P, n // P).sum(dim=(0, 2))
    return k * loss_i.sum(), k * d, stats, None
