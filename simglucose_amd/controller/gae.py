"""Advantages, value targets and per-policy advantage moments of a collected batch on the device: ``gae`` (t1d_gae in
``include/t1d.h``, ``csrc/t1d_gae.hpp``), and ``gae_reference``, the same recurrence as a plain torch loop in fp64."""
import ctypes as C

import torch

from .. import _lib

_T1D_DTYPE = {torch.float64: _lib.T1D_F64, torch.float32: _lib.T1D_F32}
_workspaces = {}                          # (device, bytes) -> tensor: one per shape, reused by every call


def _check(reward, done, value, last_value, gamma, lam, n_policies, truncated=None, cut_value=None):
    if not isinstance(reward, torch.Tensor) or reward.dtype not in _T1D_DTYPE:
        raise ValueError("gae: reward must be a float64 or float32 tensor")
    if reward.device.type != "cuda":
        raise ValueError("gae: reward must be on a GPU")
    if reward.dim() != 2 or reward.shape[0] < 1 or reward.shape[1] < 1:
        raise ValueError("gae: reward must be [K >= 1, n >= 1]")
    K, n = reward.shape
    for name, t, dt, shape in (("done", done, torch.uint8, (K, n)), ("value", value, reward.dtype, (K, n)),
                               ("last_value", last_value, reward.dtype, (n,)), ("truncated", truncated, torch.uint8, (K, n)),
                               ("cut_value", cut_value, reward.dtype, (n,))):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise ValueError("gae: %s must be a %s tensor" % (name, dt))
        if t.device != reward.device:
            raise ValueError("gae: %s must be on reward's device" % name)
        if tuple(t.shape) != shape:
            raise ValueError("gae: %s must be %s" % (name, list(shape)))
        if not t.is_contiguous():
            raise ValueError("gae: %s must be contiguous" % name)
    if not reward.is_contiguous():
        raise ValueError("gae: reward must be contiguous")
    if not (0.0 <= float(gamma) <= 1.0) or not (0.0 <= float(lam) <= 1.0):
        raise ValueError("gae: gamma and lam must be in [0, 1]")
    if int(n_policies) < 1 or n % int(n_policies):
        raise ValueError("gae: %d envs do not split into %d policies" % (n, int(n_policies)))
    if cut_value is not None and truncated is None:
        raise ValueError("gae: cut_value needs truncated")


def gae_call(reward, done=None, value=None, last_value=None, gamma=0.99, lam=0.95, n_policies=1, adv=None, ret=None,
             moments=None, workspace=None, truncated=None, cut_value=None):
    """One t1d_gae call on the current stream of reward's device (t1d_gae_limit with truncated).  adv [K, n], ret [K, n] and /
    or moments [P, 2] (float64) are written where given.  workspace: a tensor of at least t1d_gae_workspace bytes (default:
    the cached one of this shape)."""
    L = _lib.lib()
    K, n = reward.shape
    dt = _T1D_DTYPE[reward.dtype]
    io = _lib.GaeBatch()
    io.n_rows, io.n_policies, io.gamma, io.lam = K, int(n_policies), float(gamma), float(lam)
    io.reward = reward.data_ptr()
    for name, t in (("done", done), ("value", value), ("last_value", last_value), ("adv", adv), ("ret", ret)):
        setattr(io, name, t.data_ptr() if t is not None else None)
    if moments is not None:
        io.moments = moments.data_ptr()
        if workspace is None:
            need = L.t1d_gae_workspace(dt, n, C.byref(io))
            if need < 0:
                _lib.check(int(need))
            key = (str(reward.device), need)
            if key not in _workspaces:
                _workspaces[key] = torch.empty(need, dtype=torch.uint8, device=reward.device)
            workspace = _workspaces[key]
        io.workspace, io.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    with torch.cuda.device(reward.device):
        stream = C.c_void_p(torch.cuda.current_stream(reward.device).cuda_stream)
        if truncated is None:
            _lib.check(L.t1d_gae(reward.device.index, dt, n, C.byref(io), stream))
        else:
            cut = _lib.GaeCut()
            cut.truncated, cut.cut_value = truncated.data_ptr(), cut_value.data_ptr() if cut_value is not None else None
            _lib.check(L.t1d_gae_limit(reward.device.index, dt, n, C.byref(io), C.byref(cut), stream))


def gae(reward, done=None, value=None, last_value=None, gamma=0.99, lam=0.95, n_policies=1, moments=False, truncated=None,
        cut_value=None):
    """Generalised advantage estimation over a collected batch, one launch (t1d_gae, include/t1d.h).  reward [K, n] (float64
    or float32, contiguous, on the GPU: tr["reward"][1:]); done [K, n] uint8 or None (tr["done"][1:]); value [K, n] or
    None = 0: the critic on the state every step started from; last_value [n] or None = 0: the critic on the state after the
    last row.  -> (adv, ret), ret = adv + value the critic's regression target; with moments=True -> (adv, ret, mean [P],
    std [P]): the population mean and standard deviation of the advantages of each of the n_policies blocks of n /
    n_policies envs, in float64, formed from two sums whose order is fixed by the shapes -- normalising with them keeps a
    gradient reproducible.  A value behind a done is never read into the row before it: with on_done="restart" row s + 1
    of a trace belongs to the next episode of an env that finished in row s.  truncated [K, n] uint8 or None
    (tr["truncated"][1:] of collect_mlp_limit): rows cut by the time limit (t1d_gae_limit); cut_value [n] or
    None = 0: the critic on the state the cut episode ended in (cut_features).  A truncated row that is not done bootstraps
    from cut_value instead of value[s + 1] and takes no advantage from the row after it; both are selected, so neither a
    value behind a cut nor the cut_value of an env that was not cut reaches a row it does not belong to.  None is the call
    without a second mask.  Raises ValueError for non-contiguous input, a wrong dtype, device or shape.

        v = mlp_pre_output(vparams, tr["features"][1:], vpol)                                   # [K, n], the critic
        v_last = mlp_pre_output(vparams, env.policy_features(vpol, state)[None], vpol)[0]       # the bootstrap at the cut
        adv, ret, mean, std = gae(tr["reward"][1:], tr["done"][1:], v.detach(), v_last.detach(), moments=True)
    """
    _check(reward, done, value, last_value, gamma, lam, n_policies, truncated, cut_value)
    adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    if not moments:
        gae_call(reward, done, value, last_value, gamma, lam, n_policies, adv=adv, ret=ret, truncated=truncated, cut_value=cut_value)
        return adv, ret
    P = int(n_policies)
    sums = torch.empty(P, 2, dtype=torch.float64, device=reward.device)
    gae_call(reward, done, value, last_value, gamma, lam, n_policies, adv=adv, ret=ret, moments=sums, truncated=truncated,
             cut_value=cut_value)
    count = reward.shape[0] * (reward.shape[1] // P)
    mean = sums[:, 0] / count
    std = (sums[:, 1] / count - mean * mean).clamp_min(0.0).sqrt()
    return adv, ret, mean, std


def gae_reference(reward, done=None, value=None, last_value=None, gamma=0.99, lam=0.95, n_policies=1, moments=False,
                  truncated=None, cut_value=None):
    """t1d_gae's recurrence (t1d_gae_limit's with truncated) as a plain torch loop in float64, on any device: -> (adv, ret,
    scale), all [K, n] float64.
    scale[s] = |reward[s]| + g |vn| + |value[s]| + g lam scale[s+1] live bounds the partial results of row s: the magnitude
    the rounding error of a float32 / float64 evaluation is stated in.  n_policies and moments are accepted and unused."""
    r = reward.to(torch.float64)
    K, n = r.shape
    v = value.to(torch.float64) if value is not None else torch.zeros_like(r)
    vn = last_value.to(torch.float64) if last_value is not None else torch.zeros(n, dtype=torch.float64, device=r.device)
    g, gl = float(gamma), float(gamma) * float(lam)
    adv, scale = torch.empty_like(r), torch.empty_like(r)
    an = torch.zeros_like(vn)
    sn = torch.zeros_like(vn)
    zero = torch.zeros_like(vn)
    cv = cut_value.to(torch.float64) if cut_value is not None else zero
    for s in range(K - 1, -1, -1):
        live = done[s] == 0 if done is not None else torch.ones(n, dtype=torch.bool, device=r.device)
        vn = torch.where(live, vn, zero)
        an = torch.where(live, an, zero)
        sn = torch.where(live, sn, zero)
        if truncated is not None:                           # done wins; a cut row bootstraps from cut_value and ends the sum
            trunc = live & (truncated[s] != 0)
            vn = torch.where(trunc, cv, vn)
            an = torch.where(trunc, zero, an)
            sn = torch.where(trunc, zero, sn)
        an = r[s] + g * vn - v[s] + gl * an
        sn = r[s].abs() + g * vn.abs() + v[s].abs() + gl * sn
        adv[s], scale[s] = an, sn
        vn = v[s]
    return adv, adv + v, scale
