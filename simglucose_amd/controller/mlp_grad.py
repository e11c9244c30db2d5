"""The in-kernel policy network as a differentiable torch op on the device: ``mlp_pre_output`` (t1d_mlp_grad in
``include/t1d.h``, ``csrc/t1d_policy_grad.hpp``).  The forward pass is the device code the roll-outs and collectors run,
so it gives the word they acted on; the backward pass recomputes the activations in LDS and keeps none of them."""
import ctypes as C

import torch

from .. import _lib

_T1D_DTYPE = {torch.float64: _lib.T1D_F64, torch.float32: _lib.T1D_F32}
_workspaces = {}                          # (device, dtype, bytes) -> tensor: one per shape, reused by every call


def _struct(policy, params, n):
    """the t1d_mlp of `policy` with the weights `params` for n envs: the network's fields only"""
    p = _lib.Mlp()
    policy.fill_struct(p)
    p.n_policies, p.envs_per_policy, p.n_params = params.shape[0], n // params.shape[0], params.shape[1]
    p.params = params.data_ptr()
    return p


def _check(params, features, policy):
    if not isinstance(params, torch.Tensor) or not isinstance(features, torch.Tensor):
        raise ValueError("mlp_pre_output: params and features must be tensors")
    if features.dtype not in _T1D_DTYPE or params.dtype != features.dtype:
        raise ValueError("mlp_pre_output: params and features must both be float64 or both float32")
    if features.device.type != "cuda" or params.device != features.device:
        raise ValueError("mlp_pre_output: params and features must be on the same GPU")
    if features.dim() != 3 or features.shape[0] < 1 or features.shape[1] != policy.n_features:
        raise ValueError("mlp_pre_output: features must be [K >= 1, %d, n]" % policy.n_features)
    n_params = policy.count_params(policy.history, policy.widths)
    if tuple(params.shape) != (policy.n_policies, n_params):
        raise ValueError("mlp_pre_output: params must be [%d, %d]" % (policy.n_policies, n_params))
    if not features.is_contiguous() or not params.is_contiguous():
        raise ValueError("mlp_pre_output: params and features must be contiguous")
    n = features.shape[2]
    if n % policy.n_policies or (n // policy.n_policies) % 64:
        raise ValueError("mlp_pre_output: %d envs do not split into %d policies of a multiple of 64 envs each" % (n, policy.n_policies))


def check_tiles(who, tiles, features, P):
    """the `tiles` of a listed call -> the int32 [P, M] tensor itself ([M] is taken as [1, M] when P == 1)"""
    if not isinstance(tiles, torch.Tensor) or tiles.dtype != torch.int32:
        raise ValueError("%s: tiles must be an int32 tensor" % who)
    if tiles.dim() == 1 and P == 1:
        tiles = tiles.unsqueeze(0)
    if tiles.dim() != 2 or tiles.shape[0] != P or tiles.shape[1] < 1:
        raise ValueError("%s: tiles must be [%d, M >= 1]" % (who, P))
    if not tiles.is_contiguous():
        raise ValueError("%s: tiles must be contiguous" % who)
    if tiles.device.type != "cuda" or tiles.device != getattr(features, "device", None):
        raise ValueError("%s: tiles must be on the features' device, a GPU" % who)
    return tiles


def tile_list(tiles):
    """the t1d_tile_list of a checked [P, M] tensor"""
    tl = _lib.TileList()
    tl.n_tiles, tl.tiles = tiles.shape[1], tiles.data_ptr()
    return tl


def mlp_grad_call(policy, params, features, coef=None, y=None, grad=None, workspace=None, tiles=None):
    """One t1d_mlp_grad call on the current stream of the features' device.  y [K, n] and / or grad [P, n_params] are
    written where given; grad needs coef [K, n].  workspace: a tensor of at least t1d_mlp_grad_workspace bytes (default:
    the cached one of this shape).  tiles (int32 [P, M] on the device, or [M] with P == 1): t1d_mlp_grad_tiles on the
    listed 64-env tiles u = row * C + chunk of every policy instead; y is then written at those tiles alone."""
    L = _lib.lib()
    K, _, n = features.shape
    p = _struct(policy, params, n)
    dt = _T1D_DTYPE[features.dtype]
    if tiles is not None:
        tiles = check_tiles("mlp_grad_call", tiles, features, params.shape[0])
    io = _lib.MlpBatch()
    io.n_rows, io.feat = K, features.data_ptr()
    io.coef = coef.data_ptr() if coef is not None else None
    io.y = y.data_ptr() if y is not None else None
    if grad is not None:
        io.grad = grad.data_ptr()
        if workspace is None:
            need = L.t1d_mlp_grad_workspace(C.byref(p), dt, n, K) if tiles is None else \
                L.t1d_mlp_grad_tiles_workspace(C.byref(p), dt, n, tiles.shape[1])
            if need < 0:
                _lib.check(int(need))
            key = (str(features.device), features.dtype, need)
            if key not in _workspaces:
                _workspaces[key] = torch.empty(need, dtype=torch.uint8, device=features.device)
            workspace = _workspaces[key]
        io.workspace, io.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    with torch.cuda.device(features.device):
        stream = C.c_void_p(torch.cuda.current_stream(features.device).cuda_stream)
        if tiles is None:
            _lib.check(L.t1d_mlp_grad(features.device.index, dt, n, C.byref(p), C.byref(io), stream))
        else:
            _lib.check(L.t1d_mlp_grad_tiles(features.device.index, dt, n, C.byref(p), C.byref(io), C.byref(tile_list(tiles)), stream))


class _PreOutput(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, features, policy):
        _check(params, features, policy)
        params, features = params.detach(), features.detach()
        y = torch.empty(features.shape[0], features.shape[2], dtype=features.dtype, device=features.device)
        mlp_grad_call(policy, params, features, y=y)
        ctx.save_for_backward(params, features)
        ctx.policy = policy
        return y

    @staticmethod
    def backward(ctx, grad_y):
        params, features = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None
        grad = torch.empty_like(params)
        mlp_grad_call(ctx.policy, params, features, coef=grad_y.contiguous(), grad=grad)
        return grad, None, None


def mlp_pre_output(params, features, policy):
    """y [K, n] = the pre-output value of `policy`'s network (an MLPController: its history, widths and hidden activation
    are used, not its weights) under the weights params [P, n_params] (flat_params() layout, on the device, may require
    grad) on features [K, F, n] as collect_mlp records them (contiguous, same device and dtype, fp64 or fp32; pass
    tr["features"][1:], row 0 of a trace is NaN).  Differentiable in params; the features get no gradient.  Forward and
    backward are one t1d_mlp_grad call each: y is the word the collector added sigma * eps to, bit for bit, and the
    backward pass recomputes the activations instead of storing them; its summation order is fixed by the shapes
    (include/t1d.h), so a gradient is reproducible.  Raises ValueError for non-contiguous input, a wrong dtype or device.

        pol = MLPController.from_torch(net, history=4)
        params = pol.device_params(env.device, env.dtype).clone().requires_grad_(True)
        opt = torch.optim.Adam([params], lr=3e-4)
        y = mlp_pre_output(params, tr["features"][1:], pol)
        loss(y).backward(); opt.step()
        pol = MLPController.from_flat(params, pol.widths, history=pol.history, hidden=pol.hidden, output=pol.output,
                                      out_scale=pol.out_scale, out_bias=pol.out_bias)      # back into the roll-outs
    """
    return _PreOutput.apply(params, features, policy)
