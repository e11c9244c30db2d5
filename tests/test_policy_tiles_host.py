"""CPU suite: the listed calls t1d_mlp_grad_tiles / t1d_mlp_loss_tiles without a GPU -- the exports, the ctypes mirror of
t1d_tile_list, the workspace sizes against the header's formulas, every argument check (validation comes before any HIP
call), the Python checks of tiles=, tile_minibatches and gather_tiles."""
import ctypes as C
import os
import re

import pytest
import torch

from support import header_fields, identity_policy as _policy, mlp_struct as _mlp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t1d_mlp_grad_tiles_workspace", "t1d_mlp_grad_tiles", "t1d_mlp_loss_tiles_workspace", "t1d_mlp_loss_tiles")


# ------------------------------------------------------------------------------------------------ exports, structs
def test_symbols_are_declared_bound_and_exported():
    from simglucose_amd import _lib
    L = _lib.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "t1d.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    assert L.t1d_mlp_grad_tiles_workspace.restype is C.c_int64 and L.t1d_mlp_loss_tiles_workspace.restype is C.c_int64
    assert L.t1d_abi_version() == _lib.ABI_VERSION == 4
    assert "#define T1D_ABI_VERSION 4" in src


def test_tile_list_mirror_matches_header():
    from simglucose_amd import _lib
    fields = header_fields("t1d_tile_list")
    assert [(f[0], f[2]) for f in fields] == [("n_tiles", False), ("tiles", True)]
    assert fields[0][1] == "int64_t" and fields[1][1] == "int32_t"
    assert [f[0] for f in _lib.TileList._fields_] == ["n_tiles", "tiles"]
    assert C.sizeof(_lib.TileList) == 16 and _lib.TileList.tiles.offset == 8


def test_existing_structs_are_unchanged():
    from simglucose_amd import _lib
    assert [f[0] for f in header_fields("t1d_mlp_batch")] == ["n_rows", "feat", "coef", "y", "grad", "workspace", "workspace_bytes"]
    assert [f[0] for f in _lib.MlpBatch._fields_] == [f[0] for f in header_fields("t1d_mlp_batch")]
    assert C.sizeof(_lib.MlpBatch) == 56
    assert [f[0] for f in _lib.MlpLoss._fields_] == ["n_rows", "kind", "reserved", "feat", "eps", "y_old", "adv", "sigma_old", "sigma", "target",
                                                     "clip", "scale", "y", "coef_out", "grad", "stats", "workspace", "workspace_bytes"]
    assert C.sizeof(_lib.MlpLoss) == 136


# ------------------------------------------------------------------------------------------------ workspace
# P, M, widths, history; the third row has P * M = 4400 > 2048 (T = 3), the fourth P * M = 2049 (T = 2, an odd M)
WORKSPACE_ROWS = [(2, 6, (8, 8, 1), 4), (1, 1, (1,), 4), (2, 2200, (5, 1), 2), (1, 2049, (8, 8, 1), 4), (2, 1024, (32, 32, 32, 1), 12),
                  (2, 100000, (8, 8, 1), 4)]


@pytest.mark.parametrize("P,M,widths,history", WORKSPACE_ROWS)
def test_workspace_sizes_are_the_headers_formulas(P, M, widths, history):
    from simglucose_amd import _lib
    L = _lib.lib()
    for dtype, word in ((_lib.T1D_F64, 8), (_lib.T1D_F32, 4)):
        for E in (64, 192):                                            # the size does not depend on C
            p = _mlp(widths=widths, history=history, n_policies=P, envs_per_policy=E)
            T = max(1, -(-P * M // 2048))
            partials = P * -(-M // T)
            W = L.t1d_mlp_grad_tiles_workspace(C.byref(p), dtype, P * E, M)
            assert W == partials * p.n_params * word
            assert L.t1d_mlp_loss_tiles_workspace(C.byref(p), dtype, P * E, M) == (W + 7) // 8 * 8 + 32 * partials
    # M = C * n_rows: the plain call's size
    p = _mlp(widths=widths, history=history, n_policies=P, envs_per_policy=128)
    if M % 2 == 0:
        assert L.t1d_mlp_grad_tiles_workspace(C.byref(p), _lib.T1D_F64, 128 * P, M) == L.t1d_mlp_grad_workspace(C.byref(p), _lib.T1D_F64, 128 * P, M // 2)
        assert L.t1d_mlp_loss_tiles_workspace(C.byref(p), _lib.T1D_F32, 128 * P, M) == L.t1d_mlp_loss_workspace(C.byref(p), _lib.T1D_F32, 128 * P, M // 2)


def test_workspace_rejects_bad_arguments():
    from simglucose_amd import _lib
    L = _lib.lib()
    F64 = _lib.T1D_F64
    for name in ("t1d_mlp_grad_tiles_workspace", "t1d_mlp_loss_tiles_workspace"):
        f = getattr(L, name)
        for M in (0, -1, -(1 << 40)):
            assert f(C.byref(_mlp()), F64, 128, M) < 0 and b"n_tiles" in L.t1d_last_error() and name.encode() in L.t1d_last_error()
        assert f(C.byref(_mlp()), F64, 128, (1 << 30)) < 0 and b"n_tiles" in L.t1d_last_error()       # 2 policies: 2^31 positions
        assert f(C.byref(_mlp(n_policies=1, envs_per_policy=128)), F64, 128, (1 << 31) - 1) > 0
        assert f(C.byref(_mlp()), F64, 128, 1 << 62) < 0
        assert f(C.byref(_mlp(widths=(33, 1))), F64, 128, 6) < 0
        assert f(C.byref(_mlp()), 7, 128, 6) < 0
        assert f(C.byref(_mlp()), F64, 192, 6) < 0
        assert f(None, F64, 128, 6) < 0
        p = _mlp(); p.params = None                                      # the weights are not needed for the size
        assert f(C.byref(p), F64, 128, 6) > 0


# ------------------------------------------------------------------------------------------------ argument checks
def _list(n_tiles=6, tiles=0xe000):
    from simglucose_amd import _lib
    tl = _lib.TileList()
    tl.n_tiles, tl.tiles = n_tiles, tiles
    return tl


def _loss_io(kind=1, **kw):
    from simglucose_amd import _lib
    b = _lib.MlpLoss()
    d = dict(n_rows=3, feat=0x2000, eps=0x3000, y_old=0x4000, adv=0x5000, sigma_old=0x6000, sigma=0x7000, target=0x8000,
             clip=0.2, scale=1.0 / 384, y=0x9000, coef_out=0xa000, grad=0xb000, stats=0xc000, workspace=0xd000, workspace_bytes=1 << 30)
    d.update(kw)
    b.kind = kind
    for k, v in d.items():
        setattr(b, k, v)
    return b


def _grad_io(**kw):
    from simglucose_amd import _lib
    b = _lib.MlpBatch()
    d = dict(n_rows=3, feat=0x2000, coef=0x3000, y=0x4000, grad=0x5000, workspace=0x6000, workspace_bytes=1 << 30)
    d.update(kw)
    for k, v in d.items():
        setattr(b, k, v)
    return b


def _ref(x):
    return C.byref(x) if x is not None else None


def test_loss_tiles_rejects_every_invalid_argument_without_a_gpu():
    """-1 (T1D_E_INVALID) whether or not a device is present, the text naming t1d_mlp_loss_tiles"""
    from simglucose_amd import _lib
    L = _lib.lib()
    F64, PPO, MSE = _lib.T1D_F64, _lib.T1D_LOSS_PPO_CLIP, _lib.T1D_LOSS_VALUE_MSE
    io = _loss_io

    def bad(p, b, tl, word, n=128, dtype=F64):
        rc = L.t1d_mlp_loss_tiles(0, dtype, n, _ref(p), _ref(b), _ref(tl), None)
        err = L.t1d_last_error()
        assert rc == -1 and b"t1d_mlp_loss_tiles" in err and word in err, (rc, err, word)

    ok = _mlp()
    # everything the plain call rejects
    bad(_mlp(history=0), io(), _list(), b"history")
    bad(_mlp(history=13), io(), _list(), b"")
    bad(_mlp(widths=(33, 1)), io(), _list(), b"width")
    bad(_mlp(widths=(8, 2)), io(), _list(), b"last layer")
    p = _mlp(); p.n_layers = 5
    bad(p, io(), _list(), b"")
    p = _mlp(); p.n_params += 1
    bad(p, io(), _list(), b"n_params")
    p = _mlp(); p.hidden_act = 2
    bad(p, io(), _list(), b"hidden_act")
    bad(_mlp(params=None), io(), _list(), b"params")
    bad(_mlp(n_policies=0), io(), _list(), b"")
    bad(None, io(), _list(), b"")
    bad(ok, None, _list(), b"io")
    bad(ok, io(), _list(), b"dtype", dtype=5)
    bad(ok, io(), _list(), b"n_policies * envs_per_policy", n=192)
    bad(_mlp(envs_per_policy=96), io(), _list(), b"multiple of 64", n=192)
    bad(ok, io(n_rows=0), _list(), b"n_rows")
    bad(ok, io(feat=None), _list(), b"feat")
    for kind in (0, 3, -1):
        bad(ok, io(kind=kind), _list(), b"kind")
    for name in ("eps", "y_old", "adv", "sigma_old", "sigma"):
        bad(ok, io(**{name: None}), _list(), b"T1D_LOSS_PPO_CLIP needs")
    bad(ok, io(kind=MSE, target=None), _list(), b"target")
    for clip in (0.0, 1.0, -0.2, 1.5, float("nan"), float("inf")):
        bad(ok, io(clip=clip), _list(), b"clip")
    for scale in (float("nan"), float("inf"), float("-inf")):
        bad(ok, io(scale=scale), _list(), b"scale")
        bad(ok, io(kind=MSE, scale=scale), _list(), b"scale")
    bad(ok, io(y=None, coef_out=None, grad=None, stats=None), _list(), b"all NULL")
    # the list
    bad(ok, io(), None, b"list")
    bad(ok, io(), _list(tiles=None), b"tiles is NULL")
    for M in (0, -1):
        bad(ok, io(), _list(n_tiles=M), b"n_tiles < 1")
    bad(ok, io(), _list(n_tiles=1 << 30), b"n_tiles is too large")        # 2 policies x 2^30 positions
    bad(ok, io(), _list(n_tiles=1 << 62), b"n_tiles is too large")
    # the workspace of THIS call: sized by n_tiles, not by n_rows
    for M in (6, 3000):
        need = L.t1d_mlp_loss_tiles_workspace(C.byref(ok), F64, 128, M)
        assert need > 0
        for kind in (PPO, MSE):
            for out in (dict(stats=None), dict(grad=None), dict()):
                bad(ok, io(kind=kind, workspace=None, **out), _list(n_tiles=M), b"t1d_mlp_loss_tiles_workspace")
                bad(ok, io(kind=kind, workspace_bytes=need - 1, **out), _list(n_tiles=M), b"t1d_mlp_loss_tiles_workspace")
    # a workspace that would do for the plain call of these rows (3 tiles per policy) is too small for 3000 positions
    plain = L.t1d_mlp_loss_workspace(C.byref(ok), F64, 128, 3)
    assert plain < L.t1d_mlp_loss_tiles_workspace(C.byref(ok), F64, 128, 3000)
    bad(ok, io(workspace_bytes=plain), _list(n_tiles=3000), b"workspace")


def test_grad_tiles_rejects_every_invalid_argument_without_a_gpu():
    from simglucose_amd import _lib
    L = _lib.lib()
    F64 = _lib.T1D_F64
    io = _grad_io

    def bad(p, b, tl, word, n=128, dtype=F64):
        rc = L.t1d_mlp_grad_tiles(0, dtype, n, _ref(p), _ref(b), _ref(tl), None)
        err = L.t1d_last_error()
        assert rc == -1 and b"t1d_mlp_grad_tiles" in err and word in err, (rc, err, word)

    ok = _mlp()
    bad(_mlp(history=0), io(), _list(), b"history")
    bad(_mlp(widths=(33, 1)), io(), _list(), b"width")
    bad(_mlp(widths=(8, 2)), io(), _list(), b"last layer")
    p = _mlp(); p.n_params += 1
    bad(p, io(), _list(), b"n_params")
    bad(_mlp(params=None), io(), _list(), b"params")
    bad(_mlp(n_policies=0), io(), _list(), b"")
    bad(None, io(), _list(), b"")
    bad(ok, None, _list(), b"io")
    bad(ok, io(), _list(), b"dtype", dtype=5)
    bad(ok, io(), _list(), b"n_policies * envs_per_policy", n=192)
    bad(_mlp(envs_per_policy=96), io(), _list(), b"multiple of 64", n=192)
    bad(ok, io(n_rows=0), _list(), b"n_rows")
    bad(ok, io(feat=None), _list(), b"feat")
    bad(ok, io(y=None, grad=None), _list(), b"both NULL")
    bad(ok, io(coef=None), _list(), b"coef")
    bad(ok, io(), None, b"list")
    bad(ok, io(), _list(tiles=None), b"tiles is NULL")
    for M in (0, -1):
        bad(ok, io(), _list(n_tiles=M), b"n_tiles < 1")
    bad(ok, io(), _list(n_tiles=1 << 30), b"n_tiles is too large")
    for M in (6, 3000):
        need = L.t1d_mlp_grad_tiles_workspace(C.byref(ok), F64, 128, M)
        bad(ok, io(workspace=None), _list(n_tiles=M), b"t1d_mlp_grad_tiles_workspace")
        bad(ok, io(workspace_bytes=need - 1), _list(n_tiles=M), b"t1d_mlp_grad_tiles_workspace")


def test_plain_calls_keep_their_texts():
    """the plain entry points share the checks: their messages still name them"""
    from simglucose_amd import _lib
    L = _lib.lib()
    assert L.t1d_mlp_loss(0, _lib.T1D_F64, 128, C.byref(_mlp()), C.byref(_loss_io(workspace=None)), None) == -1
    assert L.t1d_last_error() == b"t1d_mlp_loss: grad and stats need a workspace of t1d_mlp_loss_workspace() bytes"
    assert L.t1d_mlp_grad(0, _lib.T1D_F64, 128, C.byref(_mlp()), C.byref(_grad_io(workspace=None)), None) == -1
    assert L.t1d_last_error() == b"t1d_mlp_grad: grad needs a workspace of t1d_mlp_grad_workspace() bytes"


# ------------------------------------------------------------------------------------------------ Python checks
def test_python_tiles_checks_raise_value_error():
    """each check of tiles= comes before the device is needed"""
    from simglucose_amd.controller import ppo_clip_loss, value_loss
    pol = _policy(4, (8, 8, 1), 2, hidden="tanh", seed=1)
    feat = torch.zeros(3, pol.n_features, 256, dtype=torch.float64)
    a = torch.zeros(3, 256, dtype=torch.float64)
    good = torch.zeros(2, 4, dtype=torch.int32)
    cases = [(good, "device"),                                          # a CPU tensor
             (good.long(), "int32"),
             (torch.zeros(3, 4, dtype=torch.int32), r"\[2, M"),           # a wrong P
             (torch.zeros(4, dtype=torch.int32), r"\[2, M"),              # [M] goes with P == 1 alone
             (torch.zeros(2, 0, dtype=torch.int32), r"\[2, M"),
             (torch.zeros(2, 8, dtype=torch.int32)[:, ::2], "contiguous"),
             ([0, 1, 2], "int32")]
    for tiles, word in cases:
        with pytest.raises(ValueError, match="ppo_clip_loss: tiles.*" + word):
            ppo_clip_loss(pol.flat_params(), feat, pol, a, a, a, 0.3, tiles=tiles)
        with pytest.raises(ValueError, match="value_loss: tiles.*" + word):
            value_loss(pol.flat_params(), feat, pol, a, tiles=tiles)


# ------------------------------------------------------------------------------------------------ tile_minibatches
@pytest.mark.parametrize("K,n,P,B", [(3, 256, 2, 3), (5, 384, 2, 4), (7, 64, 1, 2), (32, 1024, 4, 32), (3, 128, 1, 6)])
def test_tile_minibatches(K, n, P, B):
    from simglucose_amd.controller import tile_minibatches
    total = n // P // 64 * K
    M = total // B
    mbs = tile_minibatches(K, n, P, B, generator=torch.Generator().manual_seed(5))
    assert len(mbs) == B
    for mb in mbs:
        assert mb.dtype == torch.int32 and tuple(mb.shape) == (P, M) and mb.is_contiguous() and mb.device.type == "cpu"
        assert int(mb.min()) >= 0 and int(mb.max()) < total
    epoch = torch.cat(mbs, dim=1)
    for p in range(P):
        seen = torch.bincount(epoch[p].long(), minlength=total)
        assert int(seen.max()) == 1                                      # no id twice within the epoch
        assert int((seen == 0).sum()) == total % B                       # exactly the leftover is left out
    again = tile_minibatches(K, n, P, B, generator=torch.Generator().manual_seed(5))
    assert all(torch.equal(x, y) for x, y in zip(mbs, again))
    other = torch.cat(tile_minibatches(K, n, P, B, generator=torch.Generator().manual_seed(6)), dim=1)
    if total >= 6:
        assert not torch.equal(epoch, other)
        if P > 1:
            assert not torch.equal(epoch[0], epoch[1])                   # every policy its own permutation


def test_tile_minibatches_rejects():
    from simglucose_amd.controller import tile_minibatches
    with pytest.raises(ValueError):
        tile_minibatches(3, 128, 1, 7)                                   # 6 tiles, 7 minibatches: M == 0
    with pytest.raises(ValueError):
        tile_minibatches(3, 192, 2, 1)                                   # 96 envs per policy
    with pytest.raises(ValueError):
        tile_minibatches(3, 100, 1, 1)
    assert tile_minibatches(3, 128, 1, 6)[0].shape == (1, 1)


# ------------------------------------------------------------------------------------------------ gather_tiles
@pytest.mark.parametrize("P", [1, 2])
def test_gather_tiles_against_an_index_loop(P):
    from simglucose_amd.controller import gather_tiles
    K, Cn, F, M = 3, 2, 5, 7
    n = 64 * Cn * P
    g = torch.Generator().manual_seed(3)
    a2 = torch.randn(K, n, generator=g, dtype=torch.float64)
    a3 = torch.randn(K, F, n, generator=g, dtype=torch.float32)
    tiles = torch.randint(0, Cn * K, (P, M), generator=g, dtype=torch.int32)
    w2, w3 = torch.empty(M, 64 * P, dtype=a2.dtype), torch.empty(M, F, 64 * P, dtype=a3.dtype)
    for p in range(P):
        for j in range(M):
            u = int(tiles[p, j])
            row, chunk = u // Cn, u % Cn
            first = p * 64 * Cn + 64 * chunk
            for lane in range(64):
                w2[j, 64 * p + lane] = a2[row, first + lane]
                for f in range(F):
                    w3[j, f, 64 * p + lane] = a3[row, f, first + lane]
    g2, g3 = gather_tiles(a2, tiles, P), gather_tiles(a3, tiles, P)
    assert g2.is_contiguous() and g3.is_contiguous()
    assert torch.equal(g2, w2) and torch.equal(g3, w3)
    if P == 1:
        assert torch.equal(gather_tiles(a2, tiles[0], 1), w2)
        # the identity list is the batch itself, tile by tile
        ident = torch.arange(Cn * K, dtype=torch.int32)
        assert torch.equal(gather_tiles(a2, ident, 1).reshape(K, n), a2)
