"""CPU suite: t1d_gae and t1d_mlp_features without a GPU -- the exports, the struct mirror, the workspace size, every
argument check of t1d_gae (validation comes before any HIP call), and known answers of the host restatement gae_reference."""
import ctypes as C

import pytest
import torch


def test_symbols_are_exported():
    from simglucose_amd import _lib
    L = _lib.lib()
    for name in ("t1d_mlp_features", "t1d_gae_workspace", "t1d_gae"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.t1d_abi_version() == 4 == _lib.ABI_VERSION


def test_gae_batch_struct_layout():
    """t1d_gae_batch of include/t1d.h, written out by hand: thirteen 8-byte fields."""
    from simglucose_amd import _lib
    want = [("n_rows", 0), ("n_policies", 8), ("gamma", 16), ("lam", 24), ("reward", 32), ("done", 40), ("value", 48),
            ("last_value", 56), ("adv", 64), ("ret", 72), ("moments", 80), ("workspace", 88), ("workspace_bytes", 96)]
    assert [f[0] for f in _lib.GaeBatch._fields_] == [w[0] for w in want]
    for name, off in want:
        assert getattr(_lib.GaeBatch, name).offset == off and getattr(_lib.GaeBatch, name).size == 8, name
    assert C.sizeof(_lib.GaeBatch) == 104


def _io(n_rows=3, n_policies=1, gamma=0.99, lam=0.95, reward=0x1000, done=0x2000, value=0x3000, last_value=0x4000, adv=0x5000,
        ret=0x6000, moments=0x7000, workspace=0x8000, workspace_bytes=1 << 30):
    from simglucose_amd import _lib
    b = _lib.GaeBatch()
    b.n_rows, b.n_policies, b.gamma, b.lam = n_rows, n_policies, gamma, lam
    b.reward, b.done, b.value, b.last_value, b.adv, b.ret, b.moments = reward, done, value, last_value, adv, ret, moments
    b.workspace, b.workspace_bytes = workspace, workspace_bytes
    return b


def test_workspace_size():
    from simglucose_amd import _lib
    L = _lib.lib()

    def ws(n, P, K=3, dtype=_lib.T1D_F64):
        return L.t1d_gae_workspace(dtype, n, C.byref(_io(n_rows=K, n_policies=P)))

    # 16 bytes for every tile: the 64-env pieces of a policy, counted from the policy's first env
    assert ws(64, 1) == 16 and ws(65, 1) == 32 and ws(100, 1) == 32
    assert ws(100, 4) == 16 * 4 and ws(192, 3) == 16 * 3 and ws(256, 8) == 16 * 8 and ws(4, 4) == 16 * 4
    assert ws(300, 1) == 16 * 5 and ws(300, 2) == 16 * 2 * 3 and ws(1 << 20, 16) == 16 * (1 << 14)
    for n, P in ((64, 1), (100, 4), (192, 3), (300, 1), (300, 12), (1 << 20, 1), (1 << 20, 16)):
        assert ws(n, P, dtype=_lib.T1D_F32) == ws(n, P) > 0            # the sums are double whatever the dtype
        sizes = [ws(n, P, K=K) for K in (1, 2, 5, 33, 1000)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes)    # monotone in n_rows (it does not grow with it)
    assert ws(64, 1, K=0) == -1 and ws(0, 1) == -1 and ws(100, 3) == -1 and ws(64, 1, dtype=7) == -1
    assert L.t1d_gae_workspace(_lib.T1D_F64, 64, None) == -1


def test_every_invalid_argument_is_rejected_without_a_gpu():
    """-1 (T1D_E_INVALID) whether or not a device is present: nothing is launched, the device is not touched."""
    from simglucose_amd import _lib
    L = _lib.lib()
    F64 = _lib.T1D_F64

    def call(b, n=128, dtype=F64):
        rc = L.t1d_gae(0, dtype, n, C.byref(b) if b is not None else None, None)
        if rc == -1:
            assert L.t1d_last_error().startswith(b"t1d_gae:"), L.t1d_last_error()
        return rc

    assert call(None) == -1 and b"io is NULL" in L.t1d_last_error()
    assert call(_io(reward=None)) == -1 and b"reward" in L.t1d_last_error()
    assert call(_io(adv=None, ret=None, moments=None)) == -1 and b"all NULL" in L.t1d_last_error()
    assert call(_io(n_rows=0)) == -1 and b"n_rows" in L.t1d_last_error()
    assert call(_io(n_rows=-1)) == -1
    assert call(_io(), n=0) == -1 and b"n out of range" in L.t1d_last_error()
    assert call(_io(), n=-64) == -1
    assert call(_io(n_policies=3)) == -1 and b"n_policies" in L.t1d_last_error()
    assert call(_io(n_policies=0)) == -1 and b"n_policies" in L.t1d_last_error()
    assert call(_io(n_policies=-1)) == -1
    # beyond the sizes the kernels index
    assert call(_io(), n=(1 << 31) + 64) == -1 and b"n out of range" in L.t1d_last_error()
    assert call(_io(n_policies=1 << 31), n=1 << 31) == -1 and b"n_policies" in L.t1d_last_error()
    assert call(_io(n_rows=(1 << 40) // 128 + 1)) == -1 and b"n_rows" in L.t1d_last_error()
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        assert call(_io(gamma=bad)) == -1 and b"gamma" in L.t1d_last_error()
        assert call(_io(lam=bad)) == -1 and b"lambda" in L.t1d_last_error()
    assert call(_io(), dtype=2) == -1 and b"dtype" in L.t1d_last_error()
    assert call(_io(), dtype=-1) == -1
    assert call(_io(workspace=None)) == -1 and b"workspace" in L.t1d_last_error()
    need = L.t1d_gae_workspace(F64, 128, C.byref(_io()))
    assert need == 32                                                 # 128 envs of one policy: two tiles
    assert call(_io(workspace_bytes=need - 1)) == -1 and b"workspace" in L.t1d_last_error()
    assert call(_io(workspace_bytes=0)) == -1


def test_wrapper_rejects_before_the_device():
    from simglucose_amd.controller import gae
    with pytest.raises(ValueError):
        gae(torch.zeros(3, 64, dtype=torch.float64))                  # not on a GPU
    with pytest.raises(ValueError):
        gae(torch.zeros(3, 64, dtype=torch.float16))
    with pytest.raises(ValueError):
        gae([[0.0]])


R = torch.tensor([[1.0], [2.0], [3.0]], dtype=torch.float64)
V = torch.tensor([[0.5], [1.0], [2.0]], dtype=torch.float64)
V_LAST = torch.tensor([4.0], dtype=torch.float64)


def test_reference_known_answers_by_hand():
    """K = 3, one env, gamma = lambda = 0.5 (g = 0.5, g lambda = 0.25), r = 1, 2, 3, V = 0.5, 1, 2 and 4 after the last row.
    row 2: delta = 3 + 0.5 * 4 - 2 = 3,   adv = 3
    row 1: delta = 2 + 0.5 * 2 - 1 = 2,   adv = 2 + 0.25 * 3 = 2.75
    row 0: delta = 1 + 0.5 * 1 - 0.5 = 1, adv = 1 + 0.25 * 2.75 = 1.6875
    with done in row 1: row 1: delta = 2 - 1 = 1, adv = 1; row 0: adv = 1 + 0.25 * 1 = 1.25.  Every number is exact in binary."""
    from simglucose_amd.controller import gae_reference
    adv, ret, scale = gae_reference(R, None, V, V_LAST, gamma=0.5, lam=0.5)
    assert adv.dtype == torch.float64 and adv.shape == ret.shape == scale.shape == (3, 1)
    assert adv[:, 0].tolist() == [1.6875, 2.75, 3.0]
    assert ret[:, 0].tolist() == [2.1875, 3.75, 5.0]
    assert scale[:, 0].tolist() == [3.4375, 5.75, 7.0]                # 3 + 2 + 2; 2 + 1 + 1 + 0.25 * 7; 1 + 0.5 + 0.5 + 0.25 * 5.75
    done = torch.tensor([[0], [1], [0]], dtype=torch.uint8)
    adv, ret, scale = gae_reference(R, done, V, V_LAST, gamma=0.5, lam=0.5)
    assert adv[:, 0].tolist() == [1.25, 1.0, 3.0]
    assert ret[:, 0].tolist() == [1.75, 2.0, 5.0]
    assert scale[:, 0].tolist() == [2.75, 3.0, 7.0]
    # what stands behind a done is selected away, not multiplied by zero
    v_nan = V.clone(); v_nan[2] = float("nan")
    adv2, ret2, _ = gae_reference(R, done, v_nan, V_LAST, gamma=0.5, lam=0.5)
    assert adv2[:2, 0].tolist() == [1.25, 1.0] and ret2[:2, 0].tolist() == [1.75, 2.0]
    last = torch.tensor([[0], [0], [1]], dtype=torch.uint8)
    adv3, _, _ = gae_reference(R, last, V, torch.tensor([float("nan")], dtype=torch.float64), gamma=0.5, lam=0.5)
    assert adv3[:, 0].tolist() == [1 + 0.25 * (2 + 0.25 * 1), 2 + 0.25 * 1, 1.0]
    # float32 input is taken to double
    adv4, _, _ = gae_reference(R.float(), done, V.float(), V_LAST.float(), gamma=0.5, lam=0.5)
    assert adv4.dtype == torch.float64 and adv4[:, 0].tolist() == [1.25, 1.0, 3.0]


def test_reference_lambda_one_is_the_discounted_return_to_go():
    from simglucose_amd.controller import gae_reference
    g = torch.Generator().manual_seed(5)
    r = torch.randn(6, 7, generator=g, dtype=torch.float64)
    adv, ret, _ = gae_reference(r, None, None, None, gamma=0.5, lam=1.0)
    want = torch.zeros_like(r)
    run = torch.zeros(7, dtype=torch.float64)
    for s in range(5, -1, -1):
        run = r[s] + 0.5 * run
        want[s] = run
    assert torch.equal(adv, want) and torch.equal(ret, want)
    # with dones the sum stops at the end of the episode
    done = (torch.rand(6, 7, generator=g) < 0.3).to(torch.uint8)
    adv, _, _ = gae_reference(r, done, None, None, gamma=0.5, lam=1.0)
    run = torch.zeros(7, dtype=torch.float64)
    for s in range(5, -1, -1):
        run = r[s] + 0.5 * run * (done[s] == 0)
        assert torch.equal(adv[s], run)


def test_reference_lambda_zero_is_the_one_step_td_error():
    from simglucose_amd.controller import gae_reference
    g = torch.Generator().manual_seed(6)
    r = torch.randn(5, 9, generator=g, dtype=torch.float64)
    v = torch.randn(5, 9, generator=g, dtype=torch.float64)
    v_last = torch.randn(9, generator=g, dtype=torch.float64)
    done = (torch.rand(5, 9, generator=g) < 0.3).to(torch.uint8)
    adv, ret, _ = gae_reference(r, done, v, v_last, gamma=0.9, lam=0.0)
    v_next = torch.cat([v[1:], v_last[None]])
    assert torch.equal(adv, r + 0.9 * v_next * (done == 0) - v)
    assert torch.equal(ret, adv + v)
