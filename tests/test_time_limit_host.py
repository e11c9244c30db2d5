"""CPU suite: time-limited episodes without a GPU -- t1d_collect_mlp_limit and t1d_gae_limit are exported, the two struct
mirrors, every argument check of t1d_gae_limit (validation comes before any HIP call), known answers of gae_reference with a
truncation mask, and what collect_mlp_limit and new_trace refuse or build before anything is launched."""
import ctypes as C

import pytest
import torch


def test_symbols_are_exported():
    from simglucose_amd import _lib
    L = _lib.lib()
    for name in ("t1d_collect_mlp_limit", "t1d_gae_limit"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert L.t1d_abi_version() == 4 == _lib.ABI_VERSION


def test_struct_layouts():
    """t1d_time_limit and t1d_gae_cut of include/t1d.h, written out by hand: 4 + 4 + 8 + 8 = 24 bytes, and two pointers."""
    from simglucose_amd import _lib
    want = [("max_minutes", 0, 4), ("reserved", 4, 4), ("cut_trace", 8, 8), ("cut_feat", 16, 8)]
    assert [f[0] for f in _lib.TimeLimit._fields_] == [w[0] for w in want]
    for name, off, size in want:
        assert getattr(_lib.TimeLimit, name).offset == off and getattr(_lib.TimeLimit, name).size == size, name
    assert C.sizeof(_lib.TimeLimit) == 24
    want = [("truncated", 0, 8), ("cut_value", 8, 8)]
    assert [f[0] for f in _lib.GaeCut._fields_] == [w[0] for w in want]
    for name, off, size in want:
        assert getattr(_lib.GaeCut, name).offset == off and getattr(_lib.GaeCut, name).size == size, name
    assert C.sizeof(_lib.GaeCut) == 16


def _io(n_rows=3, n_policies=1, gamma=0.99, lam=0.95, reward=0x1000, done=0x2000, value=0x3000, last_value=0x4000, adv=0x5000,
        ret=0x6000, moments=0x7000, workspace=0x8000, workspace_bytes=1 << 30):
    from simglucose_amd import _lib
    b = _lib.GaeBatch()
    b.n_rows, b.n_policies, b.gamma, b.lam = n_rows, n_policies, gamma, lam
    b.reward, b.done, b.value, b.last_value, b.adv, b.ret, b.moments = reward, done, value, last_value, adv, ret, moments
    b.workspace, b.workspace_bytes = workspace, workspace_bytes
    return b


def _cut(truncated=0x9000, cut_value=0xA000):
    from simglucose_amd import _lib
    c = _lib.GaeCut()
    c.truncated, c.cut_value = truncated, cut_value
    return c


def test_every_invalid_argument_of_gae_limit_is_rejected_without_a_gpu():
    """-1 (T1D_E_INVALID) whether or not a device is present: nothing is launched, the device is not touched."""
    from simglucose_amd import _lib
    L = _lib.lib()
    F64 = _lib.T1D_F64

    def call(b, cut=_cut(), n=128, dtype=F64):
        rc = L.t1d_gae_limit(0, dtype, n, C.byref(b) if b is not None else None, C.byref(cut) if cut is not None else None, None)
        if rc == -1:
            assert L.t1d_last_error().startswith(b"t1d_gae_limit:"), L.t1d_last_error()
        return rc

    # the limit's own
    assert call(_io(), cut=None) == -1 and b"cut" in L.t1d_last_error()
    assert call(_io(), cut=_cut(truncated=None)) == -1 and b"truncated" in L.t1d_last_error()
    assert call(_io(), cut=_cut(truncated=None, cut_value=None)) == -1
    # t1d_gae's
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
    assert call(_io(), n=(1 << 31) + 64) == -1 and b"n out of range" in L.t1d_last_error()
    assert call(_io(n_policies=1 << 31), n=1 << 31) == -1 and b"n_policies" in L.t1d_last_error()
    assert call(_io(n_rows=(1 << 40) // 128 + 1)) == -1 and b"n_rows" in L.t1d_last_error()
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        assert call(_io(gamma=bad)) == -1 and b"gamma" in L.t1d_last_error()
        assert call(_io(lam=bad)) == -1 and b"lambda" in L.t1d_last_error()
    assert call(_io(), dtype=2) == -1 and b"dtype" in L.t1d_last_error()
    assert call(_io(), dtype=-1) == -1
    assert call(_io(workspace=None)) == -1 and b"workspace" in L.t1d_last_error()
    assert call(_io(workspace_bytes=31)) == -1 and b"workspace" in L.t1d_last_error()      # 128 envs of one policy: two tiles
    assert call(_io(workspace_bytes=0)) == -1


def test_wrapper_rejects_before_the_device():
    from simglucose_amd.controller import gae
    with pytest.raises(ValueError):
        gae(torch.zeros(3, 64, dtype=torch.float64), truncated=torch.zeros(3, 64, dtype=torch.uint8))     # not on a GPU


GAMMA = LAM = 0.5                                        # g = 0.5, g lambda = 0.25: every number below is exact in binary
R = torch.tensor([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0]], dtype=torch.float64)
V = torch.tensor([[0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [2.0, 2.0, 2.0]], dtype=torch.float64)
V_LAST = torch.tensor([4.0, 4.0, 4.0], dtype=torch.float64)
V_CUT = torch.tensor([8.0, float("nan"), 8.0], dtype=torch.float64)


def test_reference_known_answers_with_a_cut_in_the_middle_row():
    """3 rows x 3 envs, r = 1, 2, 3, V = 0.5, 1, 2 and 4 after the last row (tests/test_gae_host.py).  Row 2 is the same for
    all: delta = 3 + 0.5 * 4 - 2 = 3, adv = 3.
    env 0, cut in row 1 with cut_value 8: row 1: delta = 2 + 0.5 * 8 - 1 = 5, adv = 5 (nothing from row 2);
                                          row 0: delta = 1 + 0.5 * 1 - 0.5 = 1, adv = 1 + 0.25 * 5 = 2.25
    env 1, no cut, its cut_value NaN:     the uncut answers 1.6875, 2.75, 3
    env 2, done AND truncated in row 1:   done's answers: row 1: delta = 2 - 1 = 1, adv = 1; row 0: adv = 1 + 0.25 * 1 = 1.25"""
    from simglucose_amd.controller import gae_reference
    done = torch.tensor([[0, 0, 0], [0, 0, 1], [0, 0, 0]], dtype=torch.uint8)
    trunc = torch.tensor([[0, 0, 0], [1, 0, 1], [0, 0, 0]], dtype=torch.uint8)
    adv, ret, scale = gae_reference(R, done, V, V_LAST, gamma=GAMMA, lam=LAM, truncated=trunc, cut_value=V_CUT)
    assert adv.dtype == torch.float64 and adv.shape == ret.shape == scale.shape == (3, 3)
    assert adv[:, 0].tolist() == [2.25, 5.0, 3.0] and ret[:, 0].tolist() == [2.75, 6.0, 5.0]
    assert adv[:, 1].tolist() == [1.6875, 2.75, 3.0] and ret[:, 1].tolist() == [2.1875, 3.75, 5.0]
    assert adv[:, 2].tolist() == [1.25, 1.0, 3.0] and ret[:, 2].tolist() == [1.75, 2.0, 5.0]
    # scale: env 0 row 1: 2 + 0.5 * 8 + 1 = 7 (row 2's is cut off); row 0: 1 + 0.5 + 0.5 + 0.25 * 7 = 3.75; env 2 as a done
    assert scale[:, 0].tolist() == [3.75, 7.0, 7.0] and scale[:, 1].tolist() == [3.4375, 5.75, 7.0]
    assert scale[:, 2].tolist() == [2.75, 3.0, 7.0]
    # what stands behind a cut is selected away, not multiplied by zero
    v_nan = V.clone(); v_nan[2, 0] = float("nan")
    adv2, ret2, _ = gae_reference(R, done, v_nan, V_LAST, gamma=GAMMA, lam=LAM, truncated=trunc, cut_value=V_CUT)
    assert adv2[:2, 0].tolist() == [2.25, 5.0] and ret2[:2, 0].tolist() == [2.75, 6.0]
    # done NULL: only the cut speaks, and env 2 is then cut like env 0; a NULL cut_value reads as 0
    adv3, _, _ = gae_reference(R, None, V, V_LAST, gamma=GAMMA, lam=LAM, truncated=trunc, cut_value=None)
    assert adv3[:, 0].tolist() == adv3[:, 2].tolist() == [1 + 0.25 * 1, 2 + 0.0 - 1, 3.0]
    # a cut in the last row takes cut_value in the place of last_value
    last = torch.tensor([[0, 0, 0], [0, 0, 0], [1, 0, 0]], dtype=torch.uint8)
    adv4, _, _ = gae_reference(R, None, V, V_LAST, gamma=GAMMA, lam=LAM, truncated=last, cut_value=V_CUT)
    assert adv4[2].tolist() == [3 + 0.5 * 8 - 2, 3.0, 3.0]


def test_reference_without_a_mask_is_the_old_result():
    from simglucose_amd.controller import gae_reference
    g = torch.Generator().manual_seed(7)
    r = torch.randn(6, 9, generator=g, dtype=torch.float64)
    v = torch.randn(6, 9, generator=g, dtype=torch.float64)
    vl = torch.randn(9, generator=g, dtype=torch.float64)
    done = (torch.rand(6, 9, generator=g) < 0.3).to(torch.uint8)
    old = gae_reference(r, done, v, vl, gamma=0.9, lam=0.8)
    for kw in (dict(truncated=None, cut_value=None), dict(truncated=torch.zeros_like(done), cut_value=torch.full_like(vl, float("nan")))):
        new = gae_reference(r, done, v, vl, gamma=0.9, lam=0.8, **kw)
        assert all(torch.equal(a, b) for a, b in zip(old, new))
    # lambda = 0: the one-step TD error with the bootstrap chosen per sample
    trunc = ((torch.rand(6, 9, generator=g) < 0.3) & (done == 0)).to(torch.uint8)
    vc = torch.randn(9, generator=g, dtype=torch.float64)
    adv, ret, _ = gae_reference(r, done, v, vl, gamma=0.9, lam=0.0, truncated=trunc, cut_value=vc)
    v_next = torch.where(trunc != 0, vc.expand(6, 9), torch.cat([v[1:], vl[None]]))
    assert torch.equal(adv, r + 0.9 * v_next * (done == 0) - v) and torch.equal(ret, adv + v)


def _bare_env(n=128, dtype=torch.float64):
    """a BatchedT1DSimEnv that has what collect_mlp reads before its first launch, and nothing else: a call that gets past its
    argument checks ends in an AttributeError, not in a launch"""
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    e = object.__new__(BatchedT1DSimEnv)
    e.integrator, e.n, e.dtype, e.device, e.minutes_per_step = None, n, dtype, torch.device("cpu"), 3
    return e


def test_collect_mlp_limit_refuses_a_bad_limit_before_anything_is_launched():
    import inspect
    import support
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    e, pol = _bare_env(), support.constant_policy(0.05)
    F = 2 * pol.history + 3
    # collect_mlp's arguments behind the limit's two, and collect_mlp itself as it was
    sig, old = inspect.signature(BatchedT1DSimEnv.collect_mlp_limit), inspect.signature(BatchedT1DSimEnv.collect_mlp)
    assert list(sig.parameters)[1:5] == ["n_steps", "policy", "max_episode_steps", "cut_features"]
    assert list(sig.parameters)[5:] == list(old.parameters)[3:]
    assert sig.parameters["on_done"].default == "restart" and sig.parameters["cut_features"].default is None
    assert "max_episode_steps" not in old.parameters and "cut_features" not in old.parameters
    with pytest.raises(ValueError, match="on_done='restart'"):
        e.collect_mlp_limit(4, pol, 10, on_done="continue")
    with pytest.raises(ValueError, match="n_steps must not exceed"):
        e.collect_mlp_limit(11, pol, 10)
    with pytest.raises(ValueError, match="at least 1"):
        e.collect_mlp_limit(1, pol, 0)
    for bad in (torch.zeros(F, e.n + 1, dtype=torch.float64), torch.zeros(F + 1, e.n, dtype=torch.float64),
                torch.zeros(e.n, F, dtype=torch.float64), torch.zeros(F, e.n, dtype=torch.float32),
                torch.zeros(e.n, F, dtype=torch.float64).t(), [[0.0] * e.n] * F):
        with pytest.raises(ValueError, match="cut_features"):
            e.collect_mlp_limit(4, pol, 10, cut_features=bad)
    with pytest.raises(ValueError, match="truncated"):
        e.collect_mlp_limit(4, pol, 10, trace={"row": 1, "truncated": torch.zeros(4, e.n, dtype=torch.uint8)})   # rows 1 .. 4 need five rows
    # a good limit gets past the checks (and then misses what a real env has)
    with pytest.raises(AttributeError):
        e.collect_mlp_limit(10, pol, 10, cut_features=torch.zeros(F, e.n, dtype=torch.float64))
    assert "collect_mlp_dopri5" in support.mode_refusal("collect_mlp", "dopri5")
    e.integrator = "dopri5"
    with pytest.raises(Exception, match="fixed-step"):
        e.collect_mlp_limit(4, pol, 10)


def test_new_trace_has_a_truncated_column():
    e = _bare_env(n=6)
    tr = e.new_trace(4, columns=("truncated", "done"))
    assert tr["row"] == 1
    for k in ("truncated", "done"):
        assert tr[k].dtype == torch.uint8 and tuple(tr[k].shape) == (5, 6) and int(tr[k].max()) == 0
