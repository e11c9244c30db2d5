"""t1d_gae on the GPU (controller.gae -> csrc/t1d_gae.hpp): advantages and value targets against the fp64 torch loop
gae_reference at a bound stated in the rounding of the call's type; the exact properties of the recurrence; the masking of
what stands behind a done; the per-policy moments (against exact sums of the kernel's own advantages, reproducible, and
independent of where a policy's envs sit in the batch); stray writes; the wrapper's argument checks."""
import ctypes as C
import math

import pytest

from support import bits as _bits, gpu_torch as _torch

pytestmark = pytest.mark.gpu
SHAPES = [(64, 1), (100, 1), (100, 4), (192, 3), (300, 1)]        # a full wave; a partial one; policies that straddle a wave;
#                                                                   policies on wave boundaries; more than one 256-thread block
ROWS = [1, 2, 5, 33]                                               # fewer rows than a group of 8, and groups with a short first one
GAMMA_LAMBDA = [(0.99, 0.95), (1.0, 1.0), (0.9, 0.0), (0.0, 0.5)]
DTYPES = ["float64", "float32"]


_cache = {}


def _inputs(n, K, dtype_name):
    """reward, done, value, last_value on the GPU, drawn once per shape with a fixed seed and shared; done with probability
    0.2, rows 0 and K - 1 each with a set and a clear byte; the floating words rounded to the call's type"""
    torch = _torch()
    key = (n, K, dtype_name)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * n + K)
        dt = getattr(torch, dtype_name)
        r = torch.randn(K, n, generator=g, dtype=torch.float64).to(dt)
        v = (3.0 * torch.randn(K, n, generator=g, dtype=torch.float64)).to(dt)
        vl = (3.0 * torch.randn(n, generator=g, dtype=torch.float64)).to(dt)
        d = (torch.rand(K, n, generator=g) < 0.2).to(torch.uint8)
        d[0, 0], d[0, 1], d[K - 1, 2], d[K - 1, 3] = 1, 0, 1, 0
        for row in (0, K - 1):
            assert int(d[row].max()) == 1 and int(d[row].min()) == 0
        _cache[key] = tuple(t.cuda().contiguous() for t in (r, d, v, vl))
    return _cache[key]


def _rows_left(K, like):
    torch = _torch()
    return torch.arange(K, 0, -1, dtype=torch.float64, device=like.device).unsqueeze(1)       # K - s


# ---------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("n,P", SHAPES)
def test_adv_and_ret_against_the_reference(n, P, dtype_name):
    """|adv - ref| <= 4 (K - s) eps scale[s], |ret - ref| <= that + eps |ret|.  A row makes at most three roundings (two fma, one
    subtraction), each at most eps / 2 of a partial result that scale[s] bounds, and in fp32 the rounding of g and g lambda
    adds two more of the same size: 2.5 eps scale per row at most, carried on with the factor g lambda <= 1; the 4 leaves
    room for the fp64 reference's own rounding.  ret adds one rounding of its own."""
    torch = _torch()
    from simglucose_amd.controller import gae, gae_reference
    eps = torch.finfo(getattr(torch, dtype_name)).eps
    worst_a = worst_r = 0.0
    for K in ROWS:
        r, d, v, vl = _inputs(n, K, dtype_name)
        for gamma, lam in GAMMA_LAMBDA:
            adv, ret = gae(r, d, v, vl, gamma=gamma, lam=lam, n_policies=P)
            ra, rr, scale = gae_reference(r, d, v, vl, gamma=gamma, lam=lam)
            assert adv.dtype == r.dtype and adv.shape == ret.shape == (K, n)
            ea, er = (adv.double() - ra).abs(), (ret.double() - rr).abs()
            bound = 4 * _rows_left(K, scale) * eps * scale
            worst_a = max(worst_a, float((ea / (eps * scale)).max()))
            worst_r = max(worst_r, float((er / (eps * (scale + rr.abs()))).max()))
            assert bool((ea <= bound).all()), (K, gamma, lam, float((ea / (eps * scale)).max()))
            assert bool((er <= bound + eps * rr.abs()).all()), (K, gamma, lam)
    print("\n[gae %s n=%d P=%d] max |adv - ref| / (eps scale) = %.3f, max |ret - ref| / (eps (scale + |ret|)) = %.3f"
          % (dtype_name, n, P, worst_a, worst_r))


# ---------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("n,P", SHAPES)
def test_exact_properties(n, P, dtype_name):
    torch = _torch()
    from simglucose_amd.controller import gae
    from simglucose_amd.controller.gae import gae_call
    eps = torch.finfo(getattr(torch, dtype_name)).eps
    for K in ROWS:
        r, d, v, vl = _inputs(n, K, dtype_name)
        # every step ends an episode: nothing is carried from row to row
        for gamma, lam in GAMMA_LAMBDA:
            adv, ret = gae(r, torch.ones_like(d), v, vl, gamma=gamma, lam=lam, n_policies=P)
            assert torch.equal(adv, r - v) and torch.equal(ret, adv + v)
        # no critic, no episode ends, gamma = 1: the suffix sums of the rewards
        adv, ret = gae(r, None, None, None, gamma=1.0, lam=1.0, n_policies=P)
        want = torch.flip(torch.cumsum(torch.flip(r.double(), [0]), 0), [0])
        scale = torch.flip(torch.cumsum(torch.flip(r.double().abs(), [0]), 0), [0])
        assert bool(((adv.double() - want).abs() <= 4 * _rows_left(K, scale) * eps * scale).all())
        assert torch.equal(ret, adv)
        # one output alone is the full call's
        adv, ret = gae(r, d, v, vl, n_policies=P)
        only_a, only_r = torch.full_like(r, 7.0), torch.full_like(r, 7.0)
        gae_call(r, d, v, vl, n_policies=P, adv=only_a)
        gae_call(r, d, v, vl, n_policies=P, ret=only_r)
        assert torch.equal(_bits(only_a), _bits(adv)) and torch.equal(_bits(only_r), _bits(ret))


# ---------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("n,P", SHAPES)
def test_nothing_behind_a_done_reaches_the_row_before(n, P, dtype_name):
    """The trap of on_done="restart": row s + 1 belongs to the next episode of an env that finished in row s.  value[s + 1] is
    NaN wherever done[s] is set, last_value is NaN where done[K - 1] is set, and the outputs are compared, bit for bit, with
    those of the same call with zeros in those words.  With last_value poisoned alone that is every output.  value[s + 1]
    is also row s + 1's own baseline (delta[s + 1] subtracts it), so with value poisoned the rows s + 1 themselves, and the
    rows of their episode before them, are NaN by the definition of the recurrence; every other output -- the finished rows
    s first of all -- must be finite and unchanged."""
    torch = _torch()
    from simglucose_amd.controller import gae
    for K in ROWS:
        r, d, v, vl = _inputs(n, K, dtype_name)
        behind = torch.zeros_like(d, dtype=torch.bool)
        behind[1:] = d[:-1] != 0
        last = d[K - 1] != 0
        assert bool(last.any()) and (K == 1 or bool(behind.any()))
        nan = torch.full_like(v, float("nan"))
        v_nan, v_zero = torch.where(behind, nan, v), torch.where(behind, torch.zeros_like(v), v)
        vl_nan, vl_zero = torch.where(last, nan[0], vl), torch.where(last, torch.zeros_like(vl), vl)
        # what the poisoned baselines reach by definition: their own row, and through the running advantage the rows of
        # the same episode before it
        tainted = torch.zeros_like(behind)
        run = torch.zeros(n, dtype=torch.bool, device=r.device)
        for s in range(K - 1, -1, -1):
            run = (run & (d[s] == 0)) | behind[s]
            tainted[s] = run
        clean = ~tainted
        fin = d[:-1] != 0
        assert K == 1 or bool((fin & clean[:-1]).any())               # finished rows with a NaN right above them are compared
        for gamma, lam in GAMMA_LAMBDA:
            a0, r0, m0, s0 = gae(r, d, v_zero, vl_zero, gamma=gamma, lam=lam, n_policies=P, moments=True)
            a1, r1, m1, s1 = gae(r, d, v_zero, vl_nan, gamma=gamma, lam=lam, n_policies=P, moments=True)
            assert bool(torch.isfinite(a1).all()) and bool(torch.isfinite(r1).all())
            assert torch.equal(_bits(a1), _bits(a0)) and torch.equal(_bits(r1), _bits(r0))
            assert torch.equal(_bits(m1), _bits(m0)) and torch.equal(_bits(s1), _bits(s0))
            a2, r2 = gae(r, d, v_nan, vl_nan, gamma=gamma, lam=lam, n_policies=P)
            assert bool(torch.isfinite(a2[clean]).all()) and bool(torch.isfinite(r2[clean]).all())
            assert torch.equal(_bits(a2[clean]), _bits(a0[clean])) and torch.equal(_bits(r2[clean]), _bits(r0[clean]))


# ---------------------------------------------------------------------------------------------------------- 4
def _exact_sums(adv, P):
    """per policy: the exactly rounded sum of the advantages (math.fsum) and of their squares as doubles"""
    x = adv.double().cpu()
    K, n = x.shape
    E = n // P
    out = []
    for p in range(P):
        blk = x[:, p * E:(p + 1) * E].reshape(-1).tolist()
        out.append((math.fsum(blk), math.fsum(abs(t) for t in blk), math.fsum(t * t for t in blk)))
    return out


@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("n,P", SHAPES)
def test_moments(n, P, dtype_name):
    """|sum - ref| <= N u sum |adv| and |sumsq - ref| <= (N + 1) u sum adv^2, u = 2^-53, N = K E: the worst case of adding N
    doubles in any order (and one more rounding for each square)."""
    torch = _torch()
    from simglucose_amd.controller import gae
    from simglucose_amd.controller.gae import gae_call
    u = 2.0 ** -53
    E = n // P
    for K in ROWS:
        r, d, v, vl = _inputs(n, K, dtype_name)
        adv, ret, mean, std = gae(r, d, v, vl, n_policies=P, moments=True)
        a_plain, r_plain = gae(r, d, v, vl, n_policies=P)
        assert torch.equal(_bits(adv), _bits(a_plain)) and torch.equal(_bits(ret), _bits(r_plain))
        assert mean.dtype == std.dtype == torch.float64 and mean.shape == std.shape == (P,)
        sums = torch.empty(P, 2, dtype=torch.float64, device=r.device)
        gae_call(r, d, v, vl, n_policies=P, moments=sums)            # the moments alone
        N = K * E
        for p, (s1, sabs, s2) in enumerate(_exact_sums(adv, P)):
            assert abs(float(sums[p, 0]) - s1) <= N * u * sabs, (K, p)
            assert abs(float(sums[p, 1]) - s2) <= (N + 1) * u * s2, (K, p)
            assert abs(float(mean[p]) - float(sums[p, 0]) / N) <= 4 * u * abs(float(sums[p, 0]) / N)    # one division, on the device
            want_std = math.sqrt(max(s2 / N - (s1 / N) ** 2, 0.0))
            assert abs(float(std[p]) - want_std) <= 1e-9 * (want_std + abs(s1 / N)) + 1e-300
        # two calls: identical bits
        again = torch.empty_like(sums)
        gae_call(r, d, v, vl, n_policies=P, adv=torch.empty_like(r), moments=again)
        assert torch.equal(_bits(again), _bits(sums))
        # the policies' env blocks permuted as whole blocks: the permuted moments, bit for bit
        if P > 1:
            perm = torch.tensor([(p * 2 + 1) % P if P % 2 else P - 1 - p for p in range(P)])
            assert sorted(perm.tolist()) == list(range(P)) and perm.tolist() != list(range(P))
            cols = (perm.unsqueeze(1) * E + torch.arange(E).unsqueeze(0)).reshape(-1).to(r.device)
            moved = torch.empty_like(sums)
            gae_call(r[:, cols].contiguous(), d[:, cols].contiguous(), v[:, cols].contiguous(), vl[cols].contiguous(), n_policies=P,
                     moments=moved)
            assert torch.equal(_bits(moved), _bits(sums[perm.to(r.device)]))


# ---------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("n,P", SHAPES)
def test_nothing_beyond_the_outputs_is_written(n, P, dtype_name):
    torch = _torch()
    from simglucose_amd import _lib
    from simglucose_amd.controller.gae import gae_call
    K, tail = 5, 777
    r, d, v, vl = _inputs(n, K, dtype_name)
    io = _lib.GaeBatch()
    io.n_rows, io.n_policies, io.gamma, io.lam = K, P, 0.99, 0.95
    need = _lib.lib().t1d_gae_workspace(_lib.T1D_F64, n, C.byref(io))
    assert need == 16 * P * ((n // P + 63) // 64)
    adv = torch.full((K * n + tail,), -5.0, dtype=r.dtype, device=r.device)
    ret = torch.full((K * n + tail,), -6.0, dtype=r.dtype, device=r.device)
    ws = torch.full((need + tail,), 0xA5, dtype=torch.uint8, device=r.device)
    mom = torch.full((2 * P + tail,), -7.0, dtype=torch.float64, device=r.device)
    before = [t.clone() for t in (r, d, v, vl)]
    gae_call(r, d, v, vl, n_policies=P, adv=adv[:K * n].view(K, n), ret=ret[:K * n].view(K, n), moments=mom[:2 * P].view(P, 2),
             workspace=ws[:need])
    torch.cuda.synchronize()
    assert bool((adv[K * n:] == -5.0).all()) and bool((ret[K * n:] == -6.0).all())
    assert bool((ws[need:] == 0xA5).all()) and bool((mom[2 * P:] == -7.0).all())
    assert bool((adv[:K * n] != -5.0).all()) and bool((mom[:2 * P] != -7.0).all())
    for t, b in zip((r, d, v, vl), before):
        assert torch.equal(t, b)


# ---------------------------------------------------------------------------------------------------------- 6
def test_wrapper_rejects_bad_arguments():
    torch = _torch()
    from simglucose_amd.controller import gae
    r, d, v, vl = _inputs(192, 5, "float64")
    gae(r, d, v, vl)                                                 # the good call
    for bad in (dict(reward=r.t().contiguous().t()), dict(value=v.t().contiguous().t()), dict(done=d.t().contiguous().t()),
                dict(last_value=torch.zeros(2 * 192, dtype=r.dtype, device=r.device)[::2]),           # non-contiguous
                dict(reward=r.float()), dict(value=v.float()), dict(done=d.bool()), dict(done=d.int()),
                dict(last_value=vl.float()), dict(reward=r.to(torch.float16)),                       # wrong dtype
                dict(reward=r.cpu()), dict(value=v.cpu()), dict(done=d.cpu()), dict(last_value=vl.cpu()),   # wrong device
                dict(reward=r[0]), dict(value=v[:4]), dict(done=d[:, :64].contiguous()), dict(last_value=vl[:64].contiguous()),
                dict(last_value=vl.unsqueeze(0)), dict(reward=r[:0]),                                # wrong shape
                dict(n_policies=5), dict(n_policies=0), dict(gamma=1.5), dict(lam=-0.1), dict(gamma=float("nan"))):
        kw = dict(reward=r, done=d, value=v, last_value=vl)
        kw.update(bad)
        with pytest.raises(ValueError):
            gae(**kw)
