"""GPU suite: t1d_mlp_grad_tiles / t1d_mlp_loss_tiles and tiles= of controller.ppo_clip_loss / value_loss -- the fused losses
and the gradient call on a minibatch given as a list of 64-env tiles, read in place.

Everything here is a bit-for-bit comparison between two device calls (the header's two identities), so the inputs need not
stay clear of the clip boundaries.  Shapes: H = 1 (F = 5), n = 128 P and K = 3, so C = 2 chunks and 6 tiles per policy: the
smallest batch in which the row / chunk decode, the policy offset and the per-policy list row can each go wrong."""
import functools

import pytest

from support import bits, gpu_torch as _torch, identity_policy

pytestmark = pytest.mark.gpu

K, CN, CLIP = 3, 2, 0.2
TILES = CN * K
PATTERN = -7.25                                                          # what y and coef_out hold before a call
NETS = [(4, 1), (5, 3, 1)]
KINDS = ("ppo", "mse", "grad")
ARRAYS = ("feat", "eps", "y_old", "adv", "target", "coef_in")
# a shuffled list with a duplicate and a missing tile per policy, and other ones for the second policy
SHUFFLED = [[4, 1, 5, 1, 0, 3], [2, 2, 0, 5, 3, 1]]


@functools.lru_cache(maxsize=None)
def case(widths, P, f64):
    """the inputs of one case on the device, made once: features in [-2, 2], standard normal eps / adv / target / coef, the
    collector's weights and new ones, y_old = the network under the collector's weights"""
    torch = _torch()
    from simglucose_amd.controller.mlp_grad import mlp_grad_call
    dtype = torch.float64 if f64 else torch.float32
    pol = identity_policy(1, widths, P, hidden="tanh", seed=7)
    n = 64 * CN * P
    g = torch.Generator().manual_seed(11)
    dev = lambda t: t.to(dtype).cuda().contiguous()
    d = {"pol": pol, "P": P, "dtype": dtype, "n": n}
    d["feat"] = dev(torch.rand(K, pol.n_features, n, generator=g, dtype=torch.float64) * 4 - 2)
    for k in ("eps", "adv", "target", "coef_in"):
        d[k] = dev(torch.randn(K, n, generator=g, dtype=torch.float64))
    old = pol.flat_params()
    d["old"], d["params"] = dev(old), dev(old + 0.05 * torch.randn(old.shape, generator=g, dtype=torch.float64))
    d["sigma_old"] = dev(torch.full((P,), 0.3, dtype=torch.float64))
    d["sigma"] = dev(torch.tensor([0.33, 0.28], dtype=torch.float64)[:P])
    d["y_old"] = torch.empty(K, n, dtype=dtype, device="cuda")
    mlp_grad_call(pol, d["old"], d["feat"], y=d["y_old"])
    torch.cuda.synchronize()
    return d


def run(d, kind, tiles=None, scale=None):
    """one raw call -> {"y", "grad"} and for the losses {"coef", "stats"}; y and coef hold PATTERN before it, grad and stats
    NaN"""
    torch = _torch()
    from simglucose_amd import _lib
    from simglucose_amd.controller.mlp_grad import mlp_grad_call
    from simglucose_amd.controller.policy_loss import mlp_loss_call
    feat, params = d["feat"], d["params"]
    rows, n = feat.shape[0], feat.shape[2]
    full = lambda v, *shape, dt=feat.dtype: torch.full(shape, v, dtype=dt, device="cuda")
    o = {"y": full(PATTERN, rows, n), "grad": torch.full_like(params, float("nan"))}
    if scale is None:
        scale = 1.0 / (rows * n) if tiles is None else 1.0 / (64 * tiles.shape[-1] * params.shape[0])
    if kind == "grad":
        mlp_grad_call(d["pol"], params, feat, coef=d["coef_in"], y=o["y"], grad=o["grad"], tiles=tiles)
        return o
    o["coef"], o["stats"] = full(PATTERN, rows, n), full(float("nan"), params.shape[0], 4, dt=torch.float64)
    if kind == "ppo":
        mlp_loss_call(d["pol"], params, feat, _lib.T1D_LOSS_PPO_CLIP, scale, eps=d["eps"], y_old=d["y_old"], adv=d["adv"],
                      sigma_old=d["sigma_old"], sigma=d["sigma"], clip=CLIP, y=o["y"], coef_out=o["coef"], grad=o["grad"], stats=o["stats"],
                      tiles=tiles)
    else:
        mlp_loss_call(d["pol"], params, feat, _lib.T1D_LOSS_VALUE_MSE, scale, target=d["target"], y=o["y"], coef_out=o["coef"],
                      grad=o["grad"], stats=o["stats"], tiles=tiles)
    return o


def gathered(d, tiles):
    """the case restated as a batch of the listed tiles alone"""
    from simglucose_amd.controller import gather_tiles
    g = dict(d)
    for k in ARRAYS:
        g[k] = gather_tiles(d[k], tiles, d["params"].shape[0])
    return g


def one_policy(d, p):
    """policy p's envs, weights and sigmas as a single-policy case"""
    E = d["n"] // d["P"]
    g = dict(d)
    for k in ARRAYS:
        g[k] = d[k][..., p * E:(p + 1) * E].contiguous()
    for k in ("params", "sigma", "sigma_old"):
        g[k] = d[k][p:p + 1].contiguous()
    return g


def same(a, b, keys=None):
    torch = _torch()
    for k in (keys or a.keys()):
        assert torch.equal(bits(a[k]), bits(b[k])), k


def ids(rows):
    torch = _torch()
    return torch.tensor(rows, dtype=torch.int32, device="cuda").contiguous()


def visited(d, rows):
    """[K, n] bool: the words the lists `rows` (one per policy) name"""
    torch = _torch()
    E = d["n"] // d["P"]
    m = torch.zeros(K, d["n"], dtype=torch.bool)
    for p, row in enumerate(rows):
        for u in row:
            if 0 <= u < TILES:
                m[u // CN, p * E + 64 * (u % CN):p * E + 64 * (u % CN) + 64] = True
    return m.cuda()


CASES = [(w, P, f64) for w in NETS for P in (1, 2) for f64 in (True, False)]


# ------------------------------------------------------------------------------------------------ 1: the identity list
@pytest.mark.parametrize("widths,P,f64", CASES)
def test_identity_list_gives_the_plain_calls_bits(widths, P, f64):
    torch = _torch()
    d = case(widths, P, f64)
    for kind in KINDS:
        plain, listed = run(d, kind), run(d, kind, ids([list(range(TILES))] * P))
        same(plain, listed)
        assert bool(torch.isfinite(plain["grad"]).all()) and float(plain["grad"].abs().max()) > 0
        assert not bool((plain["y"] == PATTERN).any())


# ------------------------------------------------------------------------------------------------ 2: any list
@pytest.mark.parametrize("widths,P,f64", CASES)
def test_shuffled_list_equals_the_plain_call_on_the_gathered_batch(widths, P, f64):
    torch = _torch()
    from simglucose_amd.controller import gather_tiles
    d = case(widths, P, f64)
    rows = SHUFFLED[:P]
    tiles, mask = ids(rows), visited(d, rows)
    assert int(mask.sum()) == 5 * 64 * P                                 # one tile of six is missing, one is named twice
    for kind in KINDS:
        listed, ref = run(d, kind, tiles), run(gathered(d, tiles), kind)
        same(listed, ref, ("grad", "stats") if kind != "grad" else ("grad",))
        assert bool(torch.isfinite(listed["grad"]).all()) and float(listed["grad"].abs().max()) > 0
        for k in ("y", "coef") if kind != "grad" else ("y",):
            assert torch.equal(bits(gather_tiles(listed[k], tiles, P)), bits(ref[k])), k
            assert bool((listed[k][~mask] == PATTERN).all()) and not bool((listed[k][mask] == PATTERN).any()), k
        assert not torch.equal(bits(listed["grad"]), bits(run(d, kind)["grad"]))


# ------------------------------------------------------------------------------------------------ 3: a list per policy
@pytest.mark.parametrize("widths", NETS)
@pytest.mark.parametrize("f64", [True, False])
def test_every_policy_follows_its_own_row_of_the_list(widths, f64):
    torch = _torch()
    d = case(widths, 2, f64)
    tiles = ids(SHUFFLED)
    for kind in KINDS:
        both = run(d, kind, tiles)
        for p in range(2):
            alone = run(gathered(one_policy(d, p), tiles[p]), kind, scale=1.0 / (64 * 6 * 2))
            for k in ("grad", "stats") if kind != "grad" else ("grad",):
                assert torch.equal(bits(both[k][p]), bits(alone[k][0])), (k, p)
        assert not torch.equal(both["grad"][0], both["grad"][1])


# ------------------------------------------------------------------------------------------------ 4: skipped ids
@pytest.mark.parametrize("widths,P,f64", CASES)
def test_skipped_ids_add_nothing_and_touch_nothing(widths, P, f64):
    """ids outside [0, C K) beside valid ones, on valid memory throughout: the call with them equals the call without"""
    torch = _torch()
    d = case(widths, P, f64)
    big = 2 ** 31 - 1
    with_skips = [[-1, 4, TILES, 1, big, 5, 1, -1, -1, 0, 3, TILES], [big, 2, 2, -1, 0, TILES, TILES, 5, 3, big, 1, -1]][:P]
    assert [[u for u in row if 0 <= u < TILES] for row in with_skips] == SHUFFLED[:P]
    assert P * len(with_skips[0]) <= 2048                                # T = 1: every position is a partial of its own
    for kind in KINDS:
        # the same scale in both calls: the lists differ in length
        a, b = run(d, kind, ids(with_skips), scale=1.0 / 384), run(d, kind, ids(SHUFFLED[:P]), scale=1.0 / 384)
        same(a, b)
        none = run(d, kind, ids([[-1, TILES, big, -5, TILES + 1, -(2 ** 31)]] * P))
        assert bool((none["grad"] == 0).all()) and bool((none["y"] == PATTERN).all())
        if kind != "grad":
            assert bool((none["stats"] == 0).all()) and bool((none["coef"] == PATTERN).all())


# ------------------------------------------------------------------------------------------------ 5, 6: T > 1, determinism
@pytest.mark.parametrize("widths", NETS)
@pytest.mark.parametrize("f64", [True, False])
def test_two_positions_per_partial_and_determinism(widths, f64):
    """P = 2, M = 1100: 2200 positions, more than 2048, so T = 2 -- as in the plain call on the gathered [1100, F, 128] batch"""
    torch = _torch()
    d = case(widths, 2, f64)
    tiles = torch.randint(0, TILES, (2, 1100), generator=torch.Generator().manual_seed(3), dtype=torch.int32).cuda().contiguous()
    g = gathered(d, tiles)
    assert tuple(g["feat"].shape) == (1100, 5, 128)
    for kind in KINDS:
        listed, ref, again = run(d, kind, tiles), run(g, kind), run(d, kind, tiles)
        same(listed, ref, ("grad", "stats") if kind != "grad" else ("grad",))
        same(listed, again)
        assert bool(torch.isfinite(listed["grad"]).all()) and float(listed["grad"].abs().max()) > 0
        assert not bool((listed["y"] == PATTERN).any())                  # 1100 draws from 6 tiles name every one


# ------------------------------------------------------------------------------------------------ 7: the Python surface
@pytest.mark.parametrize("widths,P,f64", CASES)
def test_python_surface_equals_the_losses_on_the_gathered_arrays(widths, P, f64):
    torch = _torch()
    from simglucose_amd.controller import gather_tiles, ppo_clip_loss, tile_minibatches, value_loss
    d = case(widths, P, f64)
    mb = tile_minibatches(K, d["n"], P, 2, generator=torch.Generator().manual_seed(9))[1].cuda()
    assert tuple(mb.shape) == (P, 3)
    g = gathered(d, mb)

    def actor(c, **kw):
        params, sigma = c["params"].clone().requires_grad_(True), c["sigma"].clone().requires_grad_(True)
        loss, st = ppo_clip_loss(params, c["feat"], c["pol"], c["eps"], c["y_old"], c["adv"], sigma, sigma_old=c["sigma_old"], clip=CLIP,
                                 return_stats=True, **kw)
        loss.backward()
        return {"loss": loss.detach(), "params.grad": params.grad, "sigma.grad": sigma.grad, **st}

    def critic(c, **kw):
        params = c["params"].clone().requires_grad_(True)
        loss = value_loss(params, c["feat"], c["pol"], c["target"], **kw)
        loss.backward()
        return {"loss": loss.detach(), "params.grad": params.grad}

    a, b = actor(d, tiles=mb), actor(g)
    same(a, b)
    assert set(a) == {"loss", "params.grad", "sigma.grad", "clip_frac", "approx_kl"} and float(a["params.grad"].abs().max()) > 0
    assert float(a["sigma.grad"].abs().min()) > 0
    same(critic(d, tiles=mb), critic(g))
    if P == 1:                                                           # [M] is taken with one policy
        same(critic(d, tiles=mb[0].contiguous()), critic(g))
    same(actor(d), actor(d, tiles=ids([list(range(TILES))] * P)))        # tiles=None is the identity list's result


# ------------------------------------------------------------------------------------------------ 8: an epoch
@pytest.mark.parametrize("widths,P,f64", CASES)
def test_the_minibatches_of_an_epoch_add_up_to_the_batch(widths, P, f64):
    """6 tiles in 3 minibatches: nothing is left out.  The not-active counts add up exactly; the loss sums within the bound
    of tests/test_gpu_policy_loss.py for its loss sum, relative to the sum of the terms' magnitudes: LOSS_RTOL for PPO, and
    for the value loss (8 u + N 2^-53) sum loss_i of the same file (its terms are not negative)."""
    torch = _torch()
    from simglucose_amd.controller import ppo_clip_loss_reference, tile_minibatches
    from test_gpu_policy_loss import LOSS_RTOL
    d = case(widths, P, f64)
    mbs = [mb.cuda() for mb in tile_minibatches(K, d["n"], P, 3, generator=torch.Generator().manual_seed(4))]
    assert len(mbs) == 3 and torch.equal(torch.cat(mbs, dim=1).sort(dim=1).values.cpu(), torch.arange(TILES, dtype=torch.int32).expand(P, TILES))
    N = K * d["n"] // P
    u = 2.0 ** -53 if f64 else 2.0 ** -24
    for kind in ("ppo", "mse"):
        full = run(d, kind)
        parts = [run(d, kind, mb)["stats"] for mb in mbs]
        total = parts[0] + parts[1] + parts[2]
        if kind == "ppo":
            info = ppo_clip_loss_reference(full["y"].double(), d["eps"], d["y_old"], d["adv"], d["sigma"], d["sigma_old"], CLIP, P)[4]
            bound = LOSS_RTOL[f64] * info["loss_mag"]
            assert torch.equal(total[:, 1], full["stats"][:, 1]) and float(full["stats"][:, 1].min()) > 0
        else:
            bound = (8 * u + N * 2.0 ** -53) * full["stats"][:, 0]
        err = (total[:, 0] - full["stats"][:, 0]).abs()
        print("%s %s P %d %s: loss sum %.3e of the bound" % (kind, widths, P, d["dtype"], float((err / bound).max())))
        assert bool((err <= bound).all())
        assert float(full["stats"][:, 0].abs().min()) > 0
