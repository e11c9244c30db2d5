"""CPU suite: the device-side episode restart (t1d_restart_done) as far as it goes without a GPU -- the export, the ctypes
mirror of struct t1d_restart, argument validation, and the Python start-hour function the kernel restates."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restart_symbol_is_exported_and_struct_matches_header_field_for_field():
    from simglucose_amd import _lib
    L = _lib.lib()
    assert "t1d_restart_done" in _lib.EXPORTS and hasattr(L, "t1d_restart_done")
    assert L.t1d_abi_version() == 4                                   # no existing struct changed
    src = open(os.path.join(ROOT, "include", "t1d.h")).read()
    body = src[src.index("typedef struct t1d_restart {"):src.index("} t1d_restart;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).replace("typedef struct t1d_restart {", "")
    names, sizes = [], []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        names.append(re.findall(r"([A-Za-z_0-9]+)\s*$", stmt)[0])
        sizes.append(8 if "*" in stmt else {"int32_t": 4, "int64_t": 8, "double": 8}[stmt.split()[0]])
    assert names == [f[0] for f in _lib.Restart._fields_]
    assert sizes == [C.sizeof(f[1]) for f in _lib.Restart._fields_]
    assert C.sizeof(_lib.Restart) == sum(sizes) == 4 * 4 + 9 * 8       # no padding: four int32 ahead of the pointers
    for f, s in zip(_lib.Restart._fields_, sizes):
        assert getattr(_lib.Restart, f[0]).size == s


def test_restart_rejects_bad_arguments_without_touching_a_gpu():
    from simglucose_amd import _lib
    L = _lib.lib()
    fake = 0x1000                                                     # never dereferenced: every call below is refused

    def call(days=2, n_meals=18, normals=None, n_normals=0, x0=None, mt=fake, ma=fake + 8, rmt=fake, rma=fake + 8,
             start=fake + 16, episode=fake + 24, ep_return=None, ep_length=None, last_return=None, reserved=0,
             no_batch=False, no_restart=False, dtype=0, h_carry=None):
        b, r = _lib.Batch(), _lib.Restart()
        b.n, b.dtype, b.n_meals, b.n_normals = 64, dtype, n_meals, n_normals
        b.normals, b.x0_override, b.meal_time, b.meal_amt, b.episode = normals, x0, mt, ma, episode
        r.days, r.random_init_bg, r.reserved = days, 1, reserved
        r.meal_time, r.meal_amt, r.start_minute, r.h_carry = rmt, rma, start, h_carry
        r.ep_return, r.ep_length, r.last_return = ep_return, ep_length, last_return
        rc = L.t1d_restart_done(None, None if no_batch else C.byref(b), None, None if no_restart else C.byref(r), None)
        return rc, L.t1d_last_error()

    for kw, word in ((dict(no_batch=True), b"batch is NULL"), (dict(no_restart=True), b"restart is NULL"),
                     (dict(days=0), b"days"), (dict(days=-3), b"days"), (dict(reserved=1), b"reserved"),
                     (dict(normals=fake, n_normals=4), b"host-normals"), (dict(n_normals=4), b"host-normals"),
                     (dict(x0=fake), b"x0_override"),
                     (dict(rmt=None), b"NULL"), (dict(rma=None), b"NULL"), (dict(start=None), b"NULL"),
                     (dict(rmt=fake + 64), b"tables the batch names"), (dict(rma=fake + 64), b"tables the batch names"),
                     (dict(n_meals=12), b"6 (days + 1)"), (dict(days=1), b"6 (days + 1)"),
                     (dict(episode=None), b"episode"),
                     (dict(ep_return=fake), b"go together"), (dict(ep_length=fake), b"go together"),
                     (dict(last_return=fake), b"need ep_return"),
                     (dict(h_carry=fake, dtype=1), b"h_carry"),
                     (dict(), b"ctx is NULL")):                       # a well-formed call still needs a context
        rc, msg = call(**kw)
        assert rc == -1 and b"t1d_restart_done" in msg and word in msg, (kw, rc, msg)


def test_start_hours_are_hours_and_a_function_of_seed_episode_and_global_id_only():
    import torch
    from simglucose_amd.envs.batched_gym_env import start_hours
    gid = torch.arange(20000, dtype=torch.int64)
    for seed in (0, 3, 2 ** 63 + 5, -7):
        for ep in (0, 1, 77):
            h = start_hours(seed, ep, gid)
            assert h.dtype == torch.int64 and int(h.min()) == 0 and int(h.max()) == 23
            assert int(torch.bincount(h, minlength=24).min()) > 20000 // 24 // 2          # all 24 hours, roughly evenly
            assert torch.equal(h, start_hours(seed, torch.full_like(gid, ep), gid))       # per-env episode index = scalar
            assert torch.equal(h[5000:], start_hours(seed, ep, gid[5000:]))               # shards = slices
    assert not torch.equal(start_hours(3, 0, gid), start_hours(3, 1, gid))
    assert not torch.equal(start_hours(3, 0, gid), start_hours(4, 0, gid))
    ep = torch.arange(20000, dtype=torch.int64) % 5
    mixed = start_hours(3, ep, gid)
    for k in range(5):
        assert torch.equal(mixed[ep == k], start_hours(3, k, gid)[ep == k])
    # the value the kernel's restatement (splitmix64 in uint64 arithmetic) gives, worked out with Python integers
    M = (1 << 64) - 1
    for seed, k, g in ((3, 0, 0), (3, 2, 4095), (2 ** 63 + 5, 7, 123456789)):
        z = (g * 0x9E3779B97F4A7C15 + seed * 1000003 + k) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        assert int(start_hours(seed, k, torch.tensor([g]))[0]) == (z >> 11) % 24


def test_gym_wrapper_refuses_exact_with_device_restart_and_unknown_modes():
    """argument checks come before anything touches the GPU"""
    from simglucose_amd.envs import BatchedGymT1DSimEnv
    with pytest.raises(ValueError, match="exact"):
        BatchedGymT1DSimEnv(4, auto_reset="device", exact=True)
    with pytest.raises(ValueError, match="auto_reset"):
        BatchedGymT1DSimEnv(4, auto_reset="gpu")
