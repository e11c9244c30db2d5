"""The exact mode (t1d_step_dopri5, BatchedT1DSimEnv(integrator="dopri5")) without a GPU: the symbol, the argument checks
that need no device, the Python-side checks that run before the GPU check, and the kernel's registers."""
import ctypes as C
import os
import re

import pytest

from support import kernel_asm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_t1d_step_dopri5_is_declared_exported_and_loadable():
    from simglucose_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "t1d.h")).read(), flags=re.S)
    assert re.search(r"int\s+t1d_step_dopri5\s*\(\s*t1d_ctx\s*\*\s*ctx\s*,\s*const\s+t1d_batch\s*\*\s*b\s*,\s*double\s*\*\s*h_carry\s*,"
                     r"\s*int32_t\s*\*\s*nfev\s*,\s*int\s+minutes\s*,\s*void\s*\*\s*hip_stream\s*\)", src)
    assert "T1D_ST_SOLVER_FAILED = 16" in src and _lib.T1D_ST_SOLVER_FAILED == 16
    assert "t1d_step_dopri5" in _lib.EXPORTS
    L = _lib.lib()
    assert hasattr(L, "t1d_step_dopri5")
    assert L.t1d_abi_version() == 4
    # the header is a source of the build: an edit to it rebuilds the library
    assert os.path.join(ROOT, "simglucose_amd", "csrc", "t1d_dopri5.hpp") in _lib.SOURCES


def test_null_arguments_are_rejected_without_a_device():
    """NULL ctx, batch or h_carry -> T1D_E_INVALID; none of these paths looks at the ctx (a dummy pointer stands in)."""
    from simglucose_amd import _lib
    L = _lib.lib()
    b = _lib.Batch()
    b.n, b.dtype = 4, _lib.T1D_F64
    hc = (C.c_double * 4)()
    fake_ctx = C.c_void_p(8)
    assert L.t1d_step_dopri5(None, C.byref(b), C.cast(hc, C.c_void_p), None, 1, None) == -1
    assert b"ctx" in L.t1d_last_error()
    assert L.t1d_step_dopri5(fake_ctx, None, C.cast(hc, C.c_void_p), None, 1, None) == -1
    assert b"batch" in L.t1d_last_error()
    assert L.t1d_step_dopri5(fake_ctx, C.byref(b), None, None, 1, None) == -1
    assert b"h_carry" in L.t1d_last_error()
    b.dtype = _lib.T1D_F32
    assert L.t1d_step_dopri5(fake_ctx, C.byref(b), C.cast(hc, C.c_void_p), None, 1, None) == -1
    assert b"fp64" in L.t1d_last_error()
    b.dtype = _lib.T1D_F64
    for minutes in (0, -3, 100001):
        assert L.t1d_step_dopri5(fake_ctx, C.byref(b), C.cast(hc, C.c_void_p), None, minutes, None) == -1
        assert b"minutes" in L.t1d_last_error()


def test_integrator_argument_is_checked_before_the_gpu():
    import torch
    from simglucose_amd.batch_env import BatchedT1DSimEnv
    with pytest.raises(ValueError, match="integrator"):
        BatchedT1DSimEnv(patient="adult#001", n_envs=2, integrator="rk45")
    with pytest.raises(ValueError, match="float64"):
        BatchedT1DSimEnv(patient="adult#001", n_envs=2, integrator="dopri5", dtype=torch.float32)


def test_dopri5_kernel_needs_no_scratch():
    """One wave per SIMD with the unified VGPR + AGPR file: the seven stage vectors, y, y1 and the stage input stay in
    registers (a spill would sit inside the stage loop)."""
    mine = [k for k in kernel_asm().kernels(kernel_asm().device_asm()).values() if k.name.startswith("_ZN3t1d18dopri5_step_kernel")]
    assert len(mine) == 1, mine
    assert mine[0].figures["scratch_bytes_per_lane"] == 0, mine[0].figures
