"""Which kernel t1d_step and the roll-outs launch, on what grid and with how much LDS: dispatch_plan_driver.cpp includes the
library's source, plans hand-made calls on the CPU and checks each plan against its table of expected rows."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_dispatch_plan_matches_table(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj, exe = str(tmp_path / "driver.o"), str(tmp_path / "driver")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-fgpu-rdc", "-std=c++17", "-O1", "-c",
                           os.path.join(HERE, "dispatch_plan_driver.cpp"), "-o", obj])
    subprocess.check_call([hipcc, "-fgpu-rdc", "--hip-link", "--offload-arch=gfx950", obj, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == "162 rows, 0 failed"
