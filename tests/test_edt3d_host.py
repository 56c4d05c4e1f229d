"""The host/device arithmetic of the volume distance kernels (ust-run_amd/csrc/edt3d_plan.h: the limits and the overflow bound, the
percentile ranks, the grid folding, the radix digits of the select, and the two searches along x and along z) is pinned on the CPU:
tests/host/edt3d_plan_check.hip is compiled host-only and replays the kernels' passes in their order over small volumes, weights up
to 255 and values past 2^30, against a brute force in 64-bit integers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_edt3d_plan_helpers_equal_a_brute_force(tmp_path):
    exe = str(tmp_path / "edt3d_plan_check")
    src = os.path.join(ROOT, "tests", "host", "edt3d_plan_check.hip")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout and "7 shapes x 6 weights" in r.stdout
