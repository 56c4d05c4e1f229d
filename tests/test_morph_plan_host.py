"""The host/device arithmetic of the chamfer-distance and morphology kernels (ust-run_amd/csrc/morph_plan.h: the row pass with its
chunk carry, the L1 recurrence and the L-inf search with the outside's candidates, the thresholds, the grid folding, the limits) is
pinned on the CPU: tests/host/morph_plan_check.hip is compiled host-only and replays the kernels' passes in their order over small
planes and volumes, at the unclipped cap and at the clipped caps of ustrun_morph, against a brute force in 64-bit integers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_morph_plan_helpers_equal_a_brute_force(tmp_path):
    exe = str(tmp_path / "morph_plan_check")
    src = os.path.join(ROOT, "tests", "host", "morph_plan_check.hip")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout and "60 boxes x 2 metrics x 2 outside x 5 caps" in r.stdout
