"""The plan and the cursor of the 64 -> 64 streaming convolution (ust-run_amd/csrc/ws64_walk.h) are pinned on the CPU:
tests/host/ws64_walk_check.hip is compiled host-only and checks, over N x width x height sweeps, that a block's counting walk equals
fresh division-based decodes and ends, that the uniform plan's segments tile every strip, and that the flat plan's pieces cover every
(strip, 8-row step) exactly once, run consecutively inside a block, and take distinct statistics slots inside the buffer."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_ws64_plan_and_cursor_exact_on_their_domains(tmp_path):
    exe = str(tmp_path / "ws64_walk_check")
    src = os.path.join(ROOT, "tests", "host", "ws64_walk_check.hip")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
    for part in ("uniform plan: N = 1..40 x 5 widths x 7 heights", "flat plan: N = 1..300 x 5 widths x 7 heights + 2 pinned shapes",
                 "plan invariants:"):
        assert part in r.stdout, part
    flat = int(re.search(r"(\d+) took the flat plan", r.stdout).group(1))
    assert flat > 0, "the sweep never reached the flat plan"
