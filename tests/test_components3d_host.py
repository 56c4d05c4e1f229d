"""The third axis of connected-component labelling (ust-run_amd/csrc/components3d.h beside components.h: the pairs between adjacent
slices, their redundancy rules, the faces of a volume, the largest-component key) is pinned on the CPU:
tests/host/components3d_check.hip is compiled host-only and replays the launches' order (slice-local merges, in-plane border pairs,
z-pairs, flatten) sequentially, with the kernel's constants, over the volumes the GPU tests use, against a flood fill written there
-- unions forwards and backwards, redundant z-pairs left out and united; the z-pair enumeration must name every neighbour pair
between adjacent slices exactly once for fan 1 and fan 9, at sizes that are no multiples of the tile."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_components3d_helpers_equal_a_flood_fill(tmp_path):
    exe = str(tmp_path / "components3d_check")
    src = os.path.join(ROOT, "tests", "host", "components3d_check.hip")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout and "volumes over 10 sizes" in r.stdout
