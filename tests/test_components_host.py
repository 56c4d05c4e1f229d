"""The host/device helpers of connected-component labelling (ust-run_amd/csrc/components.h: find, unite, the neighbour rules, the
tiles, the border-pair enumeration, the filter predicate) are pinned on the CPU: tests/host/components_check.hip is compiled
host-only and replays the kernels' order (tile-local merges, border pairs, flatten) sequentially, with the kernel's tile constants,
over the planes the GPU tests use, against a flood fill written there; the border pairs must name every neighbour pair across a tile
edge or corner exactly once for both connectivities, at sizes that are no multiples of the tile."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_components_helpers_equal_a_flood_fill(tmp_path):
    exe = str(tmp_path / "components_check")
    src = os.path.join(ROOT, "tests", "host", "components_check.hip")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout and "planes over 13 sizes" in r.stdout
