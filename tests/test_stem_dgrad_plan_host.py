"""The tap and parity arithmetic of the stem convolution's input gradient (ust-run_amd/csrc/stem_dgrad_plan.h) is pinned on the CPU:
tests/host/stem_dgrad_plan_check.hip is compiled host-only and repeats the kernel's walk (tile -> quad -> parity -> offset -> tap -> patch
index) for every H, W in 1..40 and every tile origin.  Each input pixel's taps inside the output map must be exactly those of the
convolution's definition, each reading the output the definition names; every index walked must lie inside the patch the plan declares;
the tiles must cover every pixel once.  The header's constants are then compared with the ones the GPU test imports."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_stem_dgrad_plan_equals_brute_force(tmp_path):
    exe = str(tmp_path / "stem_dgrad_plan_check")
    src = os.path.join(ROOT, "tests", "host", "stem_dgrad_plan_check.hip")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout and "FAIL" not in r.stdout
    m = re.search(r"sweep: H, W = 1\.\.40, tile (\d+), patch (\d+): (\d+) pixels, (\d+) taps inside the map, (\d+) indices walked, (\d+) of them outside",
                  r.stdout)
    assert m, r.stdout
    tile, patch, pixels, taps, walked, outside = (int(v) for v in m.groups())
    assert pixels == 820 * 820 and taps > pixels and outside > 0 and walked >= taps + outside
    assert patch == tile // 2 + 3
    hdr = open(os.path.join(ROOT, "ust-run_amd", "csrc", "stem_dgrad_plan.h")).read()
    assert int(re.search(r"constexpr int SD_T = (\d+);", hdr).group(1)) == tile
    from test_gpu_deeplab_input_grad import TILE
    assert TILE == tile


def test_entry_point_is_declared_bound_and_refuses_before_any_launch():
    from ustrun import _lib
    hdr = open(os.path.join(ROOT, "include", "ustrun.h")).read()
    assert re.search(r"\bint\s+ustrun_conv_stem_dgrad\s*\(", hdr) and "resnet.py:124,160" in hdr
    assert len(_lib.SIGNATURES["ustrun_conv_stem_dgrad"][1]) == 10
    h = _lib.lib()
    rc = h.ustrun_conv_stem_dgrad(None, None, 1, 8, 8, 8, 4, None, 0, None)       # argument checks fail before any launch
    assert rc != 0 and b"conv_stem_dgrad" in h.ustrun_last_error() and b"Cin=4" in h.ustrun_last_error()
    rc = h.ustrun_conv_stem_dgrad(None, None, 1, 8, 8, 72, 3, None, 0, None)
    assert rc != 0 and b"Cout=72" in h.ustrun_last_error()
