"""The index helpers the weight-gradient kernels share (ust-run_amd/csrc/tn_gemm.h) are pinned on the CPU: tests/host/tn_index_check.hip
is compiled host-only and checks fdiv (float-reciprocal division, exact for 0 <= v < 2^24), wrap_add ((x + inc) mod W for W < 2^15,
inc <= 64) and xcd_linear (a permutation of the grid that keeps each XCD's blocks contiguous) over those whole domains, and the
tile cursor of the all-taps weight-gradient kernels (k advances from any start equal a fresh seek, in steps of one and of two tiles)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_tn_index_helpers_exact_on_their_domains(tmp_path):
    exe = str(tmp_path / "tn_index_check")
    src = os.path.join(ROOT, "tests", "host", "tn_index_check.hip")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "all checks passed" in r.stdout
    for part in ("fdiv full range: 30 divisors", "fdiv boundaries: d = 1..4096", "wrap_add: W = 1..32767", "xcd_linear: nblk = 1..4100",
                 "tile_cursor: tiles 1..8 x 1..8, N = 1 and 3, strides 1 and 2"):
        assert part in r.stdout, part
