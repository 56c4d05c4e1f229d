"""The strip plans, the item decodes and the streaming-eligibility predicate of the first convolution (ust-run_amd/csrc/conv_first_plan.h)
are pinned on the CPU: tests/host/conv_first_plan_check.hip is compiled host-only and checks, over N = 1..96 x 7 widths x 8 heights,
that the weight gradient's plan stays inside 4096 items and 1024 slabs wherever the predicate holds, has no empty segment, and that its
items cover every (image, strip, row) exactly once; that the forward's grid is a multiple of N and its items' steps cover every row of
every strip once; what the predicate refuses; and the plans at the workload's shapes as literals.  The forward's grid of every swept
shape is then compared with the statistics-row count the built library reports for that launch, and with the bound it publishes."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_conv_first_plans_exact_on_their_domains(tmp_path):
    exe = str(tmp_path / "conv_first_plan_check")
    src = os.path.join(ROOT, "tests", "host", "conv_first_plan_check.hip")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, "rows"], capture_output=True, text=True, timeout=120)
    rows = [tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("rows ")]
    rest = "\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("rows "))
    print(rest)
    assert r.returncode == 0, rest[-4000:] + r.stderr[-2000:]
    assert "all checks passed" in rest
    for part in ("sweep: N = 1..96 x 7 widths x 8 heights, 5376 shapes", "weight gradient:", "forward:", "pinned:"):
        assert part in rest, part
    w = rest.split("weight gradient: ")[1].split()
    assert int(w[0]) > 5000 and int(w[6]) > 5000, "the sweep hardly reached the streaming kernel"
    # conv_first_stat_rows (through the library's host-only query) equals the plan's grid and stays inside ustrun_conv_mtiles
    from ustrun import _lib as L
    lib = L.lib()
    assert len(rows) == 5376
    for n, h, w_, grid in rows:
        for code in (L.BF16, L.F16):
            used = lib.ustrun_debug_conv_stat_rows(n, h, w_, 3, 64, 3, 1, 1, 0, code)
            assert used == grid and used % n == 0 and used <= lib.ustrun_conv_mtiles(n, h, w_, 64), (n, h, w_, code, used, grid)
