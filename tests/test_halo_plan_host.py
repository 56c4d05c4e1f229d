"""The tile plan of the 3x3 halo convolution (ust-run_amd/csrc/halo_plan.h) is pinned on the CPU: tests/host/halo_plan_check.hip is
compiled host-only and checks, over 8 batch sizes x 28 maps x 7 channel pairs x sources x dilations x pass sizes x debug flags, that every
plan names a build the dispatch instantiates with that build's LDS size, that its tiles, statistics rows and last-pass rows follow from the
build, that the rows stay inside ustrun_conv_mtiles, what the flags must switch off, and that the sweep reaches every build.  The layers
of tests/test_gpu_production_tiles.py::CASES must plan exactly the variant codes that test asserts on the GPU.  The statistics rows of
every swept launch the library's host-only query can express are then compared with what the built library reports under the same flags."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _pins():
    from test_gpu_production_tiles import CASES, variant
    pins = []
    for c in CASES:
        name, n, cs, co, h, w, G, vf, vd = c[:9]
        if not isinstance(vf, tuple):
            continue                        # the streaming 64 -> 64 kernel's cases
        fl = c[9] if len(c) > 9 else 0
        f1, f2 = fl if isinstance(fl, tuple) else (fl, 0)
        plain = name.startswith("plain_")
        pins.append("pin=" + ",".join(str(int(v)) for v in (n, cs[0], cs[1] if len(cs) == 2 else 0, co, h, w, G, plain, f1, f2,
                                                             variant(*vf, False, not plain), variant(*vd, False, False))))
    return pins


def test_halo_plan_consistent_pinned_and_equal_to_the_library(tmp_path):
    exe = str(tmp_path / "halo_plan_check")
    src = os.path.join(ROOT, "tests", "host", "halo_plan_check.hip")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    pins = _pins()
    assert len(pins) >= 30
    r = subprocess.run([exe, "rows"] + pins, capture_output=True, text=True, timeout=120)
    rows = [tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("rows ")]
    rest = "\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith("rows "))
    print(rest)
    assert r.returncode == 0, rest[-4000:] + r.stderr[-2000:]
    assert "all checks passed" in rest and "pinned: four literals" in rest and "%d pinned layers" % len(pins) in rest
    builds = [ln.split() for ln in rest.splitlines() if ln.startswith("build ")]
    assert len(builds) == 68 and all(int(b[-2]) > 0 for b in builds), "the sweep must reach every build"

    # the plan's statistics rows equal the library's (its host-only query builds the same launch), flag by flag.  64 -> 64 layers go to
    # the streaming kernel unless ustrun_debug_flags bit 0 keeps them here: a bit the halo plan does not read
    from ustrun import _lib as L
    lib = L.lib()
    assert len(rows) > 50000 and len({(r_[7], r_[8]) for r_ in rows}) == 11
    old = lib.ustrun_debug_flags(0), lib.ustrun_debug_flags2(0)
    try:
        assert lib.ustrun_debug_conv_stat_rows(8, 72, 72, 64, 64, 3, 1, 1, 0, L.BF16) == 432       # not the halo's: 216 rows here
        cur = (0, 0)
        for n, h, w, ci, co, dil, pooled, f1, f2, used in sorted(rows, key=lambda r_: r_[7:9]):
            f1 |= 1 if (ci, co) == (64, 64) else 0
            if (f1, f2) != cur:
                lib.ustrun_debug_flags(f1)
                lib.ustrun_debug_flags2(f2)
                cur = (f1, f2)
            for code in (L.BF16, L.F16):
                got = lib.ustrun_debug_conv_stat_rows(n, h, w, ci, co, 3, 1, dil, pooled, code)
                assert got == used and got <= lib.ustrun_conv_mtiles(n, h, w, co), (n, h, w, ci, co, dil, pooled, f1, f2, code, got, used)
    finally:
        lib.ustrun_debug_flags(old[0])
        lib.ustrun_debug_flags2(old[1])
