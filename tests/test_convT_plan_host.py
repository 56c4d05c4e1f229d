"""The plan of the pixel-linear GEMM family (ust-run_amd/csrc/convT_plan.h: ConvTranspose forward / input gradient, the 1x1 convolution with
join and sums, the ConvTranspose weight gradient) is pinned on the CPU: tests/host/convT_plan_check.hip is compiled host-only and checks, over
5 batch sizes x 11 maps (odd widths, W < 8, W < 16, W >= 32768, M % 128 != 0) x 13 channel pairs x sources x pass groupings x the two debug
flags, that every plan names a build the dispatch instantiates with that build's LDS size, that tiles, grid, statistics rows and split-K
follow from the build, that tiles and stages stay inside a pass, what the flags must switch off, and that the sweep reaches all 18 + 4 builds.
The shapes of three GPU tests must plan exactly the variant codes those tests assert.  The statistics rows of every swept 1x1 the library's
host-only query can express, and the partials bound of every swept weight gradient, are then compared with the built library's answers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _params(fn):
    return [m for m in fn.pytestmark if m.name == "parametrize"][0].args[1]


def _pins():
    import test_gpu_deeplab_tiles as D
    import test_gpu_production_tiles as T
    n, h, w = D.PROD_NHW
    pins = ["pin1x1=%d,%d,%d,%d,%d,%d,%d" % (n, h, w, ci, co, fl, want) for ci, co, fl, want in _params(D.test_conv1x1_production_tiles)]
    pins += ["pinwg=%d,%d,%d,%d,%d,%d,%d,%d,%d" % (n, ci, co, h, w, G, xf, fl, v) for _, n, ci, co, h, w, G, xf, fl, v in T.CONVT_WGRAD_CASES]
    pins += ["pindg=%d,%d,%d,%d,%d,%d,%d" % (n, G, ci, co, h, w, -1 if code is None else code)
             for _, n, G, ci, co, h, w, code in _params(T.test_convT_input_gradient_with_batchnorm_backward_sums_exact)]
    pins += ["pinct=%d,%d,%d,%d,%d,%d,%d,%d,%d" % (*c, *T.convT_batched_variants(c[6])) for c in T.CONVT_BATCHED_CASES]
    return pins


def test_convT_plan_consistent_pinned_and_equal_to_the_library(tmp_path):
    exe = str(tmp_path / "convT_plan_check")
    src = os.path.join(ROOT, "tests", "host", "convT_plan_check.hip")
    r = subprocess.run([HIPCC, "--cuda-host-only", "-O2", "-std=c++17", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    pins = _pins()
    assert len(pins) == 7 + 10 + 4 + 6
    r = subprocess.run([exe, "rows"] + pins, capture_output=True, text=True, timeout=120)
    rows = {tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("rows ")}
    wg = {tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("wg ")}
    rest = "\n".join(ln for ln in r.stdout.splitlines() if not ln.startswith(("rows ", "wg ")))
    print(rest)
    assert r.returncode == 0, rest[-4000:] + r.stderr[-2000:]
    assert "all checks passed" in rest and "pinned: three refusals" in rest and "%d pinned cases" % len(pins) in rest
    builds = [ln.split() for ln in rest.splitlines() if ln.startswith("build ")]
    assert len(builds) == 18 + 4 and all(int(b[-2]) > 0 for b in builds), "the sweep must reach every build"

    from ustrun import _lib as L
    lib = L.lib()
    # ksplit x (slab + bias row) of the planned kernel fits the published partials bound (a bound over both kernels: no flag enters it)
    assert len(wg) > 100
    for ci, co, npix, need in wg:
        assert need <= lib.ustrun_wgrad_partials_bytes(4, ci, co, npix), (ci, co, npix, need)
    # the plan's statistics rows equal the library's (its host-only query builds the same 1x1 launch), flag by flag, both 16-bit types
    assert len(rows) > 300 and {r_[5] for r_ in rows} == {0, 512, 1 << 27, 512 | 1 << 27}
    old = lib.ustrun_debug_flags(0)
    try:
        cur = 0
        for n, h, w, ci, co, fl, used in sorted(rows, key=lambda r_: r_[5]):
            if fl != cur:
                lib.ustrun_debug_flags(fl)
                cur = fl
            for code in (L.BF16, L.F16):
                got = lib.ustrun_debug_conv_stat_rows(n, h, w, ci, co, 1, 1, 1, 0, code)
                assert got == used == -(-n * h * w // 128) and got <= lib.ustrun_conv_mtiles(n, h, w, co), (n, h, w, ci, co, fl, code, got, used)
    finally:
        lib.ustrun_debug_flags(old)
