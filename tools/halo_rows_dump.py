#!/usr/bin/env python3
"""A/B of two builds of the library on the halo plan's sweep, no GPU: reads the "rows ..." lines tests/host/halo_plan_check prints with
the argument `rows` on stdin and prints, for each launch and both 16-bit types, the statistics rows the library named by USTRUN_LIB
reports under that line's debug flags (64 -> 64 layers also with ustrun_debug_flags bit 0, which keeps them off the streaming kernel).
    halo_plan_check rows | USTRUN_LIB=<libustrun.so> python tools/halo_rows_dump.py > dump.txt"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ust-run_amd"))
from ustrun import _lib as L      # noqa: E402

lib = L.lib()
for ln in sys.stdin:
    if not ln.startswith("rows "):
        continue
    n, h, w, ci, co, dil, pooled, f1, f2, _ = (int(v) for v in ln.split()[1:])
    for keep in ((0, 1) if (ci, co) == (64, 64) else (0,)):
        lib.ustrun_debug_flags(f1 | keep)
        lib.ustrun_debug_flags2(f2)
        print(n, h, w, ci, co, dil, pooled, f1 | keep, f2, *(lib.ustrun_debug_conv_stat_rows(n, h, w, ci, co, 3, 1, dil, pooled, code) for code in (L.BF16, L.F16)))
