"""CPU-side checks of the two entry points behind `x.grad` and the feature output's gradient: declared in the header (with the
reference lines they stand for), bound in ustrun/_lib.py's table and exported by the built library."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ustrun_conv_first_dgrad", "ustrun_unet_backward_io")


def test_new_entry_points_are_declared_bound_and_exported():
    from ustrun import _lib
    hdr = open(os.path.join(ROOT, "include", "ustrun.h")).read()
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, hdr), s
        assert s in _lib.SIGNATURES, s
    assert "unet_parts.py:16" in hdr and "unet_model.py:25-39" in hdr
    # the argument counts the header promises
    assert len(_lib.SIGNATURES["ustrun_conv_first_dgrad"][1]) == 10
    assert len(_lib.SIGNATURES["ustrun_unet_backward_io"][1]) == 11
    if not os.path.exists(_lib.LIB_PATH):
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__ as g
        g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (ustrun_\w+)", out))
    assert set(NEW) <= exported, set(NEW) - exported


def test_operator_refuses_five_input_channels_before_any_launch():
    from ustrun import _lib
    h = _lib.lib()
    rc = h.ustrun_conv_first_dgrad(None, None, 1, 4, 4, 8, 5, None, 0, None)      # argument check fails before any launch
    assert rc != 0 and b"conv_first_dgrad" in h.ustrun_last_error() and b"Cin=5" in h.ustrun_last_error()
