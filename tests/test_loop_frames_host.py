"""sgtd_loop_frames (sequence loop detection) at the ABI boundary, without a GPU: the header declares it, the built
library exports it and the ctypes binding passes its arguments with the declared types."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from sgtd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_loop_frames():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    m = re.search(r"int\s+sgtd_loop_frames\s*\(([^;]*)\)\s*;", header)
    assert m, "sgtd_loop_frames is not declared"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["sgtd_handle h", "const float *xyz", "const uint32_t *label", "const int64_t *kp_off",
                    "int n_frames", "int32_t skip_near", "int device_ptrs"]
    assert "sgtd_loop_frames" in _lib.SYMBOLS


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm is not installed")
def test_library_exports_loop_frames():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sgtd_loop_frames$", out, re.M)


def test_binding_argument_types():
    L = _lib.lib()
    f = L.sgtd_loop_frames
    vp = ctypes.c_void_p
    assert f.argtypes == [vp, vp, vp, vp, ctypes.c_int, ctypes.c_int32, ctypes.c_int]
    assert f.restype is ctypes.c_int
    # a NULL handle is refused before anything touches a device
    assert f(None, None, None, None, 1, 0, 0) == -1
