"""sgtd_remove_frames (taking frames out of a built table) at the ABI boundary, without a GPU: the header declares it,
the built library exports it, the ctypes binding passes its arguments with the declared types and the argument checks
run before anything touches a device."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sgtd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_remove_frames():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    m = re.search(r"int\s+sgtd_remove_frames\s*\(([^;]*)\)\s*;", header)
    assert m, "sgtd_remove_frames is not declared"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["sgtd_handle h", "const uint32_t *frame_ids", "int64_t n", "int64_t *n_removed"]
    assert "sgtd_remove_frames" in _lib.SYMBOLS


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm is not installed")
def test_library_exports_remove_frames():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sgtd_remove_frames$", out, re.M)


def test_binding_argument_checks():
    L = _lib.lib()
    f = L.sgtd_remove_frames
    assert f.argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    assert f.restype is ctypes.c_int
    ids = np.array([1, 2, 3], np.uint32)
    n = ctypes.c_int64(123)
    # a NULL handle: SGTD_ERR_INVALID, and *n_removed is 0
    assert f(None, ids.ctypes.data, 3, ctypes.byref(n)) == -1 and n.value == 0
    assert f(None, None, 0, None) == -1
    assert f(None, ids.ctypes.data, -1, None) == -1
    assert f(None, None, 3, None) == -1


def test_manager_rejects_ids_outside_32_bits():
    from sgtd_amd import manager
    m = manager.STDescManager.__new__(manager.STDescManager)      # (no device: the check runs before the library call)
    m._h = None
    m._L = _lib.lib()
    for bad in ([-1], [2 ** 32]):
        with pytest.raises(ValueError):
            m.remove_frames(bad)
    with pytest.raises(_lib.SgtdError) as ei:
        m.remove_frames([5, 6])
    assert ei.value.status == -1
