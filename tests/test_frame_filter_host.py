"""sgtd_set_frame_filter (per-query frame filters) at the ABI boundary and in the Python layer, without a GPU: the
header declares it, the library exports it, the ctypes binding passes the declared types, the argument checks run
before anything touches a device, the manager packs its rows bit for bit, and evaluate.frames_near agrees with a
brute-force distance check."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sgtd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_set_frame_filter():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    m = re.search(r"int\s+sgtd_set_frame_filter\s*\(([^;]*)\)\s*;", header)
    assert m, "sgtd_set_frame_filter is not declared"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args == ["sgtd_handle h", "uint32_t frame_lo", "uint32_t n_frames", "const uint64_t *rows", "int n_rows"]
    assert "sgtd_set_frame_filter" in _lib.SYMBOLS


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm is not installed")
def test_library_exports_set_frame_filter():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sgtd_set_frame_filter$", out, re.M)


def test_binding_argument_checks():
    L = _lib.lib()
    f = L.sgtd_set_frame_filter
    assert f.argtypes == [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int]
    assert f.restype is ctypes.c_int
    rows = np.ones(4, np.uint64)
    # a NULL handle, in every form (the clearing one included): SGTD_ERR_INVALID
    assert f(None, 0, 64, rows.ctypes.data, 1) == -1
    assert f(None, 0, 0, None, 0) == -1
    assert f(None, 0, 64, rows.ctypes.data, -1) == -1
    assert f(None, 0, 64, None, 2) == -1
    assert f(None, 0, 0, rows.ctypes.data, 1) == -1


def _unpack(lo, n, rows):
    """the frame ids each packed row allows"""
    bits = np.unpackbits(rows.astype("<u8").view(np.uint8).reshape(rows.shape[0], -1), axis=1, bitorder="little")
    assert not bits[:, n:].any(), "bits beyond n_frames"
    return [lo + np.flatnonzero(b[:n]) for b in bits]


def test_pack_shared_ids():
    from sgtd_amd.manager import pack_frame_rows
    lo, n, rows = pack_frame_rows(np.array([5, 7, 70, 5]))
    assert (lo, n) == (5, 66) and rows.dtype == np.uint64 and rows.shape == (1, 2)
    # little-endian bit order: frame 5 is bit 0 of word 0, frame 7 bit 2, frame 70 bit 1 of word 1
    assert rows[0, 0] == (1 << 0) | (1 << 2) and rows[0, 1] == 1 << 1
    assert [list(r) for r in _unpack(lo, n, rows)] == [[5, 7, 70]]
    # an explicit range: the word count follows n_frames, ids outside it are dropped
    lo, n, rows = pack_frame_rows([3, 64, 130, 200], frame_lo=0, n_frames=129)
    assert (lo, n) == (0, 129) and rows.shape == (1, 3)
    assert [list(r) for r in _unpack(lo, n, rows)] == [[3, 64]]
    # exactly 64 frames: one word, the top bit set
    lo, n, rows = pack_frame_rows([0, 63])
    assert (lo, n) == (0, 64) and rows.shape == (1, 1) and rows[0, 0] == np.uint64((1 << 63) | 1)
    # an empty set allows nothing (and is still a valid filter)
    lo, n, rows = pack_frame_rows([])
    assert n >= 1 and rows.shape[0] == 1 and not rows.any()


def test_pack_per_query_rows_and_matrix():
    from sgtd_amd.manager import pack_frame_rows
    sets = [np.array([10, 11]), np.array([], np.int64), np.array([140, 12, 75])]
    lo, n, rows = pack_frame_rows(sets)
    assert (lo, n) == (10, 131) and rows.shape == (3, 3)
    assert [sorted(r.tolist()) for r in _unpack(lo, n, rows)] == [[10, 11], [], [12, 75, 140]]
    rng = np.random.default_rng(3)
    mat = rng.random((5, 200)) < 0.3
    lo, n, rows = pack_frame_rows(mat)
    assert (lo, n) == (0, 200) and rows.shape == (5, 4)
    for r, ids in enumerate(_unpack(lo, n, rows)):
        assert np.array_equal(ids, np.flatnonzero(mat[r]))
    lo, n, rows = pack_frame_rows(mat, frame_lo=1000)
    for r, ids in enumerate(_unpack(lo, n, rows)):
        assert np.array_equal(ids, 1000 + np.flatnonzero(mat[r]))
    # a random shared set, against a bit-by-bit reference
    ids = np.unique(rng.integers(3, 4000, 500))
    lo, n, rows = pack_frame_rows(ids)
    ref = np.zeros(rows.shape[1], np.uint64)
    for f in ids:
        d = int(f) - lo
        ref[d >> 6] |= np.uint64(1 << (d & 63))
    assert np.array_equal(rows[0], ref)


def test_pack_rejects_ids_outside_32_bits():
    from sgtd_amd.manager import pack_frame_rows
    for bad in ([-1], [2 ** 32], [[0], [2 ** 33]]):
        with pytest.raises(ValueError):
            pack_frame_rows(bad)
    assert pack_frame_rows([2 ** 32 - 1])[0] == 2 ** 32 - 1


def test_manager_checks_before_the_library():
    from sgtd_amd import manager
    m = manager.STDescManager.__new__(manager.STDescManager)      # (no device: the checks run before the library call)
    m._h = None
    m._L = _lib.lib()
    with pytest.raises(ValueError):
        m.set_frame_filter([-3])
    for allowed in (None, [1, 2], [[1], [2, 3]]):
        with pytest.raises(_lib.SgtdError) as ei:
            m.set_frame_filter(allowed)
        assert ei.value.status == -1


def test_frames_near_matches_brute_force():
    from sgtd_amd import evaluate
    rng = np.random.default_rng(5)
    map_xy = rng.uniform(-300, 300, (400, 2))
    prior = rng.uniform(-300, 300, (37, 2))
    for radius in (0.0, 10.0, 50.0, 1000.0):
        got = evaluate.frames_near(map_xy, prior, radius)
        assert got.shape == (37, 400) and got.dtype == np.bool_
        for q in range(37):
            for f in range(0, 400, 7):
                d = np.hypot(*(map_xy[f] - prior[q]))
                assert got[q, f] == (d <= radius), (q, f, radius)
    # a map frame exactly on the circle is inside
    assert evaluate.frames_near([[3.0, 4.0]], [[0.0, 0.0]], 5.0)[0, 0]
