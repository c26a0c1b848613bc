"""The cloud store and the registration against it (sgtd_set_frame_clouds, sgtd_register_stored,
sgtd_register_stored_loops) without a device: the header's prototypes, the library's exports, the ctypes binding, the
argument errors that need no device, and the manager's own argument checks, which come before the library is called."""
import ctypes
import os
import re

import numpy as np
import pytest

from sgtd_amd import _lib, manager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REG = ["sgtd_handle h", "const sgtd_register_options *opt", "const float *points", "int stride_floats", "const int64_t *pt_off"]
DECLS = {
    "sgtd_set_frame_clouds": ["sgtd_handle h", "const uint32_t *frame_ids", "const int64_t *pt_off", "const float *points", "int stride_floats",
                              "int64_t n", "int k_neighbors", "double plane_eps", "int device_ptrs"],
    "sgtd_frame_clouds_info": ["sgtd_handle h", "int64_t *n_frames", "int64_t *n_points", "int64_t *device_bytes", "int32_t *k_neighbors",
                               "double *plane_eps"],
    "sgtd_result_frame_cloud": ["sgtd_handle h", "uint32_t frame", "float *xyz", "double *cov", "int64_t capacity", "int64_t *n"],
    "sgtd_register_stored": REG + ["int n_clouds", "const int32_t *src_cloud", "const uint32_t *tgt_frame", "const double *init_pose", "int n_pairs",
                                   "int device_ptrs"],
    "sgtd_result_stored_registered": ["sgtd_handle h", "double *pose", "double *fitness", "double *cost", "int32_t *n_matched", "int32_t *iterations",
                                      "int32_t *status"],
    "sgtd_result_stored_covariances": ["sgtd_handle h", "int cloud", "double *cov", "int64_t capacity", "int64_t *n"],
    "sgtd_result_stored_matches": ["sgtd_handle h", "int pair", "int32_t *tgt_index", "double *d2", "int64_t capacity", "int64_t *n"],
    "sgtd_stored_register_stage_ms": ["sgtd_handle h", "float *ms_cov", "float *ms_search", "float *ms_rest", "float *ms_total"],
    "sgtd_register_stored_loops": REG + ["int max_per_query", "int start", "int device_ptrs"],
    "sgtd_result_stored_pairs": ["sgtd_handle h", "int32_t *query", "int32_t *cand", "int32_t *frame", "double *init", "int64_t capacity", "int64_t *n"],
}


def test_header_declares_the_calls():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    for name, want in DECLS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name + " is not declared"
        text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        assert [" ".join(a.split()) for a in text.split(",")] == want, name
    assert re.search(r"^#define\s+SGTD_CLOUD_STORE_MAX_POINTS\s+\(1 << 27\)", header, re.M)
    assert re.search(r"enum\s*\{\s*SGTD_START_VERIFY = 0, SGTD_START_REFINED = 1, SGTD_START_ALIGNED = 2\s*\}", header)


def test_library_exports_and_binding():
    L = _lib.lib()
    vp, i64, i32, ci, cd = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int, ctypes.c_double
    opt = ctypes.POINTER(_lib.RegisterOptions)
    want = {
        "sgtd_set_frame_clouds": [vp, vp, vp, vp, ci, i64, ci, cd, ci],
        "sgtd_frame_clouds_info": [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32), ctypes.POINTER(cd)],
        "sgtd_result_frame_cloud": [vp, ctypes.c_uint32, vp, vp, i64, ctypes.POINTER(i64)],
        "sgtd_register_stored": [vp, opt, vp, ci, vp, ci, vp, vp, vp, ci, ci],
        "sgtd_result_stored_registered": [vp] * 7,
        "sgtd_result_stored_covariances": [vp, ci, vp, i64, ctypes.POINTER(i64)],
        "sgtd_result_stored_matches": [vp, ci, vp, vp, i64, ctypes.POINTER(i64)],
        "sgtd_stored_register_stage_ms": [vp] + [ctypes.POINTER(ctypes.c_float)] * 4,
        "sgtd_register_stored_loops": [vp, opt, vp, ci, vp, ci, ci, ci],
        "sgtd_result_stored_pairs": [vp, vp, vp, vp, vp, i64, ctypes.POINTER(i64)],
    }
    assert set(want) == set(DECLS)
    for name, types in want.items():
        assert name in _lib.SYMBOLS, name
        f = getattr(L, name)      # (AttributeError: the library does not export it)
        assert f.argtypes == types and len(types) == len(DECLS[name]) and f.restype is ctypes.c_int, name


def test_a_null_handle_is_invalid_everywhere():
    L = _lib.lib()
    vp = ctypes.c_void_p
    off = np.zeros(2, np.int64)
    ids = np.zeros(1, np.uint32)
    pts = np.zeros((1, 3), np.float32)
    n = ctypes.c_int64(5)
    p = lambda a: a.ctypes.data_as(vp)      # noqa: E731
    assert L.sgtd_set_frame_clouds(None, p(ids), p(off), p(pts), 3, 1, 20, 1e-3, 0) == -1
    assert L.sgtd_set_frame_clouds(None, None, None, None, 3, 0, 0, 0.0, 0) == -1
    assert L.sgtd_frame_clouds_info(None, None, None, None, None, None) == -1
    assert L.sgtd_result_frame_cloud(None, 0, None, None, 0, ctypes.byref(n)) == -1 and n.value == 5
    assert L.sgtd_register_stored(None, None, p(pts), 3, p(off), 1, None, None, None, 0, 0) == -1
    assert L.sgtd_result_stored_registered(None, None, None, None, None, None, None) == -1
    assert L.sgtd_result_stored_covariances(None, 0, None, 0, None) == -1
    assert L.sgtd_result_stored_matches(None, 0, None, None, 0, None) == -1
    assert L.sgtd_stored_register_stage_ms(None, None, None, None, None) == -1
    assert L.sgtd_register_stored_loops(None, None, p(pts), 3, p(off), 1, 0, 0) == -1
    assert L.sgtd_result_stored_pairs(None, None, None, None, None, 0, None) == -1


class _NoLibrary:
    """stands where the library would: any call of it fails the test"""
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


@pytest.fixture
def h():
    m = manager.STDescManager.__new__(manager.STDescManager)
    m._L, m._h, m._nq = _NoLibrary(), None, 2
    return m


def test_manager_rejects_bad_arguments_before_the_library(h):
    a = np.zeros((5, 3), np.float32)
    bad_set = [
        dict(frames=None, clouds=[a]),                               # forget-all takes no clouds
        dict(frames=[0, 1], clouds=[a]),                             # one cloud per id
        dict(frames=[-1], clouds=[a]), dict(frames=[0.5], clouds=[a]), dict(frames=[1 << 32], clouds=[a]),
        dict(frames=[0], clouds=[np.zeros((5, 2), np.float32)]), dict(frames=[0], clouds=[np.zeros(5, np.float32)]),
        dict(frames=[0, 1], clouds=[a, np.zeros((5, 4), np.float32)]),      # one width
        dict(frames=[0], clouds=(a, np.array([0, 6]))),              # more points than given
        dict(frames=[0], clouds=(a, np.array([1, 5]))), dict(frames=[0, 1], clouds=(a, np.array([0, 4, 3]))),
        dict(frames=[0], clouds=[a], k_neighbors=2), dict(frames=[0], clouds=[a], k_neighbors=33), dict(frames=[0], clouds=[a], k_neighbors=True),
        dict(frames=[0], clouds=[a], plane_eps=0.0), dict(frames=[0], clouds=[a], plane_eps=np.nan), dict(frames=[0], clouds=[a], plane_eps=np.inf),
    ]
    for kw in bad_set:
        with pytest.raises(ValueError):
            h.set_frame_clouds(**kw)
    off = np.array([0, 5], np.int64)
    bad_reg = [
        dict(points=np.zeros((5, 2), np.float32)), dict(points=np.zeros(5, np.float32)), dict(pt_off=[]), dict(pt_off=[0, 6]),
        dict(tgt_frame=[0, 1]), dict(tgt_frame=[-1]), dict(init=np.zeros((2, 12))),
    ]
    for kw in bad_reg:
        arg = dict(points=a, pt_off=off, src=[0], tgt_frame=[3])
        arg.update(kw)
        with pytest.raises(ValueError):
            h.register_stored(**arg)
    with pytest.raises(TypeError):
        h._L = type("L", (), {"sgtd_default_register_options": staticmethod(lambda o: None)})()
        h.register_stored(a, off, [0], [3], no_such_option=1)
    h._L = _NoLibrary()
    qoff = np.array([0, 2, 5], np.int64)
    bad_loops = [
        dict(start="icp"), dict(max_per_query=-1), dict(max_per_query=1.5), dict(max_per_query=True),
        dict(query_points=np.zeros((5, 5), np.float32)), dict(query_pt_off=[0, 5]), dict(query_pt_off=[0, 2, 6]),
    ]
    for kw in bad_loops:
        arg = dict(query_points=a, query_pt_off=qoff)
        arg.update(kw)
        with pytest.raises(ValueError):
            h.register_loops_stored(**arg)
