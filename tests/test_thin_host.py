"""Voxel-grid thinning on the device (sgtd_thin_clouds) without a device: the header's prototypes, the library's exports, the
ctypes binding, the argument errors that need no device, the manager's own argument checks, which come before the library is
called, and the numpy restatement of the rule (tests/_thin_ref.py) against ingest.voxel_downsample."""
import ctypes
import os
import re

import numpy as np
import pytest

import _thin_ref as tr
from sgtd_amd import _lib, ingest, manager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_thin_clouds": ["sgtd_handle h", "const float *points", "int stride_floats", "const int64_t *pt_off", "int n_clouds", "double leaf",
                         "int device_ptrs"],
    "sgtd_result_thinned": ["sgtd_handle h", "int64_t *out_off", "float *points", "int32_t *n_dropped", "int64_t capacity", "int64_t *n"],
    "sgtd_thinned_device_view": ["sgtd_handle h", "const float **d_points", "int *stride_floats", "int64_t *n_points"],
    "sgtd_thin_stage_ms": ["sgtd_handle h", "float *ms_sort", "float *ms_rest", "float *ms_total"],
}


def _params(header, name):
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, name + " is not declared"
    text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    return [" ".join(a.split()) for a in text.split(",")]


def test_header_declares_the_calls():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    for name, want in DECLS.items():
        assert _params(header, name) == want, name
    assert re.search(r"^#define\s+SGTD_THIN_MAX_CELL \(1 << 20\)", header, re.M)
    assert tr.MAX_CELL == 1 << 20


def test_library_exports_and_binding():
    L = _lib.lib()
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    want = {
        "sgtd_thin_clouds": [vp, vp, ci, vp, ci, ctypes.c_double, ci],
        "sgtd_result_thinned": [vp, vp, vp, vp, i64, ctypes.POINTER(i64)],
        "sgtd_thinned_device_view": [vp, ctypes.POINTER(vp), ctypes.POINTER(ci), ctypes.POINTER(i64)],
        "sgtd_thin_stage_ms": [vp] + [ctypes.POINTER(ctypes.c_float)] * 3,
    }
    assert set(want) == set(DECLS)
    for name, types in want.items():
        assert name in _lib.SYMBOLS, name
        f = getattr(L, name)      # (AttributeError: the library does not export it)
        assert f.argtypes == types and len(types) == len(DECLS[name]) and f.restype is ctypes.c_int, name


def test_a_null_handle_is_invalid_everywhere():
    L = _lib.lib()
    vp = ctypes.c_void_p
    off = np.array([0, 1], np.int64)
    pts = np.zeros((1, 3), np.float32)
    n = ctypes.c_int64(5)
    p = lambda a: a.ctypes.data_as(vp)      # noqa: E731
    assert L.sgtd_thin_clouds(None, p(pts), 3, p(off), 1, 0.25, 0) == -1
    assert L.sgtd_thin_clouds(None, None, 3, None, 0, 0.25, 0) == -1
    assert L.sgtd_result_thinned(None, None, None, None, 0, ctypes.byref(n)) == -1 and n.value == 5
    assert L.sgtd_thinned_device_view(None, None, None, ctypes.byref(n)) == -1 and n.value == 5
    assert L.sgtd_thin_stage_ms(None, None, None, None) == -1


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
    off = np.array([0, 2, 5], np.int64)
    bad = [
        dict(points=np.zeros((5, 2), np.float32)), dict(points=np.zeros(5, np.float32)), dict(points=np.zeros((5, 5), np.float32)),
        dict(leaf=0), dict(leaf=0.0), dict(leaf=-0.25), dict(leaf=np.nan), dict(leaf=np.inf), dict(leaf="small"), dict(leaf=True), dict(leaf=None),
        dict(pt_off=[0, 3, 2]), dict(pt_off=[5, 2, 0]), dict(pt_off=[1, 5]), dict(pt_off=[0, 6]), dict(pt_off=[]),
        dict(points=np.zeros((2, 5, 3), np.float32)),      # (S, N, 3) and offsets: one or the other
    ]
    for kw in bad:
        arg = dict(points=a, pt_off=off, leaf=0.25)
        arg.update(kw)
        with pytest.raises(ValueError):
            h.thin_clouds(**arg)
    # the forms that thin first check the same things, before the library
    for kw in (dict(leaf=0.0), dict(leaf=np.nan), dict(leaf=np.inf), dict(points=np.zeros((5, 2), np.float32)), dict(pt_off=[0, 3, 2])):
        arg = dict(points=a, pt_off=off, leaf=0.25)
        arg.update(kw)
        with pytest.raises(ValueError):
            h.set_frame_scans([3, 4], (arg["points"], np.asarray(arg["pt_off"], np.int64)), arg["leaf"])
        with pytest.raises(ValueError):
            h.register_stored(arg["points"], arg["pt_off"], [0], [3], leaf=arg["leaf"])
        with pytest.raises(ValueError):
            h.register_stored_voxels(arg["points"], arg["pt_off"], [0, 1], [3], None, [0], [0], leaf=arg["leaf"])
        with pytest.raises(ValueError):
            h.register_loops_stored(arg["points"], arg["pt_off"], leaf=arg["leaf"])
        with pytest.raises(ValueError):
            h.register_loops_local_stored(arg["points"], arg["pt_off"], leaf=arg["leaf"])
    with pytest.raises(ValueError):
        h.set_frame_scans([3], (a, off), 0.25)                   # two scans, one frame id
    with pytest.raises(ValueError):
        h.register_loops_stored(a, [0, 5], leaf=0.25)            # one cloud per query of the batch (2)


def test_device_points_is_what_the_device_paths_take(h):
    d = manager.DevicePoints(4096, 4, 7)
    assert d.data_ptr() == 4096 and d.shape == (7, 4) and d.ndim == 2 and d.is_cuda and d.is_contiguous() and len(d) == 7
    shape, pp, dev = h._points_arg(d)
    assert shape == (7, 4) and pp.value == 4096 and dev == 1


def _random_cloud(rng, n, stride, spread=6.0):
    p = rng.uniform(-spread, spread, (n, stride)).astype(np.float32)
    p[rng.integers(0, n, n // 10), :3] = rng.integers(-8, 8, (n // 10, 3)).astype(np.float32) * 0.25      # on cell faces
    return p


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("stride", [3, 4])
def test_the_restatement_is_the_host_function(stride):
    rng = np.random.default_rng(40 + stride)
    for n, leaf in ((1, 0.25), (700, 0.25), (1500, 1.0), (1200, 0.1), (900, 3.0)):
        p = _random_cloud(rng, n, stride)
        if n > 10:
            p[rng.integers(0, n, 5), rng.integers(0, 3, 5)] = np.nan
            p[7, 1] = np.inf
            p[9, 2] = -np.inf
            if stride == 4:
                p[11, 3] = 2.5      # (a finite fourth column only: the host function sums whatever it holds)
        got, (n_bad, n_out) = tr.thin_cloud(p, leaf)
        want = ingest.voxel_downsample(p, leaf)
        assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (n, leaf)
        assert n_out == 0 and n_bad == int((~np.isfinite(p[:, :3]).all(axis=1)).sum())
        assert n == 1 or ((p[:, :3] < 0).any() and len(got) < n)
    # a batch is its clouds one by one
    p = _random_cloud(rng, 600, stride)
    off = np.array([0, 250, 250, 251, 600], np.int64)
    out = tr.thin(p, off, 0.5)
    for s in range(4):
        want = ingest.voxel_downsample(p[off[s]:off[s + 1]], 0.5)
        assert np.array_equal(_bits(out["points"][out["pt_off"][s]:out["pt_off"][s + 1]]), _bits(want)), s
    assert out["n_dropped"].shape == (4, 2) and not out["n_dropped"].any()


def test_the_restatement_differs_by_the_out_of_range_points_alone():
    rng = np.random.default_rng(5)
    p = _random_cloud(rng, 400, 3)
    far = p.copy()
    far[50] = [3e6, 0.0, 0.0]                      # cell 3 000 000 >= 2^20 at leaf 1.0
    far[51] = [0.0, -1048577.0, 0.0]               # cell -2^20 - 1
    far[52] = [0.0, 0.0, 1048576.0]                # cell 2^20
    far[53] = [1048575.5, -1048576.0, 0.5]         # cells 2^20 - 1 and -2^20: inside
    far[54] = [3e12, 0.0, 0.0]
    got, (n_bad, n_out) = tr.thin_cloud(far, 1.0)
    assert (n_bad, n_out) == (0, 4)
    host = ingest.voxel_downsample(far, 1.0)
    assert len(host) == len(got) + 4
    keep = np.ones(400, bool)
    keep[[50, 51, 52, 54]] = False
    assert np.array_equal(_bits(got), _bits(ingest.voxel_downsample(far[keep], 1.0)))
    # ... and the host function keeps each of them as a cell of its own
    rows = {tuple(r) for r in _bits(host).tolist()}
    assert all(tuple(_bits(far[k]).tolist()) in rows for k in (50, 51, 52, 54))
    # a leaf so small that the division overflows: out of range, not an error
    tiny, (n_bad, n_out) = tr.thin_cloud(np.array([[1e30, 0, 0], [0, 0, 0]], np.float32), 1e-300)
    assert (n_bad, n_out) == (0, 1) and np.array_equal(_bits(tiny), _bits(np.zeros((1, 3), np.float32)))
