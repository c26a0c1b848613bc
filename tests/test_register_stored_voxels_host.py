"""Voxel maps whose members are stored clouds (sgtd_register_stored_voxels) without a device: the header's prototypes, the
library's exports, the ctypes binding, the argument errors that need no device, and the manager's own argument checks,
which come before the library is called."""
import ctypes
import os
import re

import numpy as np
import pytest

from sgtd_amd import _lib, manager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_register_stored_voxels": ["sgtd_handle h", "const sgtd_voxel_register_options *opt", "const float *points", "int stride_floats",
                                    "const int64_t *pt_off", "int n_clouds", "const int32_t *map_off", "const uint32_t *map_frame",
                                    "const double *map_pose", "int n_maps", "const int32_t *src_cloud", "const int32_t *tgt_map",
                                    "const double *init_pose", "int n_pairs", "int device_ptrs"],
    "sgtd_result_stored_voxel_registered": ["sgtd_handle h", "double *pose", "double *fitness", "double *cost", "int32_t *n_matched", "int32_t *n_corr",
                                            "int32_t *iterations", "int32_t *status"],
    "sgtd_result_stored_voxel_map": ["sgtd_handle h", "int map", "int32_t *coord", "int32_t *n_points", "double *mean", "double *cov",
                                     "int64_t capacity", "int64_t *n"],
    "sgtd_result_stored_voxel_matches": ["sgtd_handle h", "int pair", "int32_t *voxel", "int64_t capacity", "int64_t *n"],
    "sgtd_stored_voxel_register_stage_ms": ["sgtd_handle h", "float *ms_cov", "float *ms_map", "float *ms_corr", "float *ms_rest", "float *ms_total"],
    "sgtd_register_stored_local_loops": ["sgtd_handle h", "const sgtd_voxel_register_options *opt", "const float *points", "int stride_floats",
                                         "const int64_t *pt_off", "int max_per_query", "int start", "double radius", "int max_members", "int device_ptrs"],
    "sgtd_result_stored_local_pairs": ["sgtd_handle h", "int32_t *query", "int32_t *cand", "int32_t *frame", "int32_t *tgt_map", "double *init",
                                       "int64_t capacity", "int64_t *n"],
    "sgtd_result_stored_local_maps": ["sgtd_handle h", "uint32_t *map_frame", "int64_t *mem_off", "uint32_t *member", "double *member_pose",
                                      "int64_t cap_maps", "int64_t cap_members", "int64_t *n_maps", "int64_t *n_members"],
}
# the getters mirror sgtd_register_voxels': the same parameters under the other name
MIRRORS = {"sgtd_result_stored_voxel_registered": "sgtd_result_voxel_registered", "sgtd_result_stored_voxel_map": "sgtd_result_voxel_map",
           "sgtd_result_stored_voxel_matches": "sgtd_result_voxel_matches", "sgtd_stored_voxel_register_stage_ms": "sgtd_voxel_register_stage_ms"}


def _params(header, name):
    m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, name + " is not declared"
    text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    return [" ".join(a.split()) for a in text.split(",")]


def test_header_declares_the_calls():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    for name, want in DECLS.items():
        assert _params(header, name) == want, name
    for name, other in MIRRORS.items():
        assert _params(header, name) == _params(header, other), name
    # the caps are sgtd_register_voxels' own
    for define in ("SGTD_VREG_MAX_MAPS 65535", r"SGTD_VREG_MAX_MEMBER_POINTS \(1 << 25\)", r"SGTD_VREG_MAX_CORR \(1 << 26\)"):
        assert re.search(r"^#define\s+" + define, header, re.M), define


def test_library_exports_and_binding():
    L = _lib.lib()
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    opt = ctypes.POINTER(_lib.VoxelRegisterOptions)
    want = {
        "sgtd_register_stored_voxels": [vp, opt, vp, ci, vp, ci, vp, vp, vp, ci, vp, vp, vp, ci, ci],
        "sgtd_result_stored_voxel_registered": [vp] * 8,
        "sgtd_result_stored_voxel_map": [vp, ci, vp, vp, vp, vp, i64, ctypes.POINTER(i64)],
        "sgtd_result_stored_voxel_matches": [vp, ci, vp, i64, ctypes.POINTER(i64)],
        "sgtd_stored_voxel_register_stage_ms": [vp] + [ctypes.POINTER(ctypes.c_float)] * 5,
        "sgtd_register_stored_local_loops": [vp, opt, vp, ci, vp, ci, ci, ctypes.c_double, ci, ci],
        "sgtd_result_stored_local_pairs": [vp, vp, vp, vp, vp, vp, i64, ctypes.POINTER(i64)],
        "sgtd_result_stored_local_maps": [vp, vp, vp, vp, vp, i64, i64, ctypes.POINTER(i64), ctypes.POINTER(i64)],
    }
    assert set(want) == set(DECLS)
    for name, types in want.items():
        assert name in _lib.SYMBOLS, name
        f = getattr(L, name)      # (AttributeError: the library does not export it)
        assert f.argtypes == types and len(types) == len(DECLS[name]) and f.restype is ctypes.c_int, name
    for name, other in MIRRORS.items():
        assert getattr(L, name).argtypes == getattr(L, other).argtypes, name


def test_a_null_handle_is_invalid_everywhere():
    L = _lib.lib()
    vp = ctypes.c_void_p
    off = np.array([0, 1], np.int64)
    moff = np.array([0, 1], np.int32)
    ids = np.zeros(1, np.uint32)
    idx = np.zeros(1, np.int32)
    pts = np.zeros((1, 3), np.float32)
    n = ctypes.c_int64(5)
    p = lambda a: a.ctypes.data_as(vp)      # noqa: E731
    assert L.sgtd_register_stored_voxels(None, None, p(pts), 3, p(off), 1, p(moff), p(ids), None, 1, p(idx), p(idx), None, 1, 0) == -1
    assert L.sgtd_register_stored_voxels(None, None, None, 3, None, 0, None, None, None, 0, None, None, None, 0, 0) == -1
    assert L.sgtd_result_stored_voxel_registered(None, None, None, None, None, None, None, None) == -1
    assert L.sgtd_result_stored_voxel_map(None, 0, None, None, None, None, 0, ctypes.byref(n)) == -1 and n.value == 5
    assert L.sgtd_result_stored_voxel_matches(None, 0, None, 0, ctypes.byref(n)) == -1 and n.value == 5
    assert L.sgtd_stored_voxel_register_stage_ms(None, None, None, None, None, None) == -1
    assert L.sgtd_register_stored_local_loops(None, None, p(pts), 3, p(off), 1, 0, 15.0, 0, 0) == -1
    assert L.sgtd_result_stored_local_pairs(None, None, None, None, None, None, 0, ctypes.byref(n)) == -1 and n.value == 5
    assert L.sgtd_result_stored_local_maps(None, None, None, None, None, 0, 0, ctypes.byref(n), ctypes.byref(n)) == -1 and n.value == 5


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
    off = np.array([0, 5], np.int64)
    bad = [
        dict(points=np.zeros((5, 2), np.float32)), dict(points=np.zeros(5, np.float32)), dict(pt_off=[]), dict(pt_off=[0, 6]),
        dict(map_off=[]), dict(map_off=[0, 3]),                              # more members than were given
        dict(map_frame=[-1, 4]), dict(map_frame=[0.5, 4]), dict(map_frame=[1 << 32, 4]),
        dict(map_pose=np.zeros((3, 12))), dict(map_pose=np.zeros((1, 12))),
        dict(tgt_map=[0, 0]), dict(src=[0, 0]), dict(init=np.zeros((2, 12))),
    ]
    for kw in bad:
        arg = dict(points=a, pt_off=off, map_off=[0, 2], map_frame=[3, 4], map_pose=None, src=[0], tgt_map=[0])
        arg.update(kw)
        with pytest.raises(ValueError):
            h.register_stored_voxels(**arg)
    with pytest.raises(TypeError):
        h._L = type("L", (), {"sgtd_default_voxel_register_options": staticmethod(lambda o: None)})()
        h.register_stored_voxels(a, off, [0, 2], [3, 4], None, [0], [0], no_such_option=1)
    with pytest.raises(TypeError):
        h.register_stored_voxels(a, off, [0, 2], [3, 4], None, [0], [0], max_corr_dist=1.0)      # (the dense calls' option)
    h._L = _NoLibrary()
    qoff = np.array([0, 2, 5], np.int64)
    bad_loops = [
        dict(start="icp"), dict(max_per_query=-1), dict(max_per_query=1.5), dict(max_per_query=True),
        dict(max_members=-1), dict(max_members=2.0), dict(max_members=False),
        dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(radius="far"), dict(radius=True),
        dict(query_points=np.zeros((5, 5), np.float32)), dict(query_pt_off=[0, 5]), dict(query_pt_off=[0, 2, 6]),
    ]
    for kw in bad_loops:
        arg = dict(query_points=a, query_pt_off=qoff)
        arg.update(kw)
        with pytest.raises(ValueError):
            h.register_loops_local_stored(**arg)
    with pytest.raises(TypeError):
        h._L = type("L", (), {"sgtd_default_voxel_register_options": staticmethod(lambda o: None)})()
        h.register_loops_local_stored(a, qoff, no_such_option=1)


# ---- the numpy restatement of the forming rule (tests/_stored_voxel_ref.py) against the rules it is made of ----
def _poses(n, seed, grid):
    """n stored poses (12 f32, row-major 3x4) whose translations lie on a grid of `grid` metres: distances repeat, and every
    d2 is exact in f64 whatever the order of its sums"""
    import _register_ref as ref
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 3, 4), np.float32)
    for k in range(n):
        p[k, :, :3] = ref.rot_axis(rng.normal(0, 1, 3), rng.uniform(-0.5, 0.5))
        p[k, :, 3] = rng.integers(-6, 7, 3) * grid
    return p.reshape(n, 12)


def test_the_restated_members_are_the_local_map_rule():
    import _local_map_ref as lm
    import _stored_voxel_ref as sv
    for seed, grid in ((1, 1.0), (2, 0.5), (3, 2.0)):
        poses = _poses(40, seed, grid)
        stored = {i: poses[i] for i in range(40)}
        elig = sv.eligible(set(range(40)), stored)
        assert elig == list(range(40))
        cut = 0
        for j in (0, 7, 39):
            for radius in (0.0, 3.0 * grid, 5.0 * grid, 100.0):
                for m in (0, 1, 2, 5, 40):
                    got = sv.members(j, elig, stored, radius, m)
                    assert got == lm.members(poses, j, radius, m), (seed, j, radius, m)
                    cut += m > 0 and len(got) == m < len(sv.members(j, elig, stored, radius, 0))
                # the poses: the identity for j, mul(inv(T_j), T_i) as the local-map rule composes it
                mem = sv.members(j, elig, stored, radius, 0)
                rel = sv.member_poses(mem, stored)
                assert rel[0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
                for k in range(1, len(mem)):
                    r, t = lm.mul(lm.inv(lm.rt(poses[j])), lm.rt(poses[mem[k]]))
                    assert np.array_equal(rel[k], np.concatenate([r.reshape(9), t])), (seed, j, radius, k)
        assert cut > 5, "the cut never took effect"
    # frames that are not eligible are no members, whatever their distance
    poses = _poses(12, 4, 1.0)
    stored = {i: poses[i] for i in range(12) if i != 5}
    stored[8] = poses[8].copy()
    stored[8][6] = np.inf
    elig = sv.eligible(set(range(12)) - {3}, stored)
    assert elig == [0, 1, 2, 4, 6, 7, 9, 10, 11]
    assert sv.members(0, elig, stored, 100.0) == elig


def test_the_restated_membership_is_voxel_map_members_without_a_cap():
    import _stored_voxel_ref as sv
    poses = _poses(30, 9, 1.0)
    stored = {i: poses[i] for i in range(30) if i % 7 != 3}
    has_cloud = set(range(30)) - {4, 11}
    elig = sv.eligible(has_cloud, stored)
    frame_poses = {i: sv.widen(stored[i]) for i in stored}
    several = 0
    for j in elig[::3]:
        for radius in (0.0, 4.0, 7.0, 50.0):
            got = sv.members(j, elig, stored, radius, 0)
            mem, rel = manager.STDescManager.voxel_map_members(j, frame_poses, lambda i: i in has_cloud, radius, 0)
            assert got == mem.tolist(), (j, radius)      # (membership only: that function composes its poses with @)
            several += len(got) > 1
    assert several > 5
