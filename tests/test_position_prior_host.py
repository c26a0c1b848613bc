"""sgtd_set_frame_poses / sgtd_set_position_prior / sgtd_result_world_poses at the ABI boundary and in the Python layer,
without a GPU: the header declares them, the library exports them, the ctypes binding passes the declared types, the
argument checks run before anything touches a device, the manager rejects bad shapes before calling the library, and a
numpy restatement of the prior's row rule agrees with evaluate.frames_near (dims 2) and with brute force (dims 3)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from sgtd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_set_frame_poses": ["sgtd_handle h", "const uint32_t *frame_ids", "const float *pose12", "int64_t n"],
    "sgtd_set_position_prior": ["sgtd_handle h", "const double *center", "const double *radius", "int n_rows", "int dims"],
    "sgtd_result_world_poses": ["sgtd_handle h", "int q", "float *world"],
}


def test_header_declares_the_calls():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    for name, want in DECLS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name + " is not declared"
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert args == want, name
        assert name in _lib.SYMBOLS


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm is not installed")
def test_library_exports_the_calls():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in DECLS:
        assert re.search(r"\bT %s$" % name, out, re.M), name


def test_binding_types_and_argument_checks():
    L = _lib.lib()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert L.sgtd_set_frame_poses.argtypes == [vp, vp, vp, i64]
    assert L.sgtd_set_position_prior.argtypes == [vp, vp, vp, ctypes.c_int, ctypes.c_int]
    assert L.sgtd_result_world_poses.argtypes == [vp, ctypes.c_int, vp]
    for name in DECLS:
        assert getattr(L, name).restype is ctypes.c_int
    ids = np.arange(4, dtype=np.uint32)
    poses = np.zeros((4, 12), np.float32)
    c, r = np.zeros(6), np.ones(3)
    w = np.zeros((50, 12), np.float32)
    # a NULL handle, in every form (the forgetting and clearing ones included): SGTD_ERR_INVALID
    f = L.sgtd_set_frame_poses
    assert f(None, ids.ctypes.data, poses.ctypes.data, 4) == -1
    assert f(None, ids.ctypes.data, None, 4) == -1
    assert f(None, None, None, 0) == -1
    assert f(None, ids.ctypes.data, poses.ctypes.data, -1) == -1
    assert f(None, None, poses.ctypes.data, 4) == -1
    f = L.sgtd_set_position_prior
    assert f(None, c.ctypes.data, r.ctypes.data, 3, 2) == -1
    assert f(None, None, None, 0, 2) == -1
    assert f(None, c.ctypes.data, r.ctypes.data, -1, 2) == -1
    assert f(None, c.ctypes.data, r.ctypes.data, 1, 4) == -1
    assert f(None, None, r.ctypes.data, 1, 2) == -1
    assert L.sgtd_result_world_poses(None, 0, w.ctypes.data) == -1
    assert L.sgtd_result_world_poses(None, 0, None) == -1


class _FakeLib:
    """records every call: the manager's own checks must fire before any"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            return 0
        return f


def _manager_without_device():
    from sgtd_amd.manager import STDescManager
    m = STDescManager.__new__(STDescManager)
    m._L, m._h = _FakeLib(), ctypes.c_void_p(1)
    m.config_setting_ = {"candidate_num": 50}
    return m


@pytest.mark.parametrize("ids, poses", [
    (np.arange(3), np.zeros((3, 11))),              # 11 floats a row
    (np.arange(3), np.zeros((2, 12))),              # fewer poses than ids
    (np.arange(3), np.zeros((3, 3, 4))),            # 3x4, not 4x4
    (np.arange(6).reshape(2, 3), np.zeros((6, 12))),
    (np.array([-1, 0, 1]), np.zeros((3, 12))),
    (np.array([0.5, 1.0]), np.zeros((2, 12))),
    (None, np.zeros((3, 12))),                      # poses without ids
])
def test_manager_rejects_bad_poses(ids, poses):
    m = _manager_without_device()
    with pytest.raises(ValueError):
        m.set_frame_poses(ids, poses)
    assert m._L.calls == []


@pytest.mark.parametrize("center, radius", [
    (np.zeros(4), 1.0),                             # dims 4
    (np.zeros(1), 1.0),                             # dims 1
    (np.zeros((2, 2, 2)), 1.0),
    (np.zeros((0, 2)), 1.0),
    (np.array([np.nan, 0.0]), 1.0),
    (np.array([np.inf, 0.0]), 1.0),
    (np.zeros((3, 2)), np.ones(2)),                 # two radii for three rows
    (np.zeros(2), -1.0),
    (np.zeros(2), np.nan),
    (np.zeros(2), None),
])
def test_manager_rejects_bad_priors(center, radius):
    m = _manager_without_device()
    with pytest.raises(ValueError):
        m.set_position_prior(center, radius)
    assert m._L.calls == []


def test_manager_accepts_good_forms():
    m = _manager_without_device()
    m.set_frame_poses(np.arange(2), np.stack([np.eye(4)] * 2))
    m.set_frame_poses(np.arange(2), np.zeros((2, 12)))
    m.set_frame_poses(np.arange(2), None)
    m.set_frame_poses(None, None)
    m.set_position_prior(np.zeros(3), np.inf)
    m.set_position_prior(np.zeros((4, 2)), np.arange(4.0))
    m.set_position_prior(None)
    assert m._L.calls == ["sgtd_set_frame_poses"] * 4 + ["sgtd_set_position_prior"] * 3


def prior_rows(t, has, center, radius):
    """the rule of sgtd_set_position_prior, restated: t (F, 3) f32 translations, has (F,) bool, center (R, dims) f64,
    radius (R,) -> bool (R, F), in the stated operation order (each f64 operation rounds; numpy does not contract)"""
    t = np.asarray(t, np.float32).astype(np.float64)
    dims = center.shape[1]
    dx = t[None, :, 0] - center[:, 0:1]
    dy = t[None, :, 1] - center[:, 1:2]
    d2 = dx * dx + dy * dy
    fin = np.isfinite(t[:, 0]) & np.isfinite(t[:, 1])
    if dims == 3:
        dz = t[None, :, 2] - center[:, 2:3]
        d2 = d2 + dz * dz
        fin = fin & np.isfinite(t[:, 2])
    rr = np.asarray(radius, np.float64) * np.asarray(radius, np.float64)
    return has[None, :] & fin[None, :] & (d2 <= rr[:, None])


def test_rule_equals_frames_near_and_brute_force():
    from sgtd_amd import evaluate as ev, synth
    smap = synth.make_map(400, 20, stream=331)
    rows = np.stack([ev.pose_row(*p) for p in smap.pose])
    t = rows[:, [3, 7, 11]]
    rng = np.random.default_rng(5)
    t[:, 2] = rng.normal(0.0, 5.0, len(t)).astype(np.float32)
    has = np.ones(len(t), bool)
    centers = t[rng.integers(0, len(t), 64), :].astype(np.float64) + rng.normal(0.0, 10.0, (64, 3))
    for radius in (0.0, 12.5, 50.0, 1e3):
        got = prior_rows(t, has, centers[:, :2], np.full(64, radius))
        assert np.array_equal(got, ev.frames_near(t[:, :2], centers[:, :2], radius)), radius
        got3 = prior_rows(t, has, centers, np.full(64, radius))
        brute = np.zeros_like(got3)
        for r in range(64):
            for f in range(len(t)):
                d = [float(t[f, i]) - float(centers[r, i]) for i in range(3)]
                brute[r, f] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= radius * radius
        assert np.array_equal(got3, brute), radius
    assert 0 < prior_rows(t, has, centers[:, :2], np.full(64, 50.0)).sum() < 64 * len(t)
    # exactly at the radius (a 3-4-5 offset) is inside; without a pose, or with a non-finite translation, never
    t2 = np.array([[3.0, 4.0, 0.0], [3.0, 4.0, 12.0], [0.0, 0.0, 0.0], [np.nan, 0, 0], [np.inf, 0, 0], [0, 0, np.nan]], np.float32)
    has2 = np.array([True, True, False, True, True, True])
    assert prior_rows(t2, has2, np.zeros((1, 2)), np.array([5.0])).tolist() == [[True, True, False, False, False, True]]
    assert prior_rows(t2, has2, np.zeros((1, 3)), np.array([13.0])).tolist() == [[True, True, False, False, False, False]]
    assert prior_rows(t2, has2, np.zeros((1, 2)), np.array([np.inf])).tolist() == [[True, True, False, False, False, True]]
