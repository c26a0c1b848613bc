"""sgtd_local_map_keypoints without a device: the declarations, the default options, the argument checks, the properties
of the rule's numpy restatement (tests/_local_map_ref.py), and the ingest helpers."""
import ctypes
import os
import re

import numpy as np
import pytest

import _local_map_ref as ref
import _scan_ref as sref
from sgtd_amd import _lib, ingest, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_local_map_keypoints": ["sgtd_handle h", "const sgtd_scan_config *cfg", "const sgtd_local_map_options *opt", "const float *points",
                                 "int stride_floats", "const uint32_t *labels", "const int64_t *pt_off", "const float *pose12", "int n_scans",
                                 "const int32_t *anchors", "int n_anchors", "int device_ptrs"],
    "sgtd_result_local_map_keypoints": ["sgtd_handle h", "int64_t *kp_off", "float *xyz", "uint32_t *label", "int32_t *n_points",
                                        "int64_t capacity", "int64_t *n_keypoints"],
    "sgtd_result_local_map_members": ["sgtd_handle h", "int64_t *mem_off", "int32_t *member", "int64_t capacity", "int64_t *n_members",
                                      "int64_t *merged_points", "int32_t *n_passes"],
    "sgtd_local_map_device_view": ["sgtd_handle h", "const float **d_xyz", "const uint32_t **d_label"],
}


def test_header_declares_the_calls():
    h = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    for name, want in DECLS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, h)
        assert m, name + " is not declared"
        text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        assert [" ".join(a.split()) for a in text.split(",")] == want, name
    assert re.search(r"void\s+sgtd_default_local_map_options\s*\(\s*sgtd_local_map_options \*opt\s*\)\s*;", h)
    body = re.search(r"typedef struct sgtd_local_map_options \{(.*?)\} sgtd_local_map_options;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == ["double radius", "int32_t max_members", "int32_t reserved",
                                                                           "int64_t max_pass_points"]
    # the rule names its departures from the reference beside the scan rule
    for word in ("current_scan_path", "rigid inverse", "one cluster for the whole class", "densitys"):
        assert word in h, word


def test_binding_declares_the_calls():
    for name in list(DECLS) + ["sgtd_default_local_map_options"]:
        assert name in _lib.SYMBOLS, name
    L = _lib.lib()
    for name, want in DECLS.items():
        assert len(getattr(L, name).argtypes) == len(want), name
        assert getattr(L, name).restype is ctypes.c_int
    assert ctypes.sizeof(_lib.LocalMapOptions) == 24


def test_default_options():
    o = _lib.LocalMapOptions(radius=-1.0, max_members=7, reserved=3, max_pass_points=9)
    _lib.lib().sgtd_default_local_map_options(ctypes.byref(o))
    assert (o.radius, o.max_members, o.reserved, o.max_pass_points) == (15.0, 0, 0, 0)


def options(**kw):
    o = _lib.LocalMapOptions()
    _lib.lib().sgtd_default_local_map_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


BAD_OPTIONS = [dict(radius=float("nan")), dict(radius=-1.0), dict(radius=float("inf")), dict(max_members=-1), dict(max_pass_points=-1),
               dict(max_pass_points=(1 << 28) + 1), dict(reserved=1)]


@pytest.mark.parametrize("kw", BAD_OPTIONS, ids=lambda kw: "%s=%s" % next(iter(kw.items())))
def test_invalid_options_return_without_a_device(kw):
    L = _lib.lib()
    off = np.zeros(1, np.int64)
    o = options(**kw)
    assert L.sgtd_local_map_keypoints(None, None, ctypes.byref(o), None, 3, None, off.ctypes.data_as(ctypes.c_void_p), None, 0, None, 0, 0) == -1


def test_null_handle_and_bad_arguments_are_invalid():
    L = _lib.lib()
    pv = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    off, bad_off = np.array([0, 4, 6], np.int64), np.array([0, 4, 2], np.int64)
    pts, lab, pose = np.zeros((6, 3), np.float32), np.zeros(6, np.uint32), np.zeros((2, 12), np.float32)
    anch = np.array([0, 2], np.int32)
    n = ctypes.c_int64(0)
    call = lambda *a: L.sgtd_local_map_keypoints(None, None, None, *a)
    assert call(pv(pts), 3, pv(lab), pv(off), pv(pose), 2, None, 0, 0) == -1              # no handle
    assert call(pv(pts), 3, pv(lab), pv(off), None, 2, None, 0, 0) == -1                  # no poses
    assert call(pv(pts), 3, pv(lab), pv(off), pv(pose), 2, pv(anch), -1, 0) == -1         # a negative count
    assert call(pv(pts), 3, pv(lab), pv(off), pv(pose), 2, pv(anch), 2, 0) == -1          # an anchor outside the scans
    assert call(pv(pts), 3, pv(lab), pv(off), pv(pose), -1, None, 0, 0) == -1
    assert call(pv(pts), 5, pv(lab), pv(off), pv(pose), 2, None, 0, 0) == -1
    assert call(pv(pts), 3, pv(lab), None, pv(pose), 2, None, 0, 0) == -1
    assert call(pv(pts), 3, pv(lab), pv(bad_off), pv(pose), 2, None, 0, 0) == -1
    assert call(None, 3, pv(lab), pv(off), pv(pose), 2, None, 0, 0) == -1
    c = _lib.ScanConfig()
    L.sgtd_default_scan_config(ctypes.byref(c))
    c.min_range = 200.0
    assert L.sgtd_local_map_keypoints(None, ctypes.byref(c), None, pv(pts), 3, pv(lab), pv(off), pv(pose), 2, None, 0, 0) == -1
    assert L.sgtd_result_local_map_keypoints(None, None, None, None, None, 0, ctypes.byref(n)) == -1
    assert L.sgtd_result_local_map_members(None, None, None, 0, ctypes.byref(n), None, None) == -1
    assert L.sgtd_local_map_device_view(None, None, None) == -1


# ---- the restatement ----
def case(counts, stream):
    p, l, off = synth.make_scans(len(counts), counts, stream=stream, n_blobs=12)
    return p, l, off, ref.path_poses(len(counts))


def test_one_scan_is_the_scan_rule():
    p, l, off, poses = case([600], 3)
    cfg = ref.small_cfg()
    got = ref.local_map_rule(p, l, off, poses, cfg=cfg)
    want = sref.scan_rule(p, l, cfg)
    assert got["member"].tolist() == [0] and got["merged_points"].tolist() == [600]
    assert np.array_equal(got["xyz"].view(np.uint32), want["xyz"].view(np.uint32)) and np.array_equal(got["n_points"], want["n_points"])
    assert len(want["label"]) > 0


def test_identical_poses_give_the_concatenation():
    p, l, off, poses = case([300, 200, 100], 4)
    poses[:] = poses[2]
    got = ref.local_map_rule(p, l, off, poses, anchors=[1], cfg=ref.small_cfg())
    assert got["member"].tolist() == [1, 0, 2]
    xyz, lab = got["clouds"][0]
    order = np.r_[300:500, 0:300, 500:600]
    # inv(T) T is the identity to rounding: the points come back within an ulp or two of a 50 m coordinate
    assert np.array_equal(xyz[:200], p[300:500, :3]) and np.allclose(xyz, p[order, :3], rtol=0, atol=2e-5)
    assert np.array_equal(lab, l[order])
    eye = np.zeros((3, 12), np.float32)
    eye[:, [0, 5, 10]] = 1.0
    xyz, _ = ref.local_map_rule(p, l, off, eye, anchors=[1], cfg=ref.small_cfg())["clouds"][0]
    assert np.array_equal(xyz, p[order, :3])


def test_member_rule_at_the_radius():
    poses = np.zeros((2, 12), np.float32)
    poses[:, [0, 5, 10]] = 1.0
    poses[1, [3, 7, 11]] = (3.0, 4.0, 0.0)
    assert ref.members(poses, 0, radius=5.0) == [0, 1]
    poses[1, 3] = np.nextafter(np.float32(3.0), np.float32(4.0))
    assert ref.members(poses, 0, radius=5.0) == [0]
    assert ref.members(poses, 0, radius=5.000001) == [0, 1]
    poses[1, 3] = np.nan
    assert ref.members(poses, 0, radius=5.0) == [0] and ref.members(poses, 1, radius=5.0) == [1]
    poses[1, 3] = np.inf
    assert ref.members(poses, 0, radius=5.0) == [0] and ref.members(poses, 1, radius=5.0) == [1]


def test_max_members_tie_goes_to_the_smaller_index():
    poses = np.zeros((5, 12), np.float32)
    poses[:, [0, 5, 10]] = 1.0
    poses[:, 3] = (2.0, 1.0, 0.0, -1.0, -3.0)      # scans 1 and 3 are equally far from the anchor 2
    assert ref.members(poses, 2, radius=5.0) == [2, 0, 1, 3, 4]
    assert ref.members(poses, 2, radius=5.0, max_members=1) == [2]
    assert ref.members(poses, 2, radius=5.0, max_members=2) == [2, 1]
    assert ref.members(poses, 2, radius=5.0, max_members=3) == [2, 1, 3]
    assert ref.members(poses, 2, radius=5.0, max_members=4) == [2, 0, 1, 3]
    assert ref.members(poses, 2, radius=5.0, max_members=9) == [2, 0, 1, 3, 4]


def test_plan_passes():
    assert ref.plan_passes([], 0) == 0 and ref.plan_passes([5, 5, 5], 0) == 1
    assert ref.plan_passes([5, 5, 5], 10) == 2 and ref.plan_passes([5, 5, 5], 5) == 3 and ref.plan_passes([0, 5, 0, 5, 0], 5) == 2


def test_sensor_poses_against_a_longhand_product():
    rng = np.random.default_rng(5)
    poses, ext = rng.normal(0.0, 1.0, (4, 12)), rng.normal(0.0, 1.0, 12)
    got = ingest.sensor_poses(poses, ext)
    assert got.shape == (4, 12) and got.dtype == np.float32
    x4 = np.vstack([ext.reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])
    for k in range(4):
        p4 = np.vstack([poses[k].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])
        want = np.zeros((3, 4))
        for r in range(3):
            for c in range(4):
                want[r, c] = sum(p4[r, m] * x4[m, c] for m in range(4))
        assert np.allclose(got[k].reshape(3, 4), want, rtol=0, atol=1e-6)
    p44 = np.tile(np.eye(4), (4, 1, 1))
    p44[:, :3, :] = poses.reshape(4, 3, 4)
    assert np.array_equal(ingest.sensor_poses(p44, x4), got)


def test_read_pose_rows_round_trip(tmp_path):
    rows = np.random.default_rng(6).normal(0.0, 10.0, (5, 12))
    with open(tmp_path / "poses.txt", "w") as f:
        for r in rows:
            f.write(" ".join(repr(float(v)) for v in r) + "\n")
        f.write("\n")
    assert np.array_equal(ingest.read_pose_rows(str(tmp_path / "poses.txt")), rows)
    with open(tmp_path / "bad.txt", "w") as f:
        f.write("1 2 3\n")
    with pytest.raises(ValueError):
        ingest.read_pose_rows(str(tmp_path / "bad.txt"))


def test_make_posed_scans_is_one_world():
    p, l, off, poses = synth.make_posed_scans(4, 500, stream=2, spacing=1.0, n_blobs=20)
    assert p.shape == (2000, 4) and off.tolist() == [0, 500, 1000, 1500, 2000] and poses.shape == (4, 12)
    # every point, moved into the world, lies near a blob that other scans see too: the scans' world clouds overlap
    world = []
    for s in range(4):
        r, t = ref.rt(poses[s])
        world.append(p[off[s]:off[s + 1], :3].astype(np.float64) @ r.T + t)
    lo, hi = world[0].min(axis=0), world[0].max(axis=0)
    assert all(np.mean(np.all((w >= lo - 1.0) & (w <= hi + 1.0), axis=1)) > 0.9 for w in world[1:])
