"""sgtd_set_frame_keypoints / sgtd_overlap / sgtd_result_overlap / sgtd_search_loop_overlap at the ABI boundary and in the
Python layer, without a GPU: the header declares them, the library exports them, the ctypes binding passes the declared
types, the argument checks run before anything touches a device, the manager rejects bad arguments before calling the
library, and the numpy restatement of the rule (tests/_overlap_ref.py) gives the answers that are known in advance."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _overlap_ref as ov
from sgtd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_set_frame_keypoints": ["sgtd_handle h", "const uint32_t *frame_ids", "const int64_t *kp_off", "const float *xyz",
                                 "const uint32_t *label", "int64_t n"],
    "sgtd_overlap": ["sgtd_handle h", "double radius", "int flags", "const float *q_xyz", "const uint32_t *q_label",
                     "const int64_t *q_kp_off"],
    "sgtd_result_overlap": ["sgtd_handle h", "int q", "int32_t *n_query_kp", "int32_t *n_frame_kp", "int32_t *n_hit_query",
                            "int32_t *n_hit_frame", "double *overlap", "double *rms"],
    "sgtd_search_loop_overlap": ["sgtd_handle h", "double icp_threshold", "double min_overlap", "int32_t *best_cand",
                                 "int32_t *best_frame", "double *best_score", "double *best_overlap"],
}


def test_header_declares_the_calls_and_the_flag():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    for name, want in DECLS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name + " is not declared"
        text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        args = [" ".join(a.split()) for a in text.split(",")]
        assert args == want, name
        assert name in _lib.SYMBOLS
    assert re.search(r"^#define\s+SGTD_OVERLAP_REFINED\s+1\b", header, re.M)


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm is not installed")
def test_library_exports_the_calls():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in DECLS:
        assert re.search(r"\bT %s$" % name, out, re.M), name


def test_binding_types_and_argument_checks():
    L = _lib.lib()
    vp, dbl, i64 = ctypes.c_void_p, ctypes.c_double, ctypes.c_int64
    assert L.sgtd_set_frame_keypoints.argtypes == [vp, vp, vp, vp, vp, i64]
    assert L.sgtd_overlap.argtypes == [vp, dbl, ctypes.c_int, vp, vp, vp]
    assert L.sgtd_result_overlap.argtypes == [vp, ctypes.c_int, vp, vp, vp, vp, vp, vp]
    assert L.sgtd_search_loop_overlap.argtypes == [vp, dbl, dbl, vp, vp, vp, vp]
    for name in DECLS:
        assert getattr(L, name).restype is ctypes.c_int
    # every listed argument error on a NULL handle: SGTD_ERR_INVALID, without a device
    ids = np.arange(2, dtype=np.uint32)
    off = np.array([0, 1, 2], np.int64)
    xyz, lab = np.zeros((2, 3), np.float32), np.zeros(2, np.uint32)
    P = lambda a: a.ctypes.data
    assert L.sgtd_set_frame_keypoints(None, P(ids), P(off), P(xyz), P(lab), 2) == -1
    assert L.sgtd_set_frame_keypoints(None, P(ids), P(off), P(xyz), P(lab), -1) == -1
    assert L.sgtd_set_frame_keypoints(None, None, P(off), P(xyz), P(lab), 2) == -1
    assert L.sgtd_set_frame_keypoints(None, P(ids), None, P(xyz), P(lab), 2) == -1
    assert L.sgtd_set_frame_keypoints(None, P(ids), P(off), P(xyz), None, 2) == -1
    assert L.sgtd_set_frame_keypoints(None, None, None, None, None, 0) == -1
    big = np.array([0, 65536, 65537], np.int64)
    assert L.sgtd_set_frame_keypoints(None, P(ids), P(big), P(xyz), P(lab), 2) == -1
    for radius in (1.0, 0.0, float("nan"), -1.0, float("inf")):
        for flags in (0, 1, 2, -1):
            assert L.sgtd_overlap(None, radius, flags, None, None, None) == -1
    assert L.sgtd_overlap(None, 1.0, 0, P(xyz), None, P(off)) == -1
    assert L.sgtd_overlap(None, 1.0, 0, P(xyz), P(lab), None) == -1
    assert L.sgtd_overlap(None, 1.0, 0, P(xyz), P(lab), P(big)) == -1
    n, x = np.zeros(50, np.int32), np.zeros(50)
    assert L.sgtd_result_overlap(None, 0, P(n), P(n), P(n), P(n), P(x), P(x)) == -1
    assert L.sgtd_result_overlap(None, 0, None, None, None, None, None, None) == -1
    assert L.sgtd_search_loop_overlap(None, 0.4, 0.4, P(n), P(n), P(x), P(x)) == -1
    assert L.sgtd_search_loop_overlap(None, 0.4, 0.0, None, None, None, None) == -1


class _FakeLib:
    """records every call: the manager's own checks must fire before any"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            return 0
        return f


def _manager_without_device(nq=3):
    from sgtd_amd.manager import STDescManager
    m = STDescManager.__new__(STDescManager)
    m._L, m._h = _FakeLib(), ctypes.c_void_p(1)
    m.config_setting_ = {"candidate_num": 50}
    m.icp_threshold_ = 0.4
    m._nq = nq
    return m


@pytest.mark.parametrize("radius, exc", [(-1.0, ValueError), (float("nan"), ValueError), (float("inf"), ValueError),
                                         ("1", TypeError), (None, TypeError), (True, TypeError)])
def test_manager_rejects_a_bad_radius(radius, exc):
    m = _manager_without_device()
    with pytest.raises(exc):
        m.overlap(radius)
    assert m._L.calls == []


def test_manager_rejects_bad_keypoints():
    m = _manager_without_device()
    xyz, lab = np.zeros((3, 5, 3), np.float32), np.zeros((3, 5), np.uint32)
    with pytest.raises(ValueError):
        m.overlap(1.0, xyz=xyz)                                   # no labels
    with pytest.raises(ValueError):
        m.overlap(1.0, label=lab)                                 # labels without xyz
    with pytest.raises(ValueError):
        m.overlap(1.0, xyz=xyz[:2], label=lab[:2])                # two rows for a batch of three
    with pytest.raises(ValueError):
        m.overlap(1.0, xyz=xyz.reshape(-1, 3), label=lab.reshape(-1), kp_off=[0, 5, 10])
    with pytest.raises(ValueError):
        m.overlap(1.0, xyz=np.zeros((70000, 3), np.float32), label=np.zeros(70000, np.uint32), kp_off=[0, 0, 0, 70000])
    with pytest.raises(ValueError):
        m.set_frame_keypoints(None, xyz, lab)
    with pytest.raises(ValueError):
        m.set_frame_keypoints([0, 1, -1], xyz, lab)
    with pytest.raises(ValueError):
        m.set_frame_keypoints([[0, 1, 2]], xyz, lab)
    with pytest.raises(ValueError):
        m.set_frame_keypoints([0.5, 1.0, 2.0], xyz, lab)
    with pytest.raises(ValueError):
        m.set_frame_keypoints([0, 1, 2], xyz)                     # no labels
    with pytest.raises(ValueError):
        m.set_frame_keypoints([0, 1], xyz, lab)                   # three rows for two ids
    with pytest.raises(ValueError):
        m.set_frame_keypoints([0, 1, 2], xyz.reshape(-1, 3), lab.reshape(-1), kp_off=[0, 5, 3, 15])
    for q, exc in ((-1, ValueError), (0.5, TypeError), (None, TypeError)):
        with pytest.raises(exc):
            m.result_overlap(q)
    for mo, exc in (("0.4", TypeError), (None, TypeError), (float("nan"), ValueError)):
        with pytest.raises(exc):
            m.search_loop_overlap(mo)
    assert m._L.calls == []


def test_manager_passes_good_arguments_on():
    m = _manager_without_device()
    xyz, lab = np.zeros((3, 5, 3), np.float32), np.zeros((3, 5), np.uint32)
    m.set_frame_keypoints([4, 5, 6], xyz, lab)
    m.set_frame_keypoints(np.array([4, 5, 6]), xyz.reshape(-1, 3), lab.reshape(-1), kp_off=[0, 0, 15, 15])
    m.set_frame_keypoints([4], None)
    m.set_frame_keypoints(None, None)
    m.overlap(1.0)
    m.overlap(0, refined=True)
    m.overlap(np.float32(0.5), xyz=xyz, label=lab)
    m.overlap(0.5, xyz=xyz.reshape(-1, 3), label=lab.reshape(-1), kp_off=np.array([0, 15, 15, 15]))
    r = m.result_overlap(2)
    bc, bf, bs, bo = m.search_loop_overlap(0.4)
    assert m._L.calls == ["sgtd_set_frame_keypoints"] * 4 + ["sgtd_overlap"] * 4 + ["sgtd_result_overlap", "sgtd_search_loop_overlap"]
    for k in ("n_query_kp", "n_frame_kp", "n_hit_query", "n_hit_frame"):
        assert r[k].shape == (50,) and r[k].dtype == np.int32
    assert r["overlap"].shape == (50,) and r["rms"].dtype == np.float64
    assert bc.shape == bf.shape == bs.shape == bo.shape == (3,) and bc.dtype == np.int32 and bo.dtype == np.float64


# ---- known answers of the restatement

def _frame(rng, n, n_labels=6):
    return rng.uniform(-40.0, 40.0, (n, 3)).astype(np.float32), rng.integers(0, n_labels, n).astype(np.uint32)


I3, Z3 = np.eye(3), np.zeros(3)


@pytest.mark.parametrize("n", [1, 200, 257])
def test_identical_frame_under_identity(n):
    xyz, lab = _frame(np.random.default_rng(n), n)
    r = ov.overlap(I3, Z3, xyz, lab, xyz, lab, 1.0)
    assert (r["n_query_kp"], r["n_frame_kp"], r["n_hit_query"], r["n_hit_frame"]) == (n, n, n, n)
    assert r["overlap"] == 1.0 and r["rms"] == 0.0
    r = ov.overlap(I3, Z3, xyz, lab, xyz, lab, 0.0)             # radius 0: m_i = 0 <= 0
    assert r["n_hit_query"] == n and r["rms"] == 0.0


def test_translation_switches_the_hits_off_exactly_past_the_radius():
    # keypoints 100 m apart: the only neighbour within reach is the keypoint's own copy, 0.75 m away (exact in f32 and f64)
    xyz = (np.arange(30, dtype=np.float32)[:, None] * np.array([100.0, 0.0, 0.0], np.float32))
    lab = np.zeros(30, np.uint32)
    t = np.array([0.0, 0.75, 0.0])
    for radius, hits in ((0.75, 30), (np.nextafter(0.75, 0.0), 0), (np.nextafter(0.75, 1.0), 30), (0.0, 0)):
        r = ov.overlap(I3, t, xyz, lab, xyz, lab, radius)
        assert r["n_hit_query"] == hits and r["n_hit_frame"] == hits, radius
        assert r["overlap"] == hits / 30.0
        assert (r["rms"] == 0.75) if hits else np.isnan(r["rms"])


def test_disjoint_labels_never_hit():
    xyz, lab = _frame(np.random.default_rng(3), 100)
    r = ov.overlap(I3, Z3, xyz, lab, xyz, lab + np.uint32(100), 1e6)
    assert r["n_hit_query"] == 0 and r["n_hit_frame"] == 0 and r["overlap"] == 0.0 and np.isnan(r["rms"])
    assert np.isinf(r["m"]).all()
    # labels are compared as u32: 2^32 - 1 is not -1 of another width, and is itself
    big = np.full(100, 0xFFFFFFFF, np.uint32)
    assert ov.overlap(I3, Z3, xyz, big, xyz, big, 0.0)["n_hit_query"] == 100


def test_many_to_one_counts_differ():
    # five query keypoints around ONE frame keypoint, and a second frame keypoint nobody reaches
    q = np.array([[0.1, 0, 0], [-0.1, 0, 0], [0, 0.1, 0], [0, -0.1, 0], [0, 0, 0.1]], np.float32)
    f = np.array([[0, 0, 0], [50, 0, 0]], np.float32)
    r = ov.overlap(I3, Z3, q, np.zeros(5, np.uint32), f, np.zeros(2, np.uint32), 0.5)
    assert r["n_hit_query"] == 5 and r["n_hit_frame"] == 1 and r["n_frame_kp"] == 2
    # and one query keypoint between two frame keypoints
    r = ov.overlap(I3, Z3, np.zeros((1, 3), np.float32), np.zeros(1, np.uint32), np.array([[0.2, 0, 0], [-0.3, 0, 0]], np.float32),
                   np.zeros(2, np.uint32), 0.5)
    assert r["n_hit_query"] == 1 and r["n_hit_frame"] == 2
    assert r["m"][0] == np.float64(np.float32(0.2)) ** 2


def test_nan_never_hits():
    xyz, lab = _frame(np.random.default_rng(5), 40, n_labels=1)
    bad = xyz.copy()
    bad[7, 1] = np.nan
    r = ov.overlap(I3, Z3, bad, lab, xyz, lab, 0.5)              # a NaN query coordinate
    assert r["n_hit_query"] == 39 and not r["hit_query"][7] and np.isinf(r["m"][7]) and r["n_hit_frame"] == 39
    r = ov.overlap(I3, Z3, xyz, lab, bad, lab, 0.5)              # a NaN frame coordinate
    assert r["n_hit_query"] == 39 and not r["hit_frame"][7] and r["n_hit_frame"] == 39
    assert r["rms"] == 0.0


def test_empty_sets_and_missing_frames():
    xyz, lab = _frame(np.random.default_rng(6), 10)
    e3, e1 = np.zeros((0, 3), np.float32), np.zeros(0, np.uint32)
    r = ov.overlap(I3, Z3, e3, e1, xyz, lab, 1.0)
    assert (r["n_query_kp"], r["n_frame_kp"], r["n_hit_query"], r["n_hit_frame"]) == (0, 10, 0, 0)
    assert np.isnan(r["overlap"]) and np.isnan(r["rms"])
    r = ov.overlap(I3, Z3, xyz, lab, e3, e1, 1.0)
    assert (r["n_query_kp"], r["n_frame_kp"], r["n_hit_query"], r["n_hit_frame"]) == (10, 0, 0, 0)
    assert r["overlap"] == 0.0 and np.isnan(r["rms"])
    r = ov.overlap(I3, Z3, xyz, lab, None, None, 1.0)
    assert (r["n_query_kp"], r["n_frame_kp"], r["n_hit_query"], r["n_hit_frame"]) == (10, -1, 0, 0)
    assert np.isnan(r["overlap"]) and np.isnan(r["rms"])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_summation_order_equals_the_plain_loop(n):
    rng = np.random.default_rng(100 + n)
    values = np.abs(rng.normal(size=n)) * 10.0 ** rng.integers(-8, 8, n)     # another order gives other bits
    take = rng.random(n) < 0.6
    take[0] = True
    a, b = ov.ordered_sum(values, take), ov.ordered_sum_loop(values, take)
    assert a.view(np.uint64) == b.view(np.uint64)
    assert abs(a - values[take].sum()) <= 1e-12 * values[take].sum()


def test_gated_choice_of_the_restatement():
    score = np.array([10.0, 30.0, 20.0, -1.0])
    o = np.array([0.5, 0.1, 0.45, np.nan])
    frames = np.array([7, 8, 9, 10])
    assert ov.search_loop_overlap(score, o, 4, frames, 0.4, 0.0) == (1, 8, 30.0, 0.1)
    assert ov.search_loop_overlap(score, o, 4, frames, 0.4, 0.4) == (2, 9, 20.0, 0.45)
    assert ov.search_loop_overlap(score, o, 4, frames, 0.4, 0.5) == (0, 7, 10.0, 0.5)
    bc, bf, bs, bo = ov.search_loop_overlap(score, o, 4, frames, 0.4, 0.6)
    assert (bc, bf, bs) == (-1, -1, 0.0) and np.isnan(bo)
    assert ov.search_loop_overlap(score, o, 1, frames, 25.0, 0.0)[:3] == (-1, -1, 0.0)
