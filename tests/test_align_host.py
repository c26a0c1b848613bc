"""sgtd_align_keypoints / sgtd_result_aligned* / sgtd_search_loop_aligned at the ABI boundary and in the Python layer,
without a GPU: the header declares them, the library exports them, the ctypes binding passes the declared types, the
argument checks run before anything touches a device, the manager rejects bad arguments before calling the library, and
the numpy restatement of the rule (tests/_align_ref.py) gives the answers that are known in advance."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _align_ref as al
import _overlap_ref as ov
from sgtd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_align_keypoints": ["sgtd_handle h", "double radius", "int iterations", "int flags", "const float *q_xyz",
                             "const uint32_t *q_label", "const int64_t *q_kp_off"],
    "sgtd_result_aligned": ["sgtd_handle h", "int q", "double *pose", "int32_t *n_fits", "int32_t *n_corr", "int32_t *stop",
                            "int32_t *counts_before", "int32_t *counts_after", "double *overlap_before", "double *rms_before",
                            "double *overlap_after", "double *rms_after", "double *moments"],
    "sgtd_result_aligned_pairs": ["sgtd_handle h", "int q", "int cand", "int32_t *frame_kp", "int64_t capacity", "int64_t *n"],
    "sgtd_result_aligned_world_poses": ["sgtd_handle h", "int q", "float *world"],
    "sgtd_search_loop_aligned": ["sgtd_handle h", "double min_overlap", "double max_rms", "int32_t *best_cand", "int32_t *best_frame",
                                 "double *best_rms", "double *best_overlap"],
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
    assert re.search(r"^#define\s+SGTD_ALIGN_REFINED\s+1\b", header, re.M)


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm is not installed")
def test_library_exports_the_calls():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in DECLS:
        assert re.search(r"\bT %s$" % name, out, re.M), name


def test_binding_types_and_argument_checks():
    L = _lib.lib()
    vp, dbl, i64, ci = ctypes.c_void_p, ctypes.c_double, ctypes.c_int64, ctypes.c_int
    assert L.sgtd_align_keypoints.argtypes == [vp, dbl, ci, ci, vp, vp, vp]
    assert L.sgtd_result_aligned.argtypes == [vp, ci] + [vp] * 11
    assert L.sgtd_result_aligned_pairs.argtypes == [vp, ci, ci, vp, i64, vp]
    assert L.sgtd_result_aligned_world_poses.argtypes == [vp, ci, vp]
    assert L.sgtd_search_loop_aligned.argtypes == [vp, dbl, dbl, vp, vp, vp, vp]
    for name in DECLS:
        assert getattr(L, name).restype is ctypes.c_int
    # every listed argument error on a NULL handle: SGTD_ERR_INVALID, without a device
    off = np.array([0, 1, 2], np.int64)
    xyz, lab = np.zeros((2, 3), np.float32), np.zeros(2, np.uint32)
    P = lambda a: a.ctypes.data
    for radius in (1.0, 0.0, float("nan"), -1.0, float("inf")):
        for iterations in (1, 10, 0, -1):
            for flags in (0, 1, 2, -1):
                assert L.sgtd_align_keypoints(None, radius, iterations, flags, None, None, None) == -1
    assert L.sgtd_align_keypoints(None, 1.0, 1, 0, P(xyz), None, P(off)) == -1
    assert L.sgtd_align_keypoints(None, 1.0, 1, 0, P(xyz), P(lab), None) == -1
    big = np.array([0, 65536, 65537], np.int64)
    assert L.sgtd_align_keypoints(None, 1.0, 1, 0, P(xyz), P(lab), P(big)) == -1
    n, n4, x, x12, x15 = np.zeros(50, np.int32), np.zeros(200, np.int32), np.zeros(50), np.zeros(600), np.zeros(750)
    assert L.sgtd_result_aligned(None, 0, P(x12), P(n), P(n), P(n), P(n4), P(n4), P(x), P(x), P(x), P(x), P(x15)) == -1
    assert L.sgtd_result_aligned(None, 0, *([None] * 11)) == -1
    cnt = ctypes.c_int64(0)
    assert L.sgtd_result_aligned_pairs(None, 0, 0, P(n), 50, ctypes.byref(cnt)) == -1
    assert L.sgtd_result_aligned_pairs(None, 0, 0, None, 0, None) == -1
    assert L.sgtd_result_aligned_world_poses(None, 0, P(np.zeros(600, np.float32))) == -1
    assert L.sgtd_result_aligned_world_poses(None, 0, None) == -1
    assert L.sgtd_search_loop_aligned(None, 0.4, 0.0, P(n), P(n), P(x), P(x)) == -1
    assert L.sgtd_search_loop_aligned(None, 0.0, 0.0, None, None, None, None) == -1


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
        m.align_keypoints(radius)
    assert m._L.calls == []


def test_manager_rejects_bad_arguments():
    m = _manager_without_device()
    xyz, lab = np.zeros((3, 5, 3), np.float32), np.zeros((3, 5), np.uint32)
    for it, exc in ((0, ValueError), (-3, ValueError), (1.5, TypeError), ("2", TypeError), (True, TypeError), (None, TypeError)):
        with pytest.raises(exc):
            m.align_keypoints(1.0, iterations=it)
    with pytest.raises(ValueError):
        m.align_keypoints(1.0, xyz=xyz)                           # no labels
    with pytest.raises(ValueError):
        m.align_keypoints(1.0, label=lab)                         # labels without xyz
    with pytest.raises(ValueError):
        m.align_keypoints(1.0, xyz=xyz[:2], label=lab[:2])        # two rows for a batch of three
    with pytest.raises(ValueError):
        m.align_keypoints(1.0, xyz=xyz.reshape(-1, 3), label=lab.reshape(-1), kp_off=[0, 5, 10])
    with pytest.raises(ValueError):
        m.align_keypoints(1.0, xyz=np.zeros((70000, 3), np.float32), label=np.zeros(70000, np.uint32), kp_off=[0, 0, 0, 70000])
    for q, exc in ((-1, ValueError), (0.5, TypeError), (None, TypeError)):
        with pytest.raises(exc):
            m.result_aligned(q)
        with pytest.raises(exc):
            m.result_aligned_world_poses(q)
        with pytest.raises(exc):
            m.result_aligned_pairs(q, 0)
        with pytest.raises(exc):
            m.result_aligned_pairs(0, q)
    for v, exc in (("0.4", TypeError), (None, TypeError), (float("nan"), ValueError), (True, TypeError)):
        with pytest.raises(exc):
            m.search_loop_aligned(v)
        with pytest.raises(exc):
            m.search_loop_aligned(0.4, v)
    assert m._L.calls == []


def test_manager_passes_good_arguments_on():
    m = _manager_without_device()
    xyz, lab = np.zeros((3, 5, 3), np.float32), np.zeros((3, 5), np.uint32)
    m.align_keypoints(1.0)
    m.align_keypoints(0, iterations=np.int64(3), refined=True)
    m.align_keypoints(np.float32(0.5), xyz=xyz, label=lab)
    m.align_keypoints(0.5, 2, xyz=xyz.reshape(-1, 3), label=lab.reshape(-1), kp_off=np.array([0, 15, 15, 15]))
    r = m.result_aligned(2)
    a = m.result_aligned_pairs(1, 4)
    w = m.result_aligned_world_poses(0)
    bc, bf, br, bo = m.search_loop_aligned(0.4, 0.5)
    m.search_loop_aligned()
    assert m._L.calls == ["sgtd_align_keypoints"] * 4 + ["sgtd_result_aligned"] + ["sgtd_result_aligned_pairs"] * 2 + \
        ["sgtd_result_aligned_world_poses"] + ["sgtd_search_loop_aligned"] * 2
    for k in ("n_fits", "n_corr", "stop"):
        assert r[k].shape == (50,) and r[k].dtype == np.int32
    for k in ("counts_before", "counts_after"):
        assert r[k].shape == (50, 4) and r[k].dtype == np.int32
    for k in ("overlap_before", "rms_before", "overlap_after", "rms_after"):
        assert r[k].shape == (50,) and r[k].dtype == np.float64
    assert r["rot"].shape == (50, 3, 3) and r["t"].shape == (50, 3) and r["moments"].shape == (50, 15)
    assert a.dtype == np.int32 and a.shape == (0,) and w.shape == (50, 12) and w.dtype == np.float32
    assert bc.shape == bf.shape == br.shape == bo.shape == (3,) and bc.dtype == np.int32 and br.dtype == np.float64


# ---- known answers of the restatement

I3, Z3 = np.eye(3), np.zeros(3)


def _grid(n):
    """n keypoints 100 m apart on a plane (no three on a line beyond the first row), one label"""
    i = np.arange(n)
    return np.stack([(i % 6) * 100.0, (i // 6) * 100.0, (i % 5) * 10.0], axis=1).astype(np.float32), np.zeros(n, np.uint32)


def test_a_pure_translation_is_recovered_in_one_fit():
    # the frame is the query moved by (0.25, -0.5, 0.125): exact in f32 and f64, every nearest neighbour is the own copy
    q, lab = _grid(30)
    d = np.array([0.25, -0.5, 0.125])
    f = (q.astype(np.float64) + d).astype(np.float32)
    r = al.align(I3, Z3, q, lab, f, lab, 1.0, 10)
    assert (r["n_fits"], r["n_corr"], r["stop"]) == (1, 30, 2)             # converged on the second iteration
    assert np.array_equal(r["assign"], np.arange(30))
    assert np.allclose(r["rot"], I3, atol=1e-12) and np.allclose(r["t"], d, atol=1e-9)
    assert r["before"]["n_hit_query"] == 30 and r["before"]["rms"] == np.sqrt(0.25 ** 2 + 0.5 ** 2 + 0.125 ** 2)
    assert r["after"]["n_hit_query"] == 30 and r["after"]["rms"] < 1e-9
    assert np.array_equal(r["moments"][:3] + d, r["moments"][3:6])       # cw = cp + d, exactly (sums of exact values)
    one = al.align(I3, Z3, q, lab, f, lab, 1.0, 1)                        # one iteration: out of iterations
    assert (one["n_fits"], one["stop"]) == (1, 0) and np.array_equal(one["moments"].view(np.uint64), r["moments"].view(np.uint64))


def test_fewer_than_three_assignable_keypoints():
    q, lab = _grid(30)
    f = q.copy()
    f[2:] += np.float32(50.0)                                              # only two keypoints keep a neighbour in reach
    R0 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    for R, t in ((I3, Z3), (R0, np.array([1e4, 0.0, 0.0]))):              # two assigned; a start pose far off: none
        r = al.align(R, t, q, lab, f, lab, 1.0, 10)
        assert (r["n_fits"], r["n_corr"], r["stop"]) == (0, 0, 1)
        assert np.array_equal(r["rot"], R) and np.array_equal(r["t"], t)  # the start pose stands
        assert np.isnan(r["moments"]).all()
        for k in ov.KEYS:
            assert ov.same_value(r["before"][k], r["after"][k])
    assert np.count_nonzero(al.align(I3, Z3, q, lab, f, lab, 1.0, 10)["assign"] >= 0) == 2
    # no stored keypoints, and an empty query
    r = al.align(I3, Z3, q, lab, None, None, 1.0, 10)
    assert (r["n_fits"], r["stop"], r["before"]["n_frame_kp"], r["after"]["n_hit_query"]) == (0, 1, -1, 0) and (r["assign"] == -1).all()
    r = al.align(I3, Z3, np.zeros((0, 3), np.float32), np.zeros(0, np.uint32), f, lab, 1.0, 10)
    assert (r["n_fits"], r["stop"], r["assign"].size) == (0, 1, 0) and np.isnan(r["after"]["overlap"])


def test_duplicate_frame_keypoints_give_the_lowest_index():
    q, lab = _grid(12)
    f = np.concatenate([q[:5], q, q])                                      # keypoint i of the query: copies at i (i < 5), 5 + i, 17 + i
    fl = np.zeros(len(f), np.uint32)
    a, m, fragile = al.assignment(I3, Z3, q, lab, f, fl, 0.0)
    assert np.array_equal(a, np.concatenate([np.arange(5), 5 + np.arange(5, 12)])) and (m == 0).all() and fragile
    # labels gate: with the first copies under another label the next ones are taken
    fl[:5] = 7
    a, _, _ = al.assignment(I3, Z3, q, lab, f, fl, 0.0)
    assert np.array_equal(a, 5 + np.arange(12))
    # a label present on one side only is never assigned
    a, m, _ = al.assignment(I3, Z3, q, lab + np.uint32(3), f, fl, 1e6)
    assert (a == -1).all() and np.isinf(m).all()


def test_nan_keypoints_are_never_assigned():
    q, lab = _grid(20)
    bad = q.copy()
    bad[7, 1] = np.nan
    a, m, _ = al.assignment(I3, Z3, bad, lab, q, lab, 0.5)                 # a NaN query coordinate
    assert a[7] == -1 and np.isinf(m[7]) and np.array_equal(np.delete(a, 7), np.delete(np.arange(20), 7))
    a, m, _ = al.assignment(I3, Z3, q, lab, bad, lab, 0.5)                 # a NaN frame coordinate: never the minimum
    assert a[7] == -1 and m[7] > 0.25 and np.array_equal(np.delete(a, 7), np.delete(np.arange(20), 7))
    r = al.align(I3, np.array([0.25, 0.0, 0.0]), bad, lab, q, lab, 0.5, 10)
    assert r["n_corr"] == 19 and r["assign"][7] == -1 and r["stop"] == 2 and np.isfinite(r["moments"]).all()
    inf = q.copy()
    inf[3, 0] = np.inf
    a, _, _ = al.assignment(I3, Z3, inf, lab, q, lab, 1e3)                 # an infinite coordinate: r2 = +inf, not <= rr
    assert a[3] == -1


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_summation_order_equals_the_plain_loop(n):
    rng = np.random.default_rng(200 + n)
    values = rng.normal(size=n) * 10.0 ** rng.integers(-8, 8, n)          # another order gives other bits
    take = rng.random(n) < 0.6
    take[0] = True
    a, b = ov.ordered_sum(values, take), ov.ordered_sum_loop(values, take)
    assert a.view(np.uint64) == b.view(np.uint64)
    # and the fit's sums are that sum, component by component
    q = rng.uniform(-40, 40, (n, 3)).astype(np.float32)
    f = rng.uniform(-40, 40, (n + 3, 3)).astype(np.float32)
    asg = np.where(take, rng.integers(0, n + 3, n), -1).astype(np.int32)
    cp, cw, H = al.fit(q, f, asg)
    c = np.float64(np.count_nonzero(take))
    p, w = q.astype(np.float64), f.astype(np.float64)[np.where(take, asg, 0)]
    assert (ov.ordered_sum_loop(p[:, 1], take) / c).view(np.uint64) == cp[1].view(np.uint64)
    assert (ov.ordered_sum_loop(w[:, 2], take) / c).view(np.uint64) == cw[2].view(np.uint64)
    assert ov.ordered_sum_loop((p[:, 0] - cp[0]) * (w[:, 2] - cw[2]), take).view(np.uint64) == H[0, 2].view(np.uint64)


def test_the_choice_of_the_restatement():
    nan = np.nan
    score = np.array([10.0, 30.0, 20.0, 5.0, 40.0, -1.0])
    rms = np.array([0.30, 0.10, 0.10, 0.05, nan, nan])
    o = np.array([0.50, 0.45, 0.45, 0.10, 0.90, nan])
    stop = np.array([2, 2, 0, 1, 1, -1])
    fr = np.array([7, 8, 9, 10, 11, 12])
    f = lambda n, mo, mr: al.search_loop_aligned(score, o, rms, stop, n, fr, mo, mr)
    assert f(6, 0.0, 0.0) == (3, 10, 0.05, 0.10)                          # no bounds: the smallest rms
    assert f(6, 0.4, 0.0) == (1, 8, 0.10, 0.45)                           # equal rms: the larger verify_score
    assert f(6, 0.4, np.inf) == (1, 8, 0.10, 0.45) and f(6, -1.0, -1.0) == (3, 10, 0.05, 0.10)
    assert f(6, 0.5, 0.0) == (0, 7, 0.30, 0.50)
    assert f(6, 0.0, 0.07) == (3, 10, 0.05, 0.10) and f(6, 0.4, 0.07)[:2] == (-1, -1)
    bc, bf, br, bo = f(6, 0.6, 0.0)                                       # the NaN rms is left out whatever its overlap
    assert (bc, bf) == (-1, -1) and np.isnan(br) and np.isnan(bo)
    assert f(1, 0.0, 0.0) == (0, 7, 0.30, 0.50)
    same = al.search_loop_aligned(np.array([5.0, 5.0]), np.array([0.5, 0.5]), np.array([0.2, 0.2]), np.array([2, 2]), 2, fr, 0.0, 0.0)
    assert same[0] == 0                                                   # a full tie: the lower candidate index
