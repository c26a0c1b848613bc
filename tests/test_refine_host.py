"""sgtd_refine_poses / sgtd_result_refined / sgtd_result_refined_world_poses at the ABI boundary and in the Python layer,
without a GPU: the header declares them, the library exports them, the ctypes binding passes the declared types, the
argument checks run before anything touches a device, the manager rejects bad arguments before calling the library, and
the numpy restatement of the rule (tests/_refine_ref.py) recovers a known rigid motion and sums in the header's order."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _refine_ref as rr
from sgtd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_refine_poses": ["sgtd_handle h", "int iterations"],
    "sgtd_result_refined": ["sgtd_handle h", "int q", "double *pose", "double *rmse", "double *rmse_verify", "int32_t *n_pairs",
                            "double *moments"],
    "sgtd_result_refined_world_poses": ["sgtd_handle h", "int q", "float *world"],
}


def test_header_declares_the_calls():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    for name, want in DECLS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name + " is not declared"
        text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        args = [" ".join(a.split()) for a in text.split(",")]
        assert args == want, name
        assert name in _lib.SYMBOLS


@pytest.mark.skipif(shutil.which("nm") is None, reason="binutils nm is not installed")
def test_library_exports_the_calls():
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in DECLS:
        assert re.search(r"\bT %s$" % name, out, re.M), name


def test_binding_types_and_argument_checks():
    L = _lib.lib()
    vp = ctypes.c_void_p
    assert L.sgtd_refine_poses.argtypes == [vp, ctypes.c_int]
    assert L.sgtd_result_refined.argtypes == [vp, ctypes.c_int, vp, vp, vp, vp, vp]
    assert L.sgtd_result_refined_world_poses.argtypes == [vp, ctypes.c_int, vp]
    for name in DECLS:
        assert getattr(L, name).restype is ctypes.c_int
    # a NULL handle and iterations < 1: SGTD_ERR_INVALID, without a device
    for it in (1, 3, 0, -1):
        assert L.sgtd_refine_poses(None, it) == -1
    pose, x, n, mom = np.zeros((50, 12)), np.zeros(50), np.zeros(50, np.int32), np.zeros((50, 15))
    assert L.sgtd_result_refined(None, 0, pose.ctypes.data, x.ctypes.data, x.ctypes.data, n.ctypes.data, mom.ctypes.data) == -1
    assert L.sgtd_result_refined(None, 0, None, None, None, None, None) == -1
    w = np.zeros((50, 12), np.float32)
    assert L.sgtd_result_refined_world_poses(None, 0, w.ctypes.data) == -1
    assert L.sgtd_result_refined_world_poses(None, 0, None) == -1


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


@pytest.mark.parametrize("iterations, exc", [(0, ValueError), (-2, ValueError), (1.5, TypeError), ("2", TypeError),
                                             (None, TypeError), (True, TypeError)])
def test_manager_rejects_bad_iterations(iterations, exc):
    m = _manager_without_device()
    with pytest.raises(exc):
        m.refine_poses(iterations)
    assert m._L.calls == []


@pytest.mark.parametrize("q, exc", [(-1, ValueError), (0.5, TypeError), (None, TypeError), ("0", TypeError)])
def test_manager_rejects_bad_query_index(q, exc):
    m = _manager_without_device()
    for call in (m.result_refined, m.result_refined_world_poses):
        with pytest.raises(exc):
            call(q)
    assert m._L.calls == []


def test_manager_passes_good_arguments_on():
    m = _manager_without_device()
    m.refine_poses()
    m.refine_poses(np.int64(3))
    r = m.result_refined(2)
    assert m._L.calls == ["sgtd_refine_poses", "sgtd_refine_poses", "sgtd_result_refined"]
    assert r["rot"].shape == (50, 3, 3) and r["t"].shape == (50, 3) and r["moments"].shape == (50, 15)
    assert r["n_pairs"].dtype == np.int32 and r["rmse"].shape == (50,) and r["rmse_verify"].shape == (50,)
    assert m.result_refined_world_poses(0).shape == (50, 12)


def _motion(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q, rng.uniform(-50.0, 50.0, 3)


@pytest.mark.parametrize("n_list", [4, 255, 256, 257, 1000])
def test_restatement_recovers_a_rigid_motion(n_list):
    rng = np.random.default_rng(n_list)
    R, t = _motion(rng)
    p = rng.uniform(-60.0, 60.0, (n_list, 3, 3))
    w = p @ R.T + t
    in_set = rng.random(n_list) < 0.7
    in_set[:4] = True
    got = rr.refine(p, w, in_set, 1, np.eye(3), np.zeros(3))
    assert np.abs(got["rot"] - R).max() <= 1e-12
    assert np.abs(got["t"] - t).max() <= 1e-12 * (1 + np.linalg.norm(got["cp"]) + np.linalg.norm(got["cw"]))
    assert got["n_pairs"] == np.count_nonzero(in_set) and got["rmse"] <= 1e-12 and got["rmse_verify"] > 1.0
    assert got["stop"] is None and got["fits"] == 1
    # noiseless data: the second iteration selects every pair of the list, the third finds that set unchanged
    got = rr.refine(p, w, in_set, 5, np.eye(3), np.zeros(3))
    assert got["n_pairs"] == n_list and got["set"].all()
    assert got["stop"] == "same" and got["fits"] == (1 if in_set.all() else 2)
    assert np.abs(got["rot"] - R).max() <= 1e-12


def test_restatement_stops_on_a_small_set():
    rng = np.random.default_rng(7)
    R, t = _motion(rng)
    p = rng.uniform(-60.0, 60.0, (40, 3, 3))
    w = p @ R.T + t
    w[3:] += rng.uniform(20.0, 30.0, (37, 3, 3))        # three pairs fit, the rest are far off under their motion
    set0 = np.zeros(40, bool)
    set0[:3] = True                                     # (a set sgtd_verify would not hand out: the rule itself)
    got = rr.refine(p, w, set0, 3, np.eye(3), np.zeros(3))
    assert got["stop"] == "few" and got["fits"] == 1 and got["n_pairs"] == 3 and np.array_equal(got["set"], set0)


@pytest.mark.parametrize("n_list", [1, 3, 256, 300, 777])
def test_summation_order_equals_the_plain_loop(n_list):
    rng = np.random.default_rng(100 + n_list)
    # values of very different magnitude: another order gives other bits
    terms = rng.normal(size=(n_list, 3, 3)) * 10.0 ** rng.integers(-8, 8, (n_list, 3, 3))
    in_set = rng.random(n_list) < 0.6
    a, b = rr.ordered_sum(terms, in_set), rr.ordered_sum_loop(terms, in_set)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    if n_list >= 300:
        naive = terms[in_set].sum(axis=(0, 1))
        assert not np.array_equal(a.view(np.uint64), naive.view(np.uint64))
    # matrices go component by component
    t4 = terms[:, :, :, None] * terms[:, :, None, :]
    a, b = rr.ordered_sum(t4, in_set), rr.ordered_sum_loop(t4, in_set)
    assert a.shape == (3, 3) and np.array_equal(a.view(np.uint64), b.view(np.uint64))
