"""sgtd_consistent_loops without a device: the numpy restatement of the rule (tests/_consistency_ref.py) on a planted world
and on hand-made graphs, the header's prototypes and the ctypes binding."""
import ctypes
import os
import re

import numpy as np

import _consistency_ref as cr
from sgtd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_consistent_loops": ["sgtd_handle h", "int64_t n", "const uint32_t *frame_a", "const uint32_t *frame_b", "const double *rel_pose",
                              "const float *pose_a", "double max_trans", "double max_rot", "int32_t *n_set"],
    "sgtd_result_consistent": ["sgtd_handle h", "int32_t *in_set", "int32_t *degree", "int32_t *pick", "double *thresholds"],
    "sgtd_result_consistency_rows": ["sgtd_handle h", "int64_t first", "int64_t n_rows", "uint64_t *rows"],
    "sgtd_result_loop_edges": ["sgtd_handle h", "double icp_threshold", "int flags", "int32_t *query", "uint32_t *frame_a",
                               "uint32_t *frame_b", "double *rel_pose", "double *score", "int64_t capacity", "int64_t *n_edges"],
}


def test_planted_world_keeps_exactly_the_true_loops():
    # 150 frames a quarter of a metre apart: the session spans some 30 m, so a pair of true loops (2 cm, 0.2 deg of
    # noise each) closes within sqrt(2) * (0.035 + 0.0035 * 30) = 0.2 m at one sigma of its farthest pairs; 1 m and 5 deg
    # are five of those, the aliases sit 29 m away
    w = cr.planted_world(60, 15, 5, seed=7)
    tt, min_trace = cr.thresholds(1.0, np.deg2rad(5.0))
    ref = cr.consistent(w["ids"], w["poses"], w["frame_a"], w["frame_b"], w["rel_pose"], tt, min_trace)
    assert ref["valid"].all()
    assert ref["n_set"] == 60
    assert np.array_equal(ref["in_set"].astype(bool), w["is_true"])
    # the five aliases agree with each other and with no true loop: no per-loop gate could tell them apart
    al = np.flatnonzero(w["is_alias"])
    assert ref["adj"][np.ix_(al, al)].sum() == 5 * 4
    assert not ref["adj"][np.ix_(al, np.flatnonzero(w["is_true"]))].any()
    # C is a clique, the picks are a permutation of 0 .. |C| - 1
    c = np.flatnonzero(ref["in_set"])
    assert ref["adj"][np.ix_(c, c)].sum() == c.size * (c.size - 1)
    assert sorted(ref["pick"][c]) == list(range(c.size)) and (ref["pick"][ref["in_set"] == 0] == -1).all()
    assert cr.clear_of_thresholds(ref, tt, min_trace)
    # the shortcut is the rule
    short = cr.consistent(w["ids"], w["poses"], w["frame_a"], w["frame_b"], w["rel_pose"], tt, min_trace, shortcut=True)
    for k in ("in_set", "degree", "pick", "n_set"):
        assert np.array_equal(ref[k], short[k]), k


def _graph(n, cliques=(), extra=()):
    adj = np.zeros((n, n), bool)
    for c in cliques:
        for a in c:
            for b in c:
                if a != b:
                    adj[a, b] = True
    for a, b in extra:
        adj[a, b] = adj[b, a] = True
    return adj


def _both(adj, valid=None):
    valid = np.ones(adj.shape[0], bool) if valid is None else valid
    plain = cr.greedy(adj, valid)
    short = cr.greedy(adj, valid, shortcut=True)
    for a, b in zip(plain, short):
        assert np.array_equal(a, b)
    return plain


def test_tie_rule_and_shortcut_on_hand_made_graphs():
    # two disjoint cliques of equal size: the one holding the lowest index wins, in ascending order
    in_set, degree, pick, n_set = _both(_graph(8, cliques=[(1, 3, 5, 7), (0, 2, 4, 6)]))
    assert n_set == 4 and in_set.tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    assert pick.tolist() == [0, -1, 1, -1, 2, -1, 3, -1] and degree.tolist() == [3] * 8
    # a clique plus a pendant: the pendant's neighbour has the largest degree and goes first
    in_set, degree, pick, n_set = _both(_graph(5, cliques=[(0, 1, 2, 3)], extra=[(2, 4)]))
    assert n_set == 4 and in_set.tolist() == [1, 1, 1, 1, 0]
    assert pick.tolist() == [1, 2, 0, 3, -1] and degree.tolist() == [3, 3, 4, 3, 1]
    # the empty graph: the lowest valid index alone
    in_set, degree, pick, n_set = _both(_graph(4))
    assert n_set == 1 and pick.tolist() == [0, -1, -1, -1] and degree.tolist() == [0] * 4
    valid = np.array([False, True, True, False])
    in_set, degree, pick, n_set = _both(_graph(4), valid)
    assert n_set == 1 and pick.tolist() == [-1, 0, -1, -1] and degree.tolist() == [-1, 0, 0, -1]
    # the max-degree vertex outside the largest clique: greedy follows it and ends smaller than the maximum
    adj = _graph(10, cliques=[(1, 2, 3, 4)], extra=[(0, 5), (0, 6), (0, 7), (0, 8), (0, 9), (5, 6)])
    in_set, degree, pick, n_set = _both(adj)
    assert n_set == 3 and np.flatnonzero(in_set).tolist() == [0, 5, 6] and pick[[0, 5, 6]].tolist() == [0, 1, 2]
    # nothing at all
    in_set, degree, pick, n_set = _both(np.zeros((0, 0), bool), np.zeros(0, bool))
    assert n_set == 0 and in_set.size == 0


def test_pack_rows_layout():
    adj = _graph(70, extra=[(0, 1), (0, 63), (0, 64), (69, 5)])
    rows = cr.pack_rows(adj)
    assert rows.shape == (70, 2) and rows.dtype == np.uint64
    assert int(rows[0, 0]) == (1 << 1) | (1 << 63) and int(rows[0, 1]) == 1
    assert int(rows[69, 0]) == 1 << 5 and int(rows[5, 1]) == 1 << 5
    assert cr.pack_rows(np.zeros((0, 0), bool)).shape == (0, 0)


def test_restatement_arithmetic_order():
    # a sum whose value depends on the order: ((a + b) + c) with a = 1e16, b = -1e16, c = 1 differs from a + (b + c)
    R = np.array([[[1e16, -1e16, 1.0], [0, 1, 0], [0, 0, 1]]])
    one = (np.ones((1, 3, 3)), np.zeros((1, 3)))
    Z = cr.mul((R, np.zeros((1, 3))), one)
    assert Z[0][0, 0, 0] == 1.0
    Ri, ti = cr.inv((np.eye(3)[None] * 2.0, np.array([[1.0, 2.0, 3.0]])))
    assert ti.tolist() == [[-2.0, -4.0, -6.0]] and Ri[0, 1, 1] == 2.0


def test_header_declares_the_calls():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    for name, want in DECLS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name + " is not declared"
        text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        args = [" ".join(a.split()) for a in text.split(",")]
        assert args == want, name
    assert re.search(r"^#define\s+SGTD_MAX_LOOP_EDGES\s+32768\b", header, re.M)
    assert re.search(r"^#define\s+SGTD_LOOP_EDGES_REFINED\s+1\b", header, re.M)


def test_binding_declares_the_calls():
    for name in DECLS:
        assert name in _lib.SYMBOLS, name
    L = _lib.lib()
    vp, dbl, i64, ci = ctypes.c_void_p, ctypes.c_double, ctypes.c_int64, ctypes.c_int
    assert L.sgtd_consistent_loops.argtypes == [vp, i64, vp, vp, vp, vp, dbl, dbl, ctypes.POINTER(ctypes.c_int32)]
    assert L.sgtd_result_consistent.argtypes == [vp, vp, vp, vp, vp]
    assert L.sgtd_result_consistency_rows.argtypes == [vp, i64, i64, vp]
    assert L.sgtd_result_loop_edges.argtypes == [vp, dbl, ci, vp, vp, vp, vp, vp, i64, ctypes.POINTER(i64)]
    for name, want in DECLS.items():
        assert len(getattr(L, name).argtypes) == len(want), name
        assert getattr(L, name).restype is ctypes.c_int
    # a NULL handle is SGTD_ERR_INVALID in all four, without a device
    n_set, n_edges = ctypes.c_int32(0), i64(0)
    assert L.sgtd_consistent_loops(None, 0, None, None, None, None, 1.0, 0.1, ctypes.byref(n_set)) == -1
    assert L.sgtd_result_consistent(None, None, None, None, None) == -1
    assert L.sgtd_result_consistency_rows(None, 0, 0, None) == -1
    assert L.sgtd_result_loop_edges(None, 0.0, 0, None, None, None, None, None, 0, ctypes.byref(n_edges)) == -1
    assert ctypes.sizeof(_lib.Stats) % 8 == 0
