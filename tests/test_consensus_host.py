"""sgtd_pose_consensus without a device: the numpy restatement of the rule (tests/_consensus_ref.py) on a planted batch,
the properties that follow from the rule, the header's prototypes and the ctypes binding."""
import ctypes
import os
import re

import numpy as np

import _consensus_ref as ref
import _consistency_ref as cr
from sgtd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_pose_consensus_rows": ["sgtd_handle h", "int64_t n_queries", "int cand_num", "const int32_t *n_cand", "const int32_t *cand_frame",
                                 "const double *score", "const double *rel_pose", "double max_trans", "double max_rot"],
    "sgtd_pose_consensus": ["sgtd_handle h", "double max_trans", "double max_rot", "int flags"],
    "sgtd_result_consensus": ["sgtd_handle h", "int64_t first", "int64_t n", "double *pose", "int32_t *n_valid", "int32_t *n_set",
                              "int32_t *seed", "uint64_t *mask", "double *support_score", "double *spread_t2", "double *spread_trace",
                              "double *thresholds"],
    "sgtd_result_consensus_rows": ["sgtd_handle h", "int q", "uint64_t *rows", "int32_t *degree", "int32_t *pick"],
    "sgtd_search_loop_consensus": ["sgtd_handle h", "int min_support", "int32_t *best_cand", "int32_t *best_frame", "double *best_score",
                                   "int32_t *support"],
    "sgtd_result_consensus_edges": ["sgtd_handle h", "int min_support", "int32_t *query", "uint32_t *frame_a", "uint32_t *frame_b",
                                    "double *rel_pose", "double *score", "int64_t capacity", "int64_t *n_edges"],
}

MAX_TRANS, MAX_ROT = 0.5, np.deg2rad(5.0)


def _planted(nq=24, cn=50, seed=11):
    b = ref.planted_batch(nq, cn, seed)
    tt, min_trace = cr.thresholds(MAX_TRANS, MAX_ROT)
    r = ref.consensus(b["ids"], b["poses"], b["n_cand"], b["cand_frame"], b["score"], b["rel_pose"], tt, min_trace)
    return b, r, tt, min_trace


def test_planted_batch_holds_every_kind():
    b, r, tt, min_trace = _planted()
    kinds = set(np.unique(b["kind"]).tolist())
    assert kinds == {ref.KIND_TRUE, ref.KIND_ALIAS, ref.KIND_LONER, ref.KIND_REJECTED, ref.KIND_NO_POSE, ref.KIND_NAN_POSE, ref.KIND_PAST}
    assert b["n_cand"][2] == 0 and r["n_valid"][2] == 0
    assert b["n_cand"][1] > 0 and r["n_valid"][1] == 0
    # validity is the header's: only the first three kinds are valid
    assert np.array_equal(r["valid"], b["kind"] <= ref.KIND_LONER)
    assert ref.clear_of_thresholds(r, tt, min_trace)


def test_true_group_wins_and_alias_only_where_larger():
    b, r, tt, min_trace = _planted()
    seen_true = seen_alias = 0
    for q in range(b["n_cand"].size):
        members = ref.members_of(r["mask"][q], 50)
        n_true = int((b["kind"][q] == ref.KIND_TRUE).sum())
        n_alias = int((b["kind"][q] == ref.KIND_ALIAS).sum())
        assert members.size == r["n_set"][q]
        if r["n_valid"][q] == 0:
            assert members.size == 0 and r["seed"][q] == -1 and np.isnan(r["pose"][q]).all() and r["support_score"][q] == 0.0
            assert np.isnan(r["spread_t2"][q]) and np.isnan(r["spread_trace"][q])
            continue
        # members are pairwise adjacent
        assert r["adj"][q][np.ix_(members, members)].sum() == members.size * (members.size - 1)
        if n_true > n_alias:
            assert np.array_equal(members, np.flatnonzero(b["kind"][q] == ref.KIND_TRUE)), q
            seen_true += 1
            # the fused pose is the true one up to the noise
            assert np.linalg.norm(r["pose"][q].reshape(3, 4)[:, 3] - b["true_pose"][1][q]) < 0.1
        elif n_alias > n_true:
            assert np.array_equal(members, np.flatnonzero(b["kind"][q] == ref.KIND_ALIAS)), q
            seen_alias += 1
        assert r["seed"][q] in members and r["pick"][q][r["seed"][q]] == 0
        assert sorted(r["pick"][q][members]) == list(range(members.size))
        assert r["support_score"][q] == b["score"][q][members].sum()        # (small integers: exact in any order)
    assert seen_true >= 10 and seen_alias >= 2


def test_spreads_stay_inside_the_bounds():
    # a mean lies inside a set of pairwise diameter <= max_trans; for max_rot <= 90 degrees the normalised quaternion
    # sum lies within max_rot of every member
    b, r, tt, min_trace = _planted()
    some = 0
    for q in range(b["n_cand"].size):
        if r["n_set"][q] == 0:
            continue
        members = ref.members_of(r["mask"][q], 50)
        that = r["pose"][q].reshape(3, 4)[:, 3]
        d2 = ((r["world"][1][q][members] - that) ** 2).sum(1)
        assert (d2 <= tt * (1 + 1e-9)).all()
        assert abs(d2.max() - r["spread_t2"][q]) <= 1e-9 * max(1.0, d2.max())
        assert r["spread_trace"][q] >= min_trace - 1e-9 * max(1.0, abs(min_trace))
        Rh = r["pose"][q].reshape(3, 4)[:, :3]
        assert np.allclose(Rh @ Rh.T, np.eye(3), atol=1e-12)
        some += 1
    assert some >= 15


def test_adjacency_is_consistent_loops_under_one_pose_a():
    # the query's valid candidates as edges that share one pose_a: the same decisions, the same greedy choice
    b, r, tt, min_trace = _planted(nq=9, cn=50, seed=5)
    eye = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    for q in range(9):
        v = np.flatnonzero(r["valid"][q])
        if v.size == 0:
            continue
        c = cr.consistent(b["ids"], b["poses"], None, b["cand_frame"][q][v].astype(np.uint32), b["rel_pose"][q][v], tt, min_trace,
                          pose_a=np.tile(eye, (v.size, 1)))
        assert c["valid"].all()
        assert np.array_equal(c["adj"], r["adj"][q][np.ix_(v, v)])
        assert np.array_equal(c["degree"], r["degree"][q][v]) and np.array_equal(c["pick"], r["pick"][q][v])
        assert np.array_equal(np.flatnonzero(c["in_set"]), np.searchsorted(v, ref.members_of(r["mask"][q], 50)))


def test_tie_rule_shortcut_and_seed_63():
    tt, min_trace = cr.thresholds(3.0, 0.1)
    # two groups of equal size 10 apart: the one holding the lowest index wins
    b = ref.line_batch([100, 0, 101, 1, 102, 2])
    for shortcut in (False, True):
        r = ref.consensus(b["ids"], b["poses"], b["n_cand"], b["cand_frame"], b["score"], b["rel_pose"], tt, min_trace, shortcut)
        assert r["pick"][0].tolist() == [0, -1, 1, -1, 2, -1] and r["seed"][0] == 0 and int(r["mask"][0]) == 0b010101
        assert r["pose"][0].tolist() == [1, 0, 0, 101, 0, 1, 0, 0, 0, 0, 1, 0]
        assert r["spread_t2"][0] == 1.0 and r["spread_trace"][0] == 3.0 and r["support_score"][0] == 10 + 12 + 14
    # candidate 63 between two pairs agrees with all four and is the seed; the pair with the lower index follows
    xs = [None] * 64
    xs[10], xs[20], xs[30], xs[40], xs[63] = 0, 0, 5, 5, 3
    b = ref.line_batch(xs)
    r = ref.consensus(b["ids"], b["poses"], b["n_cand"], b["cand_frame"], b["score"], b["rel_pose"], tt, min_trace)
    assert r["seed"][0] == 63 and int(r["mask"][0]) == (1 << 63) | (1 << 20) | (1 << 10)
    assert r["pick"][0][[63, 10, 20]].tolist() == [0, 1, 2] and r["degree"][0][63] == 4
    assert int(r["rows"][0][63]) == (1 << 10) | (1 << 20) | (1 << 30) | (1 << 40) and int(r["rows"][0][10]) == (1 << 63) | (1 << 20)


def test_header_declares_the_calls():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    for name, want in DECLS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name + " is not declared"
        text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        args = [" ".join(a.split()) for a in text.split(",")]
        assert args == want, name
    assert re.search(r"^#define\s+SGTD_CONSENSUS_REFINED\s+1\b", header, re.M)
    assert re.search(r"^#define\s+SGTD_CONSENSUS_ALIGNED\s+2\b", header, re.M)


def test_binding_declares_the_calls():
    for name in DECLS:
        assert name in _lib.SYMBOLS, name
    L = _lib.lib()
    vp, dbl, i64, ci = ctypes.c_void_p, ctypes.c_double, ctypes.c_int64, ctypes.c_int
    assert L.sgtd_pose_consensus_rows.argtypes == [vp, i64, ci, vp, vp, vp, vp, dbl, dbl]
    assert L.sgtd_pose_consensus.argtypes == [vp, dbl, dbl, ci]
    assert L.sgtd_result_consensus.argtypes == [vp, i64, i64] + [vp] * 9
    assert L.sgtd_result_consensus_rows.argtypes == [vp, ci, vp, vp, vp]
    assert L.sgtd_search_loop_consensus.argtypes == [vp, ci, vp, vp, vp, vp]
    assert L.sgtd_result_consensus_edges.argtypes == [vp, ci, vp, vp, vp, vp, vp, i64, ctypes.POINTER(i64)]
    for name, want in DECLS.items():
        assert len(getattr(L, name).argtypes) == len(want), name
        assert getattr(L, name).restype is ctypes.c_int
    # a NULL handle is SGTD_ERR_INVALID in all six, without a device
    n_edges = i64(0)
    assert L.sgtd_pose_consensus_rows(None, 0, 1, None, None, None, None, 1.0, 0.1) == -1
    assert L.sgtd_pose_consensus(None, 1.0, 0.1, 0) == -1
    assert L.sgtd_result_consensus(None, 0, 0, None, None, None, None, None, None, None, None, None) == -1
    assert L.sgtd_result_consensus_rows(None, 0, None, None, None) == -1
    assert L.sgtd_search_loop_consensus(None, 1, None, None, None, None) == -1
    assert L.sgtd_result_consensus_edges(None, 1, None, None, None, None, None, 0, ctypes.byref(n_edges)) == -1
