"""sgtd_consistent_loops on the device against the numpy restatement of the rule in include/sgtd_accel.h
(tests/_consistency_ref.py), fed with the thresholds the library hands back.  The bit matrix is compared word for word,
degree, in_set, pick and n_set exactly.  The handles here need no table: the poses are set with set_frame_poses.

The comparison is exact, so the inputs must keep every pair away from the thresholds (the device and numpy round each
operation alike, but nothing here leans on that for a pair that sits on a threshold): every world-based case asserts that
the restatement finds no pair within 1e-9 * max(1, |threshold|) of either threshold.  The cases built to sit ON a
threshold use integer-valued poses, whose arithmetic is exact."""
import ctypes as C

import numpy as np
import pytest

import _consistency_ref as cr

pytestmark = pytest.mark.gpu

TILE = 128           # SGTD_CONS_TILE: columns a workgroup of the pair pass stages
ROWS = 64            # SGTD_CONS_ROWS
PARITY_N = [0, 1, 2, 63, 64, 65, 127, 128, 129, 257, 3 * TILE + 1, 1500]
MAX_TRANS, MAX_ROT = 1.0, np.deg2rad(5.0)


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, evaluate, manager, synth
    return manager, synth, _lib, evaluate


@pytest.fixture(scope="module")
def g(mods):
    h = mods[0].STDescManager()
    yield h
    h.close()


def parity_world(n):
    """n edges: about 70 % true loops, the rest wrong, a fifth of those aliases of one wrong place.  The true loops carry
    0.35 m of noise against the 1 m bound, so their pairs fall on both sides of it: the graph is no plain clique and the
    choice takes many rounds"""
    n_out = (3 * n) // 10
    return cr.planted_world(n - n_out, n_out, n_out // 5, seed=1000 + n, n_frames=max(2 * n, 64), noise_t=0.35)


_refs = {}


def parity_ref(n, thr):
    """the restatement's answer for parity_world(n), computed once"""
    key = (n, float(thr[0]), float(thr[1]))
    if key not in _refs:
        w = parity_world(n)
        _refs[key] = (w, cr.consistent(w["ids"], w["poses"], w["frame_a"], w["frame_b"], w["rel_pose"], thr[0], thr[1]))
    return _refs[key]


def _load(h, ids, poses):
    h.set_frame_poses(None, None)
    h.set_frame_poses(ids, poses)


def _same(got, rows, ref, where=None):
    assert got["n_set"] == ref["n_set"], (where, got["n_set"], ref["n_set"])
    assert rows.shape == ref["rows"].shape and np.array_equal(rows, ref["rows"]), (where, "rows")
    for k in ("degree", "in_set", "pick"):
        assert np.array_equal(got[k], ref[k]), (where, k)


def _run(h, w, max_trans=MAX_TRANS, max_rot=MAX_ROT, pose_a=None, frame_a=True):
    got = h.consistent_loops(w["frame_a"] if frame_a else None, w["frame_b"], w["rel_pose"], max_trans, max_rot, pose_a=pose_a)
    return got, h.consistency_rows()


def _ref_of(w, thr, pose_a=None, clear=True):
    ref = cr.consistent(w["ids"], w["poses"], w["frame_a"], w["frame_b"], w["rel_pose"], thr[0], thr[1], pose_a=pose_a)
    if clear:
        assert cr.clear_of_thresholds(ref, thr[0], thr[1]), (ref["min_gap_d2"], ref["min_gap_tr"])
    return ref


# ---- parity ----
@pytest.mark.parametrize("n", PARITY_N)
def test_parity(g, n):
    w = parity_world(n)
    _load(g, w["ids"], w["poses"])
    got, rows = _run(g, w)
    thr = got["thresholds"]
    assert thr[0] == MAX_TRANS * MAX_TRANS and abs(thr[1] - (1.0 + 2.0 * np.cos(MAX_ROT))) < 1e-15
    w, ref = parity_ref(n, thr)
    assert cr.clear_of_thresholds(ref, thr[0], thr[1]), (n, ref["min_gap_d2"], ref["min_gap_tr"])
    _same(got, rows, ref, n)
    assert rows.shape == (n, (n + 63) // 64)
    if n % 64:
        assert not (rows[:, -1] >> np.uint64(n % 64)).any()         # the padding bits
    if n >= 63:       # the world exercises the rule: pairs on both sides of the bound among the true loops, a choice of many rounds
        t = np.flatnonzero(w["is_true"])
        sub = ref["adj"][np.ix_(t, t)]
        assert 0.2 < sub.mean() < 0.98 and 3 < ref["n_set"] < t.size


# ---- integer-valued worlds: pure translations, exact arithmetic ----
def translation_world(g_shift, seed=3, a=None):
    """edge i: frame_a = i at a_i, frame_b = n + i at b_i (integer positions, identity rotations) and a loop that puts the
    query at a_i + g_shift[i]: the pair (i, j) closes its cycle up to g_shift[j] - g_shift[i], exactly"""
    g_shift = np.asarray(g_shift, np.float64).reshape(-1, 3)
    n = g_shift.shape[0]
    rng = np.random.default_rng(seed)
    a = rng.integers(-500, 500, (n, 3)).astype(np.float64) if a is None else np.asarray(a, np.float64)
    b = rng.integers(-500, 500, (n, 3)).astype(np.float64)
    eye = np.broadcast_to(np.eye(3), (2 * n, 3, 3))
    poses = cr.rows34(eye, np.concatenate([a, b])).astype(np.float32)
    rel = np.zeros((n, 12))
    rel[:, [0, 4, 8]] = 1.0
    rel[:, 9:] = a - b + g_shift
    return {"ids": np.arange(2 * n, dtype=np.uint32), "poses": poses, "frame_a": np.arange(n, dtype=np.uint32),
            "frame_b": np.arange(n, 2 * n, dtype=np.uint32), "rel_pose": rel}


def test_all_pairs_consistent(g):
    """the clique shortcut's path: everything joins, in ascending order"""
    n = 3 * TILE + 7
    w = translation_world(np.zeros((n, 3)))
    _load(g, w["ids"], w["poses"])
    got, rows = _run(g, w, 0.5, 0.1)
    ref = _ref_of(w, got["thresholds"])
    _same(got, rows, ref)
    assert got["n_set"] == n and np.array_equal(got["pick"], np.arange(n)) and (got["degree"] == n - 1).all()
    assert g.stats()["consistency_rounds"] == 1


def test_no_pair_consistent(g):
    n = 200
    shift = np.arange(n)[:, None] * np.array([[3.0, 0.0, 0.0]])
    w = translation_world(shift)
    w["frame_b"][0] = 4_000_000_000          # edge 0 has no pose: the lowest VALID index is 1
    _load(g, w["ids"], w["poses"])
    got, rows = _run(g, w, 1.0, 0.1)
    ref = _ref_of(w, got["thresholds"])
    _same(got, rows, ref)
    assert got["n_set"] == 1 and got["pick"][1] == 0 and got["in_set"].sum() == 1 and not rows.any()
    assert got["degree"][0] == -1 and (got["degree"][1:] == 0).all()


def test_two_equal_cliques(g):
    """two groups of 40 that agree inside and not across; the group holding index 0 wins"""
    n = 80
    grp = (np.arange(n) % 2 == 0)             # even indices: the shifted group, it holds the lowest index
    w = translation_world(np.where(grp[:, None], [[100.0, 0.0, 0.0]], [[0.0, 0.0, 0.0]]))
    _load(g, w["ids"], w["poses"])
    got, rows = _run(g, w, 1.0, 0.1)
    _same(got, rows, _ref_of(w, got["thresholds"]))
    assert got["n_set"] == 40 and np.array_equal(got["in_set"].astype(bool), grp)
    assert np.array_equal(got["pick"][grp], np.arange(40)) and (got["degree"] == 39).all()


def test_greedy_is_not_the_maximum(g):
    """vertex 0 has the largest degree and lies outside the largest clique {1, 2, 3, 4}: the rule follows it"""
    pts = [(0, 0, 0), (1000, 0, 0), (1001, 0, 0), (1000, 1, 0), (1000, 0, 1), (8, 0, 0), (6, 6, 0), (-8, 0, 0), (0, -9, 0), (0, 0, 9)]
    w = translation_world(np.array(pts, np.float64))
    _load(g, w["ids"], w["poses"])
    got, rows = _run(g, w, 10.0, 0.1)
    ref = _ref_of(w, got["thresholds"])
    _same(got, rows, ref)
    assert got["n_set"] == 3 and np.flatnonzero(got["in_set"]).tolist() == [0, 5, 6] and got["pick"][[0, 5, 6]].tolist() == [0, 1, 2]
    assert got["degree"].tolist() == [5, 3, 3, 3, 3, 2, 2, 1, 1, 1]


# ---- validity ----
def test_invalid_edges_are_left_out(g):
    n = 150
    w = parity_world(n)
    bad = {"no_pose_b": 3, "no_pose_a": 40, "beyond_max_frame_n": 64, "beyond_u32_store": 65, "nan_rel": 100, "inf_t": 127, "nan_rot": 149}
    ids, poses = w["ids"].copy(), w["poses"].copy()
    fa, fb, rel = w["frame_a"].copy(), w["frame_b"].copy(), w["rel_pose"].copy()
    hole_b, hole_a, inf_frame = len(ids) + 5, len(ids) + 6, len(ids) + 9          # ids inside the stored range without a pose / with a bad one
    fb[bad["no_pose_b"]] = hole_b
    fa[bad["no_pose_a"]] = hole_a
    fb[bad["beyond_max_frame_n"]] = g.config_setting_["max_frame_n"] + 17
    fa[bad["beyond_u32_store"]] = 0xFFFFFFFF
    rel[bad["nan_rel"], 10] = np.nan
    rel[bad["nan_rot"], 0] = np.nan
    fb[bad["inf_t"]] = inf_frame
    inf_pose = poses[0].copy()
    inf_pose[7] = np.inf
    ids = np.concatenate([ids, [inf_frame, inf_frame + 1]]).astype(np.uint32)
    poses = np.concatenate([poses, inf_pose[None], poses[:1]])
    _load(g, ids, poses)
    wi = dict(w, ids=ids, poses=poses, frame_a=fa, frame_b=fb, rel_pose=rel)
    got, rows = _run(g, wi)
    ref = _ref_of(wi, got["thresholds"])
    _same(got, rows, ref)
    idx = np.array(sorted(bad.values()))
    assert (got["degree"][idx] == -1).all() and (got["pick"][idx] == -1).all() and not got["in_set"][idx].any()
    assert not rows[idx].any()
    for i in idx:                                                        # ... and an empty column
        assert not ((rows[:, i >> 6] >> np.uint64(i & 63)) & np.uint64(1)).any()
    # the others: as in a run without the invalid edges
    keep = np.setdiff1d(np.arange(n), idx)
    wk = dict(wi, frame_a=fa[keep], frame_b=fb[keep], rel_pose=rel[keep])
    got_k, rows_k = _run(g, wk)
    assert got_k["n_set"] == got["n_set"] and (got_k["degree"] >= 0).all()
    for k in ("degree", "in_set", "pick"):
        assert np.array_equal(got_k[k], got[k][keep]), k
    assert np.array_equal(rows_k, cr.pack_rows(ref["adj"][np.ix_(keep, keep)]))


def test_pose_a_without_frame_ids(g):
    n = 130
    w = parity_world(n)
    _load(g, w["ids"], w["poses"])
    base, base_rows = _run(g, w)
    pose_a = w["poses"][w["frame_a"]]
    got, rows = _run(g, w, pose_a=pose_a, frame_a=False)
    _same(got, rows, _ref_of(w, got["thresholds"], pose_a=pose_a))
    _same(got, rows, dict(base, rows=base_rows))
    # pose_a wins over the stored pose of frame_a, and a bad row invalidates its edge alone
    pa = pose_a.copy()
    pa[7, 3] = np.nan
    wrong_ids = np.full(n, 0xFFFFFFF0, np.uint32)
    got2, rows2 = _run(g, dict(w, frame_a=wrong_ids), pose_a=pa)
    _same(got2, rows2, _ref_of(w, got2["thresholds"], pose_a=pa))
    assert got2["degree"][7] == -1 and (np.delete(got2["degree"], 7) >= 0).all()


# ---- thresholds ----
def test_zero_translation_bound_keeps_exact_duplicates(g):
    shift = np.array([[0, 0, 0], [5, 0, 0], [0, 0, 0], [5, 0, 0], [0, 0, 0], [7, 1, 0]], np.float64)
    w = translation_world(shift, a=np.tile([[10.0, -4.0, 2.0]], (6, 1)))
    w["frame_a"][:] = 0                  # exact duplicates: the same frames, the same loop
    w["frame_b"][:] = 6
    w["rel_pose"][:, 9:] = (np.array([10.0, -4.0, 2.0]) - cr.from_rows34(w["poses"][6:7])[1][0]) + shift
    _load(g, w["ids"], w["poses"])
    got, rows = _run(g, w, 0.0, 0.0)
    assert got["thresholds"].tolist() == [0.0, 3.0]
    ref = _ref_of(w, got["thresholds"], clear=False)
    _same(got, rows, ref)
    assert got["degree"].tolist() == [2, 1, 2, 1, 2, 0] and np.flatnonzero(got["in_set"]).tolist() == [0, 2, 4]


def test_rotation_bounds(g):
    n = 140
    w = parity_world(n)
    _load(g, w["ids"], w["poses"])
    # pi: the trace bound is -1, only the translation decides
    got, rows = _run(g, w, 2.0, np.pi)
    assert got["thresholds"][1] == -1.0
    ref = _ref_of(w, got["thresholds"])
    _same(got, rows, ref)
    assert ref["n_set"] > 1
    # 0: the trace bound is 3; a noisy rotation's trace falls short of it or not by rounding alone, so the world is the
    # exact one: identity rotations give tr = 3 exactly and pass through >=
    wt = translation_world(np.zeros((70, 3)))
    _load(g, wt["ids"], wt["poses"])
    got, rows = _run(g, wt, 1.0, 0.0)
    assert got["thresholds"][1] == 3.0
    _same(got, rows, _ref_of(wt, got["thresholds"], clear=False))
    assert got["n_set"] == 70


def test_pair_exactly_on_the_translation_bound(g):
    """d2 = 25 = tt exactly (3, 4, 0) is consistent through <=; (3, 4, 1) is not"""
    w = translation_world(np.array([[0, 0, 0], [3, 4, 0], [-3, -4, -1], [40, 0, 0]], np.float64))
    _load(g, w["ids"], w["poses"])
    got, rows = _run(g, w, 5.0, 0.1)
    assert got["thresholds"][0] == 25.0
    ref = _ref_of(w, got["thresholds"], clear=False)
    assert ref["gap_d2"][0, 1] == 0.0 and ref["adj"][0, 1] and not ref["adj"][0, 2] and ref["gap_d2"][0, 2] == 1.0
    _same(got, rows, ref)
    assert rows[:, 0].tolist() == [0b0010, 0b0001, 0, 0]


# ---- worlds ----
def test_sides_in_different_world_frames(g):
    # exact: the a side moved by a quarter turn about z and an integer translation
    n = 90
    rng = np.random.default_rng(5)
    shift = rng.integers(-2, 3, (n, 3)).astype(np.float64)
    w = translation_world(shift)
    _load(g, w["ids"], w["poses"])
    common, common_rows = _run(g, w, 2.5, 0.1)
    Ra, ta = cr.from_rows34(w["poses"][w["frame_a"]])
    O_R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    O_t = np.array([250.0, -75.0, 12.0])
    odo = cr.rows34(O_R @ Ra, (O_R @ ta[..., None])[..., 0] + O_t).astype(np.float32)
    got, rows = _run(g, w, 2.5, 0.1, pose_a=odo)
    _same(got, rows, dict(common, rows=common_rows))
    _same(got, rows, _ref_of(w, got["thresholds"], pose_a=odo, clear=False))
    assert 1 < got["n_set"] < n
    # a general offset on a noisy world: the restatement's answer
    wp = parity_world(160)
    _load(g, wp["ids"], wp["poses"])
    Ra, ta = cr.from_rows34(wp["poses"][wp["frame_a"]])
    O_R = cr.rot_axis_angle([0.2, -0.1, 1.0], 0.7)
    odo = cr.rows34(O_R @ Ra, (O_R @ ta[..., None])[..., 0] + np.array([31.5, -12.25, 3.0])).astype(np.float32)
    got, rows = _run(g, wp, pose_a=odo)
    ref = _ref_of(wp, got["thresholds"], pose_a=odo)
    _same(got, rows, ref)
    assert ref["n_set"] > 50


# ---- independence ----
def _batch_results(h, nq):
    out = []
    for q in range(nq):
        out += list(h.result_verify(q))
        r, o = h.result_refined(q), h.result_overlap(q)
        out += [r[k] for k in sorted(r)] + [o[k] for k in sorted(o)]
    out += list(h.search_loop())
    return [np.ascontiguousarray(a).tobytes() for a in out]


def test_independent_of_the_pending_batch(mods):
    manager, synth, _lib, ev = mods
    m = synth.make_map(24, 120, stream=3)
    qs = synth.make_queries(m, 3, stream=3)
    h = manager.STDescManager()
    try:
        h.add_frames(m.xyz, m.label, keep_keypoints=True)
        h.set_frame_poses(np.arange(24), np.stack([ev.pose_row(*p) for p in m.pose]))
        h.query_frames(qs.xyz, qs.label)
        h.verify()
        h.refine_poses(1)
        h.overlap(1.0)
        before = _batch_results(h, 3)
        w = translation_world(np.zeros((10, 3)))           # ids 0..19: poses the handle holds
        first = h.consistent_loops(np.arange(10), np.arange(10, 20), w["rel_pose"], 1.0, 0.1)
        assert _batch_results(h, 3) == before
        # a second call replaces the first's results
        second = h.consistent_loops(np.arange(4), np.arange(10, 14), w["rel_pose"][:4], 1000.0, np.pi)
        assert h.consistency_rows().shape == (4, 1) and second["in_set"].size == 4
        assert first["in_set"].size == 10
        rows_before = h.consistency_rows()
        # ... and they survive a new query batch
        h.query_frames(qs.xyz[:2], qs.label[:2])
        h.verify()
        in_set = np.zeros(4, np.int32)
        thr = np.zeros(2)
        assert h._L.sgtd_result_consistent(h._h, in_set.ctypes.data_as(C.c_void_p), None, None, thr.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(in_set, second["in_set"]) and np.array_equal(thr, second["thresholds"])
        assert np.array_equal(h.consistency_rows(), rows_before)
    finally:
        h.close()


# ---- errors ----
def test_errors(mods):
    manager, synth, _lib, _ = mods
    h = manager.STDescManager()
    try:
        L, P = h._L, lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
        w = translation_world(np.zeros((5, 3)))
        h.set_frame_poses(w["ids"], w["poses"])
        fa, fb, rel = w["frame_a"], w["frame_b"], w["rel_pose"]
        pa = w["poses"][:5].copy()
        n_set = C.c_int32(-5)
        out, thr, n_edges = np.zeros(8, np.int32), np.zeros(2), C.c_int64(0)
        rows = np.zeros(8, np.uint64)
        # before any run: STATE
        assert L.sgtd_result_consistent(h._h, P(out), None, None, P(thr)) == -7
        assert L.sgtd_result_consistency_rows(h._h, 0, 0, P(rows)) == -7
        assert L.sgtd_result_loop_edges(h._h, 0.4, 0, None, None, None, None, None, 0, C.byref(n_edges)) == -7
        assert L.sgtd_result_loop_edges(h._h, 0.4, 2, None, None, None, None, None, 0, C.byref(n_edges)) == -1     # unknown flag bits
        allocs = h.stats()["device_allocs_total"]
        call = lambda hh, n, a, b, r, p, mt, mr, ns: L.sgtd_consistent_loops(hh, n, a, b, r, p, mt, mr, ns)          # noqa: E731
        ns = C.byref(n_set)
        invalid = [
            (None, 5, P(fa), P(fb), P(rel), None, 1.0, 0.1, ns),
            (h._h, -1, P(fa), P(fb), P(rel), None, 1.0, 0.1, ns),
            (h._h, 5, P(fa), None, P(rel), None, 1.0, 0.1, ns),
            (h._h, 5, P(fa), P(fb), None, None, 1.0, 0.1, ns),
            (h._h, 5, None, P(fb), P(rel), None, 1.0, 0.1, ns),
            (h._h, 5, P(fa), P(fb), P(rel), None, 1.0, 0.1, None),
            (h._h, 5, P(fa), P(fb), P(rel), None, float("nan"), 0.1, ns),
            (h._h, 5, P(fa), P(fb), P(rel), None, -0.5, 0.1, ns),
            (h._h, 5, P(fa), P(fb), P(rel), None, float("inf"), 0.1, ns),
            (h._h, 5, P(fa), P(fb), P(rel), None, 1.0, float("nan"), ns),
            (h._h, 5, P(fa), P(fb), P(rel), None, 1.0, -0.01, ns),
            (h._h, 5, P(fa), P(fb), P(rel), None, 1.0, 3.2, ns),
            (h._h, 0, None, None, None, None, float("nan"), 0.1, ns),
        ]
        for k, a in enumerate(invalid):
            assert call(*a) == -1, k
        assert h.stats()["device_allocs_total"] == allocs
        assert L.sgtd_result_consistent(h._h, P(out), None, None, P(thr)) == -7        # (still no results)
        # too many edges: UNSUPPORTED with a message
        big = 32768 + 1
        assert call(h._h, big, P(np.zeros(big, np.uint32)), P(np.zeros(big, np.uint32)), P(np.zeros((big, 12))), None, 1.0, 0.1, ns) == -6
        assert b"32768" in L.sgtd_last_error(h._h)
        assert L.sgtd_result_consistent(h._h, P(out), None, None, P(thr)) == -7
        # n == 0 with NULL arrays is a run: nothing is done
        assert call(h._h, 0, None, None, None, None, 1.0, 0.1, ns) == 0 and n_set.value == 0
        assert L.sgtd_result_consistent(h._h, None, None, None, P(thr)) == 0 and thr[0] == 1.0
        assert L.sgtd_result_consistency_rows(h._h, 0, 0, None) == 0
        assert L.sgtd_result_consistency_rows(h._h, 0, 1, P(rows)) == -1
        # pose_a with frame_a NULL is fine; the rows' range is checked against n
        assert call(h._h, 5, None, P(fb), P(rel), P(pa), 1.0, 0.1, ns) == 0 and n_set.value == 5
        assert L.sgtd_result_consistency_rows(h._h, 0, 5, P(rows)) == 0 and rows[:5].tolist() == [30, 29, 27, 23, 15]
        assert L.sgtd_result_consistency_rows(h._h, 4, 1, P(rows)) == 0 and rows[0] == 15
        assert L.sgtd_result_consistency_rows(h._h, 5, 0, P(rows)) == 0
        for first, cnt in ((-1, 1), (0, 6), (5, 1), (6, 0), (0, -1), (3, 3)):
            assert L.sgtd_result_consistency_rows(h._h, first, cnt, P(rows)) == -1, (first, cnt)
        assert L.sgtd_result_consistency_rows(h._h, 0, 5, None) == -1
        # a failed call drops the results
        assert call(h._h, big, P(np.zeros(big, np.uint32)), P(np.zeros(big, np.uint32)), P(np.zeros((big, 12))), None, 1.0, 0.1, ns) == -6
        assert L.sgtd_result_consistent(h._h, P(out), None, None, P(thr)) == -7
    finally:
        h.close()


# ---- views and groups ----
def test_view_and_single_device_group(mods, g):
    manager, synth, _lib, _ = mods
    w = parity_world(129)
    _load(g, w["ids"], w["poses"])
    base, base_rows = _run(g, w)
    m = synth.make_map(16, 120, stream=3)
    owner, view = manager.STDescManager(), manager.STDescManager()
    grp = manager.STDescManager(devices=[0])
    try:
        owner.add_frames(m.xyz[:8], m.label[:8])
        owner.finalize()
        view.attach_table(owner)
        view.set_frame_poses(w["ids"], w["poses"])
        owner.add_frames(m.xyz[8:], m.label[8:])           # the owner's table changes: the view's table calls are STATE now
        with pytest.raises(_lib.SgtdError) as ei:
            view.query_frames(m.xyz[:1], m.label[:1])
        assert ei.value.status == -7
        got, rows = _run(view, w)
        _same(got, rows, dict(base, rows=base_rows))
        with pytest.raises(_lib.SgtdError):                # the owner holds no poses: its own run sees no valid edge
            owner.consistency_rows()
        own, _ = _run(owner, w)
        assert own["n_set"] == 0 and (own["degree"] == -1).all()
        grp.set_frame_poses(w["ids"], w["poses"])
        got, rows = _run(grp, w)
        _same(got, rows, dict(base, rows=base_rows))
    finally:
        view.close()
        owner.close()
        grp.close()


# ---- end to end ----
def test_loop_session_end_to_end(mods):
    """a closed session of 120 frames 4 m apart (synth's trajectory runs out along an arc and back over it, so the second
    half revisits the first): loop_frames, verify, loop_edges, then the joint check over the session's poses with three
    aliased edges injected.  The joint check runs twice, with bounds from the poses' own accuracy:
    verify()'s pose is the motion of ONE triangle pair; keypoints carry 2 cm of noise and a triangle's sides go down to
    about half a metre, so its rotation is good to atan(0.028 / 0.5), some 3 to 4 degrees, only.  A rotation error acts
    over the lever arm between the two loops' query frames, up to some 100 m here: two such loops close their cycle
    within 2 * 0.07 rad * 100 m = 14 m and 8 degrees.  Bounds: 15 m, 10 degrees.
    refine_poses' pose averages over hundreds to thousands of inlier pairs: millimetres and hundredths of a degree for
    the loops to a frame nearby, 0.02 deg * 100 m = 4 cm over the lever arm.  Bounds: 2 m, 5 degrees, as a back end
    would set them.  The injected edges are off by more than 50 m in both runs."""
    manager, synth, _lib, ev = mods
    F = 120
    m = synth.make_map(F, 200, stream=431, spacing=4.0)
    rows = np.stack([ev.pose_row(*p) for p in m.pose]).astype(np.float32)
    h = manager.STDescManager()
    try:
        h.set_frame_poses(np.arange(F), rows)
        h.loop_frames(m.xyz, m.label, skip_near=30, batch=F)
        h.verify()
        with pytest.raises(_lib.SgtdError) as ei:
            h.loop_edges(refined=True)
        assert ei.value.status == -7
        e = h.loop_edges()
        bc, bf, bs = h.search_loop()
        acc = np.flatnonzero(bc >= 0)
        assert np.array_equal(e["query"], acc) and np.array_equal(e["frame_a"], acc) and np.array_equal(e["frame_b"], bf[acc])
        assert np.array_equal(e["score"], bs[acc])
        for k, q in enumerate(acc):
            score, rot, t = h.result_verify(int(q))
            assert np.array_equal(e["rel_pose"][k, :9], rot[bc[q]].reshape(9)) and np.array_equal(e["rel_pose"][k, 9:], t[bc[q]])
        h.refine_poses(1)
        er = h.loop_edges(refined=True)
        assert np.array_equal(er["query"], e["query"]) and np.array_equal(er["frame_b"], e["frame_b"])
        for k, q in enumerate(acc):
            r = h.result_refined(int(q))
            assert np.array_equal(er["rel_pose"][k, :9], r["rot"][bc[q]].reshape(9)) and np.array_equal(er["rel_pose"][k, 9:], r["t"][bc[q]])
        # capacity: the count is still reported, the first edges written
        n_edges = C.c_int64(0)
        q1 = np.full(1, -1, np.int32)
        st = h._L.sgtd_result_loop_edges(h._h, h.icp_threshold_, 0, q1.ctypes.data_as(C.c_void_p), None, None, None, None, 1, C.byref(n_edges))
        assert n_edges.value == acc.size and (st == -4 if acc.size > 1 else st == 0) and q1[0] == acc[0]
        # the joint check: every loop to a frame within 5 m of the query's true position stays, the aliases go
        dist = np.hypot(*(m.pose[e["frame_a"], :2] - m.pose[e["frame_b"], :2]).T)
        near = dist <= 5.0
        assert near.sum() >= 3, (acc.size, np.sort(dist)[:8])
        src = np.flatnonzero(near)[:3]
        # the same loop claimed against the frame farthest from the true one (more than 50 m off)
        far = np.array([np.argmax(np.hypot(*(m.pose[:, :2] - m.pose[b, :2]).T)) for b in e["frame_b"][src]])
        assert (np.hypot(*(m.pose[far, :2] - m.pose[e["frame_b"][src], :2]).T) > 50.0).all()
        for edges, max_trans, max_rot in ((e, 15.0, np.deg2rad(10.0)), (er, 2.0, np.deg2rad(5.0))):
            fa = np.concatenate([edges["frame_a"], edges["frame_a"][src]]).astype(np.uint32)
            fb = np.concatenate([edges["frame_b"], far]).astype(np.uint32)
            rel = np.concatenate([edges["rel_pose"], edges["rel_pose"][src]])
            got = h.consistent_loops(fa, fb, rel, max_trans, max_rot)
            ref = cr.consistent(np.arange(F), rows, fa, fb, rel, *got["thresholds"])
            _same(got, h.consistency_rows(), ref, max_trans)
            assert not got["in_set"][acc.size:].any(), max_trans
            assert got["in_set"][:acc.size][near].all(), (max_trans, dist[near], got["in_set"][:acc.size][near])
    finally:
        h.close()
