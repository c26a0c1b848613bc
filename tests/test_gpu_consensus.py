"""sgtd_pose_consensus on the device against the numpy restatement of the rule in include/sgtd_accel.h
(tests/_consensus_ref.py), fed with the thresholds the library hands back.  Every output is compared exactly: the rows
word for word, the integers as they are, the doubles bit for bit.

The comparison is exact, so the inputs must keep every pair away from the thresholds: every noise-based case asserts
that the restatement finds no pair within 1e-9 * max(1, |threshold|) of either threshold (the planted batches' seeds were
chosen for that).  The cases built to sit ON a threshold use integer-valued poses, whose arithmetic is exact."""
import ctypes as C

import numpy as np
import pytest

import _consensus_ref as ref
import _consistency_ref as cr

pytestmark = pytest.mark.gpu

MAX_TRANS, MAX_ROT = 0.5, np.deg2rad(5.0)
PARITY_NQ = [0, 1, 3, 4, 5, 257]
PARITY_CN = [1, 2, 50, 64]
INT_KEYS = ("n_valid", "n_set", "seed", "mask")
DBL_KEYS = ("pose", "support_score", "spread_t2", "spread_trace")
F, NQ = 60, 8


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, evaluate, manager, synth
    return manager, synth, _lib, evaluate


@pytest.fixture(scope="module")
def g(mods):
    h = mods[0].STDescManager()
    yield h
    h.close()


@pytest.fixture(scope="module")
def world(mods):
    _, synth, _, ev = mods
    m = synth.make_map(F, 200, stream=511, spacing=6.0)
    qs = synth.make_queries(m, 2 * NQ, stream=512)
    rows = np.stack([ev.pose_row(*p) for p in m.pose])
    return m, qs, rows


def _new(manager, m, rows, **kw):
    h = manager.STDescManager(**kw)
    h.add_frames(m.xyz, m.label, keep_keypoints=True)
    h.finalize()
    h.set_frame_poses(np.arange(len(rows)), rows)
    return h


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _status(_lib, call, *a, **kw):
    with pytest.raises(_lib.SgtdError) as ei:
        call(*a, **kw)
    return ei.value.status


def _load(h, b):
    h.set_frame_poses(None, None)
    h.set_frame_poses(b["ids"], b["poses"])


def _rows(h, b, max_trans=MAX_TRANS, max_rot=MAX_ROT):
    return h.pose_consensus_rows(b["n_cand"], b["cand_frame"], b["score"], b["rel_pose"], max_trans, max_rot)


def _ref_of(b, thr, clear=True, shortcut=False):
    r = ref.consensus(b["ids"], b["poses"], b["n_cand"], b["cand_frame"], b["score"], b["rel_pose"], thr[0], thr[1], shortcut)
    if clear:
        assert ref.clear_of_thresholds(r, thr[0], thr[1]), (r["min_gap_d2"], r["min_gap_tr"])
    return r


def _same(h, got, want, where=None):
    """every output of the call against the restatement's"""
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), (where, k, got[k], want[k])
    for k in DBL_KEYS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (where, k)
    for q in range(want["n_set"].size):
        rows, degree, pick = h.consensus_rows(q)
        assert np.array_equal(rows, want["rows"][q]), (where, q, "rows")
        assert np.array_equal(degree, want["degree"][q]) and np.array_equal(pick, want["pick"][q]), (where, q)


_planted = {}


def planted(nq, cn):
    if (nq, cn) not in _planted:
        _planted[(nq, cn)] = ref.planted_batch(nq, cn, seed=7000 + 100 * cn + nq)
    return _planted[(nq, cn)]


# ---- parity through the rows form ----
@pytest.mark.parametrize("cn", PARITY_CN)
@pytest.mark.parametrize("nq", PARITY_NQ)
def test_parity(g, nq, cn):
    b = planted(nq, cn)
    _load(g, b)
    got = _rows(g, b)
    thr = got["thresholds"]
    assert thr[0] == MAX_TRANS * MAX_TRANS and abs(thr[1] - (1.0 + 2.0 * np.cos(MAX_ROT))) < 1e-15
    want = _ref_of(b, thr)
    if nq > 16:      # (the getter's ranges; the per-query rows of a few queries)
        part = g.result_consensus(5, 9)
        for k in INT_KEYS:
            assert np.array_equal(part[k], want[k][5:14]), k
        assert np.array_equal(_bits(part["pose"]), _bits(want["pose"][5:14]))
        for k in INT_KEYS:
            assert np.array_equal(got[k], want[k]), k
        for k in DBL_KEYS:
            assert np.array_equal(_bits(got[k]), _bits(want[k])), k
        for q in list(range(0, nq, 9)) + [nq - 1]:
            rows, degree, pick = g.consensus_rows(q)
            assert np.array_equal(rows, want["rows"][q]) and np.array_equal(degree, want["degree"][q]) and np.array_equal(pick, want["pick"][q]), q
    else:
        _same(g, got, want, (nq, cn))
    if nq >= 3:
        assert b["n_cand"][2] == 0 and got["n_set"][2] == 0 and got["seed"][2] == -1 and np.isnan(got["pose"][2]).all()
        assert got["n_valid"][1] == 0 and got["mask"][1] == 0 and got["support_score"][1] == 0.0
    if nq == 257 and cn == 64:
        assert (got["mask"] >> np.uint64(63)).any() and (got["n_set"] >= 5).sum() > 50      # candidate 63 in a set


def test_parity_many_rounds(g):
    """0.2 m of noise against the 0.5 m bound: the pairs of a true group fall on both sides of it, the graph is no plain
    clique and the choice takes many picks before the shortcut, if it fires at all"""
    b = ref.planted_batch(33, 64, seed=902, noise_t=0.2)
    _load(g, b)
    got = _rows(g, b)
    want = _ref_of(b, got["thresholds"])
    _same(g, got, want)
    dens = [want["adj"][q][np.ix_(b["kind"][q] == 0, b["kind"][q] == 0)].mean() for q in range(33) if (b["kind"][q] == 0).sum() > 3]
    assert 0.3 < np.mean(dens) < 0.8 and want["pick"].max() >= 10
    again = _ref_of(b, got["thresholds"], shortcut=True)          # the shortcut is the rule
    assert np.array_equal(again["pick"], want["pick"]) and np.array_equal(again["mask"], want["mask"])


def test_candidate_63_valid_member_and_seed(g):
    tt = 9.0
    xs = [None] * 64
    xs[10], xs[20], xs[30], xs[40], xs[63] = 0, 0, 5, 5, 3
    seed63 = ref.line_batch(xs)
    member63 = ref.line_batch([None] * 60 + [7, 8, 9, 9])                     # a clique of the last four: the shortcut
    alone63 = ref.line_batch([None] * 63 + [4])
    b = ref.stack([seed63, member63, alone63])
    _load(g, b)
    got = _rows(g, b, 3.0, 0.1)
    assert got["thresholds"][0] == tt
    want = _ref_of(b, got["thresholds"], clear=False)
    _same(g, got, want)
    assert got["seed"].tolist() == [63, 60, 63] and got["n_set"].tolist() == [3, 4, 1]
    assert int(got["mask"][0]) == (1 << 63) | (1 << 20) | (1 << 10) and int(got["mask"][1]) == 0xF << 60 and int(got["mask"][2]) == 1 << 63
    rows, degree, pick = g.consensus_rows(0)
    assert int(rows[63]) == (1 << 10) | (1 << 20) | (1 << 30) | (1 << 40) and degree[63] == 4 and pick[63] == 0
    assert g.consensus_rows(1)[2][60:].tolist() == [0, 1, 2, 3]


# ---- thresholds ----
def test_pair_exactly_on_the_translation_bound(g):
    """d2 == tt agrees through <=; the next double above tt does not"""
    on = ref.line_batch([0, 1])
    above = ref.line_batch([0, 1])
    above["rel_pose"][0, 1, 10] = 2.0 ** -26            # d2 = 1 + 2^-52, exactly
    below = ref.line_batch([0, 1])
    below["rel_pose"][0, 0, 10] = 2.0 ** -26            # the pair taken with the lower index first: the same d2
    b = ref.stack([on, above, below])
    _load(g, b)
    got = _rows(g, b, 1.0, 0.1)
    assert got["thresholds"][0] == 1.0
    want = _ref_of(b, got["thresholds"], clear=False)
    assert want["adj"][0, 0, 1] and not want["adj"][1, 0, 1] and not want["adj"][2, 0, 1]
    _same(g, got, want)
    assert got["n_set"].tolist() == [2, 1, 1] and g.consensus_rows(0)[0].tolist() == [2, 1] and not g.consensus_rows(1)[0].any()


def test_rotation_bounds(g):
    b = planted(5, 50)
    _load(g, b)
    got = _rows(g, b, 2.0, np.pi)           # pi: the trace bound is -1, only the translation decides
    assert got["thresholds"][1] == -1.0
    _same(g, got, _ref_of(b, got["thresholds"]))
    # 0: the bound is 3; identity rotations give tr = 3 exactly and pass through >=
    bt = ref.line_batch([0, 1, 2, 9])
    _load(g, bt)
    got = _rows(g, bt, 2.0, 0.0)
    assert got["thresholds"].tolist() == [4.0, 3.0]
    _same(g, got, _ref_of(bt, got["thresholds"], clear=False))
    assert got["n_set"][0] == 3 and got["spread_trace"][0] == 3.0
    # a noisy batch under a zero rotation bound: nothing agrees (no pair sits on 3 by the clearance condition)
    _load(g, b)
    got = _rows(g, b, 2.0, 0.0)
    _same(g, got, _ref_of(b, got["thresholds"]))
    assert (got["n_set"] <= 1).all()


def test_tie_rule_and_shortcut(g):
    # two groups of equal size: the one holding the lowest index wins; a clique joins in ascending order
    tie = ref.line_batch([100, 0, 101, 1, 102, 2], cn=8)
    clique = ref.line_batch([0, 1, 2, 1, 0, 2, 1, 0])
    pendant = ref.line_batch([0, 1, 2, 3, 6, None, 1, 2])         # no clique at the start: picks, then the shortcut
    b = ref.stack([tie, clique, pendant])
    _load(g, b)
    got = _rows(g, b, 3.0, 0.1)
    for shortcut in (False, True):
        _same(g, got, _ref_of(b, got["thresholds"], clear=False, shortcut=shortcut))
    assert g.consensus_rows(0)[2].tolist() == [0, -1, 1, -1, 2, -1, -1, -1] and got["seed"][0] == 0
    assert got["pose"][0].tolist() == [1, 0, 0, 101, 0, 1, 0, 0, 0, 0, 1, 0] and got["spread_t2"][0] == 1.0
    assert g.consensus_rows(1)[2].tolist() == list(range(8)) and got["n_set"][1] == 8


# ---- the batch form ----
@pytest.fixture(scope="module")
def batch(mods, world):
    manager, _, _, _ = mods
    m, qs, rows = world
    h = _new(manager, m, rows)
    res = h.query_frames(qs.xyz[:NQ], qs.label[:NQ])
    h.verify()
    h.refine_poses(1)
    h.align_keypoints(1.0, iterations=5)
    yield h, res
    h.close()


def _stage_arrays(h, nq, which):
    """score (nq, cn) and rel_pose (nq, cn, 12) as the stage's getter gives them"""
    score, rel = [], []
    for q in range(nq):
        s, rot, t = h.result_verify(q)
        if which == "refined":
            r = h.result_refined(q)
            rot, t = r["rot"], r["t"]
        elif which == "aligned":
            r = h.result_aligned(q)
            rot, t = r["rot"], r["t"]
        score.append(s)
        rel.append(np.concatenate([rot.reshape(-1, 9), t.reshape(-1, 3)], axis=1))
    return np.stack(score), np.stack(rel)


BATCH_TRANS, BATCH_ROT = 2.0, np.deg2rad(10.0)


@pytest.mark.parametrize("which", ["verify", "refined", "aligned"])
def test_batch_form(batch, world, which):
    h, res = batch
    m, qs, rows = world
    got = h.pose_consensus(BATCH_TRANS, BATCH_ROT, refined=which == "refined", aligned=which == "aligned")
    per_q = [h.consensus_rows(q) for q in range(NQ)]
    score, rel = _stage_arrays(h, NQ, which)
    b = {"ids": np.arange(F, dtype=np.uint32), "poses": rows, "n_cand": res.n_cand, "cand_frame": res.cand_frame, "score": score, "rel_pose": rel}
    want = _ref_of(b, got["thresholds"])
    _same(h, got, want, which)
    # the rows form fed with the getters' arrays: the same, and independent of the pending batch
    again = _rows(h, b, BATCH_TRANS, BATCH_ROT)
    for k in INT_KEYS:
        assert np.array_equal(got[k], again[k]), k
    for k in DBL_KEYS:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), k
    for q in range(NQ):
        for x, y in zip(per_q[q], h.consensus_rows(q)):
            assert np.array_equal(x, y), q
    # the batch exercises the rule: several verified candidates agree on the place they came from
    assert (got["n_set"] >= 2).sum() >= NQ // 2 and got["n_valid"].max() >= 3


def test_cross_check_with_consistent_loops(batch, world):
    """one query's candidates as edges under one pose_a: the rows, pick and in_set of sgtd_consistent_loops"""
    h, res = batch
    got = h.pose_consensus(BATCH_TRANS, BATCH_ROT)
    q = int(np.argmax(got["n_valid"]))
    rows, degree, pick = h.consensus_rows(q)
    mask = int(got["mask"][q])
    score, rel = _stage_arrays(h, NQ, "verify")
    v = np.flatnonzero(degree >= 0)
    assert v.size >= 3
    eye = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (v.size, 1))
    c = h.consistent_loops(None, res.cand_frame[q][v].astype(np.uint32), rel[q][v], BATCH_TRANS, BATCH_ROT, pose_a=eye)
    crow = h.consistency_rows()[:, 0]
    for i, k in enumerate(v):
        want_row = sum(1 << j for j, l in enumerate(v) if (int(rows[k]) >> int(l)) & 1)
        assert int(crow[i]) == want_row, k
        assert c["pick"][i] == pick[k] and c["degree"][i] == degree[k] and c["in_set"][i] == (mask >> int(k)) & 1, k
    assert c["n_set"] == got["n_set"][q]
    h.pose_consensus(BATCH_TRANS, BATCH_ROT)      # (the consistency call left the consensus results alone; leave fresh ones)


def test_search_and_edges(batch, world, mods):
    h, res = batch
    _lib = mods[2]
    m, qs, rows = world
    got = h.pose_consensus(BATCH_TRANS, BATCH_ROT, refined=True)
    score = _stage_arrays(h, NQ, "verify")[0]
    ids = np.arange(F, dtype=np.uint32)
    q0 = int(np.argmax(got["n_set"]))
    for min_support in (1, 2, int(got["n_set"][q0]), int(got["n_set"][q0]) + 1):
        bc, bf, bs, sup = h.search_loop_consensus(min_support)
        assert np.array_equal(sup, got["n_set"])
        edges = h.consensus_edges(min_support)
        e = 0
        for q in range(NQ):
            if got["n_set"][q] < min_support:
                assert (bc[q], bf[q], bs[q]) == (-1, -1, 0.0)
                continue
            mem = ref.members_of(got["mask"][q], score.shape[1])
            k = int(mem[np.argmax(score[q][mem])])              # (argmax: the first of the largest)
            assert (bc[q], bf[q], bs[q]) == (k, res.cand_frame[q][k], score[q][k])
            assert edges["query"][e] == q and edges["frame_b"][e] == res.cand_frame[q][k] and edges["frame_a"][e] == res.query_frame_id
            assert edges["score"][e] == got["support_score"][q]
            assert np.array_equal(_bits(edges["rel_pose"][e]), _bits(ref.edge_pose(ids, rows, res.cand_frame[q][k], got["pose"][q])))
            e += 1
        assert e == edges["query"].size
    assert h.search_loop_consensus(int(got["n_set"][q0]))[0][q0] >= 0 and h.search_loop_consensus(int(got["n_set"][q0]) + 1)[0][q0] == -1
    # capacity: the count comes back, the first entries are written
    full = h.consensus_edges(1)
    n = full["query"].size
    assert n >= 2
    assert _status(_lib, h.consensus_edges, 1, capacity=n - 1) == -4
    # the edges feed sgtd_consistent_loops unchanged
    eye = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (n, 1))
    c = h.consistent_loops(None, full["frame_b"], full["rel_pose"], 1000.0, np.pi, pose_a=eye)
    assert c["n_set"] == n


# ---- handles and lifetime ----
def _batch_results(h, nq):
    out = []
    for q in range(nq):
        out.append([_bits(x).tolist() for x in h.result_verify(q)])
        r = h.result_refined(q)
        out.append([_bits(r["rot"]).tolist(), _bits(r["rmse"]).tolist()])
    out.append([x.tolist() for x in h.search_loop(4.0)])
    return out


def test_lifetime_and_errors(mods, world):
    manager, _, _lib, _ = mods
    m, qs, rows = world
    h = _new(manager, m, rows)
    b = ref.line_batch([0, 1, 2, 9])
    # state errors before any run
    assert _status(_lib, h.result_consensus) == -7 and _status(_lib, h.consensus_rows, 0) == -7
    assert _status(_lib, h.search_loop_consensus, 1) == -7 and _status(_lib, h.consensus_edges, 1) == -7
    assert _status(_lib, h.pose_consensus, 1.0, 0.1) == -7                  # no batch
    res = h.query_frames(qs.xyz[:NQ], qs.label[:NQ])
    assert _status(_lib, h.pose_consensus, 1.0, 0.1) == -7                  # no verification
    h.verify()
    assert _status(_lib, h.pose_consensus, 1.0, 0.1, refined=True) == -7    # the stage named by the flag has not run
    assert _status(_lib, h.pose_consensus, 1.0, 0.1, aligned=True) == -7
    h.refine_poses(1)
    # argument errors
    L, hp = h._L, h._h
    assert L.sgtd_pose_consensus(hp, 1.0, 0.1, 3) == -1 and L.sgtd_pose_consensus(hp, 1.0, 0.1, 4) == -1
    for mt, mr in ((np.nan, 0.1), (-1.0, 0.1), (np.inf, 0.1), (1.0, np.nan), (1.0, -0.1), (1.0, 3.2)):
        assert L.sgtd_pose_consensus(hp, mt, mr, 0) == -1, (mt, mr)
        assert _status(_lib, _rows, h, b, mt, mr) == -1, (mt, mr)
    p = manager._p
    nc, cf, sc, rel = b["n_cand"], b["cand_frame"], b["score"], b["rel_pose"]
    assert L.sgtd_pose_consensus_rows(hp, -1, 4, p(nc), p(cf), p(sc), p(rel), 1.0, 0.1) == -1
    for cn in (0, 65, -3):
        assert L.sgtd_pose_consensus_rows(hp, 1, cn, p(nc), p(cf), p(sc), p(rel), 1.0, 0.1) == -1
    for args in ((None, p(cf), p(sc), p(rel)), (p(nc), None, p(sc), p(rel)), (p(nc), p(cf), None, p(rel)), (p(nc), p(cf), p(sc), None)):
        assert L.sgtd_pose_consensus_rows(hp, 1, 4, *args, 1.0, 0.1) == -1
    assert L.sgtd_pose_consensus_rows(hp, 0, 4, None, None, None, None, 1.0, 0.1) == 0       # nothing to do
    assert L.sgtd_result_consensus(hp, 0, 0, *([None] * 9)) == 0 and L.sgtd_result_consensus(hp, 0, 1, *([None] * 9)) == -1
    # other results are unchanged after the call
    before = _batch_results(h, 3)
    got = h.pose_consensus(BATCH_TRANS, BATCH_ROT)
    assert _batch_results(h, 3) == before
    assert _status(_lib, h.search_loop_consensus, 0) == -1 and _status(_lib, h.consensus_edges, 0) == -1
    n_edges = C.c_int64(0)
    assert L.sgtd_result_consensus_edges(hp, 1, None, None, None, None, None, -1, C.byref(n_edges)) == -1
    assert L.sgtd_result_consensus_edges(hp, 1, None, None, None, None, None, 0, None) == -1
    assert L.sgtd_result_consensus_edges(hp, 1, None, None, None, None, None, 0, C.byref(n_edges)) in (0, -4) and n_edges.value >= 1
    assert L.sgtd_result_consensus(hp, NQ, 1, *([None] * 9)) == -1 and L.sgtd_result_consensus(hp, -1, 1, *([None] * 9)) == -1
    assert L.sgtd_result_consensus(hp, 0, NQ, *([None] * 9)) == 0
    assert _status(_lib, h.consensus_rows, NQ) == -1 and _status(_lib, h.consensus_rows, -1) == -1
    # a failed call drops the results
    assert L.sgtd_pose_consensus(hp, -1.0, 0.1, 0) == -1
    assert _status(_lib, h.result_consensus) == -7
    # the rows form's results: no batch stands behind them, and they survive a new batch
    _load(h, b)
    r4 = _rows(h, b, 2.0, 0.1)
    assert r4["n_set"].tolist() == [3] and _status(_lib, h.search_loop_consensus, 1) == -7
    h.query_frames(qs.xyz[:2], qs.label[:2])
    h.verify()
    assert h.result_consensus()["n_set"].tolist() == [3]
    h.set_frame_poses(np.arange(len(rows)), rows)
    # the batch form's results drop after a new verification and after a new batch
    h.pose_consensus(BATCH_TRANS, BATCH_ROT)
    assert h.result_consensus()["n_set"].size == 2
    h.verify()
    assert _status(_lib, h.result_consensus) == -7
    h.pose_consensus(BATCH_TRANS, BATCH_ROT)
    h.query_frames(qs.xyz[:3], qs.label[:3])
    assert _status(_lib, h.result_consensus) == -7 and _status(_lib, h.search_loop_consensus, 1) == -7
    h.close()


def test_view_and_three_shards(mods, world):
    manager, _, _lib, _ = mods
    m, qs, rows = world
    single, multi = _new(manager, m, rows), _new(manager, m, rows, devices=[0, 0, 0])
    a, b = single.query_frames(qs.xyz[:NQ], qs.label[:NQ]), multi.query_frames(qs.xyz[:NQ], qs.label[:NQ])
    assert np.array_equal(a.cand_frame, b.cand_frame)
    for h in (single, multi):
        h.verify()
        assert _status(_lib, h.pose_consensus, 1.0, 0.1, refined=True) == -7
        h.refine_poses(1)
        h.align_keypoints(1.0, iterations=5)
    for kw in ({}, {"refined": True}, {"aligned": True}):
        ra, rb = single.pose_consensus(BATCH_TRANS, BATCH_ROT, **kw), multi.pose_consensus(BATCH_TRANS, BATCH_ROT, **kw)
        for k in INT_KEYS:
            assert np.array_equal(ra[k], rb[k]), (kw, k)
        for k in DBL_KEYS + ("thresholds",):
            assert np.array_equal(_bits(ra[k]), _bits(rb[k])), (kw, k)
        for q in range(NQ):
            for x, y in zip(single.consensus_rows(q), multi.consensus_rows(q)):
                assert np.array_equal(x, y), (kw, q)
        for x, y in zip(single.search_loop_consensus(2), multi.search_loop_consensus(2)):
            assert np.array_equal(x, y), kw
        ea, eb = single.consensus_edges(2), multi.consensus_edges(2)
        assert np.array_equal(_bits(ea["rel_pose"]), _bits(eb["rel_pose"])) and np.array_equal(ea["frame_b"], eb["frame_b"])
        assert (ra["n_set"] >= 2).any()
    multi.verify()
    assert _status(_lib, multi.result_consensus) == -7
    multi.close()
    # a view: its own poses, its own results
    want = single.pose_consensus(BATCH_TRANS, BATCH_ROT)
    v = manager.STDescManager()
    v.attach_table(single)
    v.query_frames(qs.xyz[:NQ], qs.label[:NQ])
    v.verify()
    assert _status(_lib, v.result_consensus) == -7               # (the owner's pass is not the view's)
    none = v.pose_consensus(BATCH_TRANS, BATCH_ROT)              # the view has no poses stored
    assert not none["n_valid"].any() and np.isnan(none["pose"]).all()
    v.set_frame_poses(np.arange(len(rows)), rows)
    mine = v.pose_consensus(BATCH_TRANS, BATCH_ROT)
    for k in INT_KEYS:
        assert np.array_equal(mine[k], want[k]), k
    assert np.array_equal(_bits(mine["pose"]), _bits(want["pose"]))
    assert np.array_equal(_bits(single.result_consensus()["pose"]), _bits(want["pose"]))
    v.close()
    single.close()


def test_evaluate_consensus(mods, world):
    """evaluate.evaluate_consensus books the fused pose beside SearchLoop's choice on the same batch"""
    manager, _, _, ev = mods
    m, qs, rows = world
    h = _new(manager, m, rows)
    map4 = np.stack([ev.pose_matrix(*p) for p in m.pose])
    gt4 = np.stack([ev.pose_matrix(*p) for p in qs.pose[:NQ]])
    out = ev.evaluate_consensus(h, map4, qs.xyz[:NQ], qs.label[:NQ], gt4, BATCH_TRANS, BATCH_ROT, min_support=2)
    got = h.result_consensus()
    cons, sl = out["consensus"], out["search_loop"]
    assert cons["queries"] == sl["queries"] == NQ and cons["support"] == got["n_set"].tolist()
    assert cons["accepted"] == int((got["n_set"] >= 2).sum()) >= NQ // 2 and len(cons["t_errors"]) == cons["accepted"]
    assert cons["wrong"] == 0 and max(cons["t_errors"]) < 5.0 and max(cons["r_errors"]) < 10.0
    assert sl["accepted"] == int((h.search_loop()[1] > 0).sum())
    h.close()
