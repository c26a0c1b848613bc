"""sgtd_set_frame_filter / STDescManager.set_frame_filter: with a filter set, each query must be answered exactly as by a
handle that holds only that query's allowed frames (same ids, same order, same current_frame_id_).  Yardsticks: the
oracle that added only the allowed frames, and a copy of the map from which the other frames were removed
(sgtd_remove_frames), compared bit for bit — candidates, full vote arrays, ordered match lists (entries mapped by their
rank among the allowed frames' entries), candidate_verify, SearchLoop's choice, sgtd_search_frame and the rough list."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 200
SPACING = 25.0
# query q re-observes frame GT[q]; WIN[q] is its window (three distinct ones; the last query's excludes its own place)
GT = np.array([10, 70, 130, 30, 100, 180, 50, 150])
WINDOWS = [np.arange(0, 80), np.arange(60, 140), np.arange(120, 200)]
WIN = [0, 1, 2, 0, 1, 2, 0, 0]
SHARED = np.array(sorted(set(range(0, 120)) - {3, 17, 64, 65, 66, 100}) + [150, 151, 199])
DESC_FIELDS = ("side", "angle", "center", "vertex", "label", "frame", "node_id")


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from sgtd_amd import _lib, evaluate, manager, synth
    oracle.build_library()
    return oracle, manager, synth, _lib, evaluate


@pytest.fixture(scope="module")
def world(mods):
    oracle, _, synth, _, _ = mods
    m = synth.make_map(F, 200, stream=311, spacing=SPACING)
    qs = synth.make_queries(m, len(GT), stream=312, frames=GT)
    descs = []
    o = oracle.OracleManager()
    for i in range(F):
        o.set_current_frame_id(i)
        descs.append(o.build(m.xyz[i], m.label[i]))
    return m, descs, qs


def _oracle_with(oracle, descs, frames, current):
    o = oracle.OracleManager()
    for f in frames:
        o.add(descs[f])
    o.set_current_frame_id(current)
    return o


def _entry_map(counts, frames):
    """full-table entry index -> the index the same entry has in a table of only `frames` (in order)"""
    full_off = np.concatenate([[0], np.cumsum(counts)])
    keep = np.zeros(len(counts), bool)
    keep[np.asarray(frames, np.int64)] = True
    sub_off = np.concatenate([[0], np.cumsum(np.where(keep, counts, 0))])

    def f(e):
        e = np.asarray(e, np.int64)
        fr = np.searchsorted(full_off, e, side="right") - 1
        assert keep[fr].all(), "an entry of a frame that is not allowed"
        return sub_off[fr] + (e - full_off[fr])
    return f


def _full_votes(lo, v, n):
    out = np.zeros(n, np.int64)
    out[lo:lo + len(v)] = v
    return out


def _same_votes(lo_a, va, lo_b, vb):
    n = max(lo_a + len(va), lo_b + len(vb))
    return np.array_equal(_full_votes(lo_a, va, n), _full_votes(lo_b, vb, n))


def _new(manager, m, n=None, **kw):
    g = manager.STDescManager(**kw)
    g.add_frames(m.xyz[:n] if n else m.xyz, m.label[:n] if n else m.label)
    g.finalize()
    return g


def _check_against_oracle(oracle, descs, g, res, bc, bf, bs, qs, allowed, rough=(), icp=0.4, held=None):
    """held: the frames the handle's table holds (entry ids number these), all of them by default"""
    counts = np.array([d.n for d in descs])
    if held is not None:
        counts = np.where(np.isin(np.arange(F), held), counts, 0)
    for q in range(qs.xyz.shape[0]):
        frames = np.sort(np.asarray(allowed[q]))
        o = _oracle_with(oracle, descs, frames, F)
        o.build(qs.xyz[q], qs.label[q], export=False)
        r = o.select()
        nc = len(r["cand_frame"])
        assert int(res.n_cand[q]) == nc, q
        assert np.array_equal(res.cand_frame[q, :nc], r["cand_frame"]), q
        assert np.array_equal(res.cand_votes[q, :nc], r["cand_votes"]), q
        assert np.array_equal(res.pair_off[q, :nc + 1], r["cand_off"]), q
        qi, de = g.result_pairs(q, res)
        emap = _entry_map(counts, frames)
        assert np.array_equal(qi, r["q_idx"]) and np.array_equal(emap(de), r["db_entry"]), q
        lo, v = g.result_votes(q)
        assert _same_votes(lo, v, 0, o.votes()), q
        best_s, best_k = 0.0, -1
        score, rot, t = g.result_verify(q)
        for k in range(nc):
            s, o_t, o_rot, _ = o.verify(k, int(r["cand_off"][k + 1] - r["cand_off"][k]))
            assert score[k] == s, (q, k)
            if s >= 0:
                assert np.array_equal(t[k], o_t) and np.array_equal(rot[k], o_rot), (q, k)
            if s > best_s:
                best_s, best_k = s, k
        f = int(r["cand_frame"][best_k]) if best_s > icp else -1
        assert int(bf[q]) == f and float(bs[q]) == (best_s if f >= 0 else 0.0), q
        if f >= 0:
            assert int(bc[q]) == best_k
    # the rough lists last: the diagnostic re-run replaces the batch's verification
    for q in rough:
        frames = np.sort(np.asarray(allowed[q]))
        o = _oracle_with(oracle, descs, frames, F)
        o.build(qs.xyz[q], qs.label[q], export=False)
        o.select()
        gr, orr = g.result_rough(q), o.rough_matches()
        for k in ("q_idx", "cell", "frame", "dis"):
            assert np.array_equal(gr[k], orr[k]), (k, q)
        assert np.array_equal(_entry_map(counts, frames)(gr["db_entry"]), orr["db_entry"]), q
    return res


def test_oracle_parity_shared_and_per_query(mods, world):
    oracle, manager, _, _, _ = mods
    m, descs, qs = world
    g = _new(manager, m)
    nq = len(GT)
    # one row for the whole batch
    g.set_frame_filter(SHARED)
    res = g.query_frames(qs.xyz, qs.label)
    g.verify()
    bc, bf, bs = g.search_loop(0.4)
    _check_against_oracle(oracle, descs, g, res, bc, bf, bs, qs, [SHARED] * nq, rough=(0,))
    assert int(np.sum(res.n_cand > 0)) > 0
    # one row per query: three distinct windows
    per_q = [WINDOWS[w] for w in WIN]
    g.set_frame_filter(per_q)
    res = g.query_frames(qs.xyz, qs.label)
    g.verify()
    bc, bf, bs = g.search_loop(0.4)
    _check_against_oracle(oracle, descs, g, res, bc, bf, bs, qs, per_q, rough=(1, 7))
    for q in range(nq):
        assert np.isin(res.cand_frame[q, :res.n_cand[q]], per_q[q]).all()
    assert int(np.sum(bf >= 0)) >= 5
    g.close()


def _same_results(a, b, ra, rb, nq, entry_map=None, verify=True, icp=0.4):
    """handle a (batch ra) and handle b (batch rb) answered alike; entry_map maps a's entries to b's"""
    for k in ("n_cand", "cand_frame", "cand_votes", "pair_off"):
        assert np.array_equal(getattr(ra, k), getattr(rb, k)), k
    if verify:
        a.verify()
        b.verify()
        sa, sb = a.search_loop(icp), b.search_loop(icp)
        for x, y in zip(sa, sb):
            assert np.array_equal(x, y)
    for q in range(nq):
        qa, da = a.result_pairs(q, ra)
        qb, db = b.result_pairs(q, rb)
        assert np.array_equal(qa, qb), q
        assert np.array_equal(entry_map(da) if entry_map else da, db), q
        la, va = a.result_votes(q)
        lb, vb = b.result_votes(q)
        assert _same_votes(la, va, lb, vb), q
        if verify:
            s1, r1, t1 = a.result_verify(q)
            s2, r2, t2 = b.result_verify(q)
            assert np.array_equal(s1, s2) and np.array_equal(r1, r2) and np.array_equal(t1, t2), q


def test_equals_removal_on_10000_frames(mods):
    _, manager, synth, _lib, _ = mods
    big = 10000
    m = synth.make_map(big, 200, stream=1)
    qs = synth.make_queries(m, 256, stream=313)
    rng = np.random.default_rng(21)
    gone = np.union1d(np.arange(2000, 4500), rng.choice(big, 1500, replace=False))
    allowed = np.setdiff1d(np.arange(big), gone)
    a, b = _new(manager, m), _new(manager, m)
    b.remove_frames(gone)
    a.set_frame_filter(allowed)
    ra, rb = a.query_frames(qs.xyz, qs.label), b.query_frames(qs.xyz, qs.label)
    assert a.stats()["last_M"] == b.stats()["last_M"]          # the batch's match count M
    # entries per frame, from the handle's own table (the frame field alone)
    E = a.stats()["n_entries"]
    fr = np.zeros(E, np.uint32)
    soa = _lib.DescSoa()
    soa.frame = fr.ctypes.data
    idx = np.arange(E, dtype=np.int64)
    assert a._L.sgtd_fetch_entries(a._h, idx.ctypes.data, E, ctypes.byref(soa)) == 0
    counts = np.bincount(fr.astype(np.int64), minlength=big)
    _same_results(a, b, ra, rb, 256, entry_map=_entry_map(counts, allowed))
    assert int(np.sum(ra.n_cand > 0)) > 50
    assert not np.isin(ra.cand_frame[ra.cand_frame >= 0], gone).any()
    a.close()
    b.close()


def test_identity_cases(mods, world):
    _, manager, _, _, _ = mods
    m, _, qs = world
    g = _new(manager, m)
    r0 = g.query_frames(qs.xyz, qs.label)
    g.verify()
    s0 = g.search_loop(0.4)
    ref = [(g.result_pairs(q, r0), g.result_votes(q), g.result_verify(q)) for q in range(len(GT))]
    st0 = g.stats()

    def same_as_unfiltered(res):
        for k in ("n_cand", "cand_frame", "cand_votes", "pair_off"):
            assert np.array_equal(getattr(res, k), getattr(r0, k)), k
        g.verify()
        for x, y in zip(g.search_loop(0.4), s0):
            assert np.array_equal(x, y)
        for q in range(len(GT)):
            (qa, da), (la, va), (sa, ra_, ta) = ref[q]
            qb, db = g.result_pairs(q, res)
            lb, vb = g.result_votes(q)
            sb, rb_, tb = g.result_verify(q)
            assert np.array_equal(qa, qb) and np.array_equal(da, db) and la == lb and np.array_equal(va, vb), q
            assert np.array_equal(sa, sb) and np.array_equal(ra_, rb_) and np.array_equal(ta, tb), q
        assert g.stats()["last_M"] == st0["last_M"] and g.stats()["last_P"] == st0["last_P"]

    # every frame allowed, with a range wider than the table
    g.set_frame_filter(np.ones((1, F + 300), bool))
    same_as_unfiltered(g.query_frames(qs.xyz, qs.label))
    # cleared: the unfiltered results again
    g.set_frame_filter(None)
    same_as_unfiltered(g.query_frames(qs.xyz, qs.label))
    # the keyword form leaves no filter behind
    g.query_frames(qs.xyz, qs.label, allowed=[5])
    same_as_unfiltered(g.query_frames(qs.xyz, qs.label))
    # nothing allowed: no candidates, no loop, M = 0, every vote 0 (the visits still count the whole map)
    g.set_frame_filter([])
    res = g.query_frames(qs.xyz, qs.label)
    assert np.all(res.n_cand == 0)
    g.verify()
    _, bf, _ = g.search_loop(0.4)
    assert np.all(bf == -1)
    assert g.stats()["last_M"] == 0 and g.stats()["last_P"] == st0["last_P"]
    for q in range(len(GT)):
        assert not g.result_votes(q)[1].any()
    g.close()


def test_scope_later_adds_remove_and_load(mods, world, tmp_path):
    oracle, manager, _, _, _ = mods
    m, descs, qs = world
    g = _new(manager, m, n=150)
    # [40, 150): frames 150.. added later are outside the range
    g.set_frame_filter(np.arange(40, 150))
    g.add_frames(m.xyz[150:], m.label[150:])
    res = g.query_frames(qs.xyz, qs.label)
    assert not (res.cand_frame[res.cand_frame >= 0] >= 150).any()
    assert int(np.sum(res.n_cand > 0)) > 0
    g.verify()
    bc, bf, bs = g.search_loop(0.4)
    _check_against_oracle(oracle, descs, g, res, bc, bf, bs, qs, [np.arange(40, 150)] * len(GT))
    # global ids survive sgtd_remove_frames (the table's frame_lo moves) and save / load
    g.remove_frames(np.arange(0, 50))
    res = g.query_frames(qs.xyz, qs.label)
    g.verify()
    bc, bf, bs = g.search_loop(0.4)
    _check_against_oracle(oracle, descs, g, res, bc, bf, bs, qs, [np.arange(50, 150)] * len(GT), held=np.arange(50, F))
    g.save_table(tmp_path / "t.tab")
    h = manager.STDescManager()
    h.load_table(tmp_path / "t.tab")
    h.set_frame_filter(np.arange(40, 150))
    g.load_table(tmp_path / "t.tab")              # (the filter set before the load stays)
    for x in (g, h):
        res = x.query_frames(qs.xyz, qs.label)
        x.verify()
        bc, bf, bs = x.search_loop(0.4)
        _check_against_oracle(oracle, descs, x, res, bc, bf, bs, qs, [np.arange(50, 150)] * len(GT), held=np.arange(50, F))
    g.close()
    h.close()


@pytest.mark.parametrize("lists_only", [False, True])
def test_search_frame_with_filter(mods, world, lists_only):
    oracle, manager, _, _, _ = mods
    m, descs, qs = world
    g = _new(manager, m)
    counts = np.array([d.n for d in descs])
    n_found = 0
    for q in range(len(GT)):
        allowed = WINDOWS[WIN[q]]
        d = g.BuildSingleScanSTD(qs.xyz[q], qs.label[q])
        fs = g.search_frame(d, capacity=1 << 16, lists_only=lists_only, allowed=allowed)
        assert fs["status"] == 0
        # the same call through query_descs + verify + search_loop under the same filter
        g.set_frame_filter(allowed)
        lists = g.candidate_selector(d)
        nc = fs["n_cand"]
        assert nc == len(lists)
        assert [int(x.match_id_[1]) for x in lists] == fs["cand_frame"][:nc].tolist()
        assert [x.votes for x in lists] == fs["cand_votes"][:nc].tolist()
        if lists_only:
            qi = np.concatenate([x.q_idx for x in lists]) if lists else np.zeros(0, np.int32)
            de = np.concatenate([x.db_entry for x in lists]) if lists else np.zeros(0, np.int64)
            assert np.array_equal(fs["inlier_q_idx"], qi)
            ent = g.fetch_entries(de)
            for f in DESC_FIELDS:
                assert np.array_equal(getattr(fs["entries"], f), getattr(ent, f)), f
        else:
            g.verify()
            bc, bf, bs = g.search_loop(0.4)
            score, rot, t = g.result_verify(0)
            assert np.array_equal(fs["score"][:nc], score[:nc])
            assert np.array_equal(fs["rot"][:nc], rot[:nc]) and np.array_equal(fs["t"][:nc], t[:nc])
        g.set_frame_filter(None)
        # and the oracle of the allowed frames
        o = _oracle_with(oracle, descs, allowed, F)
        o.build(qs.xyz[q], qs.label[q], export=False)
        r = o.select()
        assert np.array_equal(fs["cand_frame"][:nc], r["cand_frame"]) and np.array_equal(fs["pair_off"][:nc + 1], r["cand_off"])
        if lists_only:
            assert np.array_equal(_entry_map(counts, allowed)(de), r["db_entry"])
        n_found += nc > 0
    assert n_found >= 5
    g.close()


def test_rough_list_equals_removed_handle(mods, world):
    _, manager, _, _, _ = mods
    m, descs, qs = world
    gone = np.setdiff1d(np.arange(F), SHARED)
    a, b = _new(manager, m), _new(manager, m)
    b.remove_frames(gone)
    a.set_frame_filter(SHARED)
    ra, rb = a.query_frames(qs.xyz, qs.label), b.query_frames(qs.xyz, qs.label)
    emap = _entry_map(np.array([d.n for d in descs]), SHARED)
    n = 0
    for q in range(len(GT)):
        x, y = a.result_rough(q), b.result_rough(q)
        for k in ("q_idx", "cell", "frame", "dis"):
            assert np.array_equal(x[k], y[k]), (k, q)
        assert np.array_equal(emap(x["db_entry"]), y["db_entry"]), q
        n += len(x["q_idx"])
    assert n > 0
    # the diagnostic re-run answers as before: the lists are the removed handle's too
    _same_results(a, b, a.results(), b.results(), len(GT), entry_map=emap, verify=False)
    a.close()
    b.close()


def test_three_shard_handle(mods, world):
    _, manager, _, _, _ = mods
    m, descs, qs = world
    per_q = [WINDOWS[w] for w in WIN]
    per_q[3] = np.array([5, 63, 64, 127, 128, 129, 191, 192])      # across the 64-frame shard blocks
    single = _new(manager, m)
    multi = _new(manager, m, devices=[0, 0, 0])
    for h in (single, multi):
        h.set_frame_filter(per_q)
    a, b = single.query_frames(qs.xyz, qs.label), multi.query_frames(qs.xyz, qs.label)
    for k in ("n_cand", "cand_frame", "cand_votes", "pair_off"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    single.verify()
    multi.verify()
    for x, y in zip(single.search_loop(0.4), multi.search_loop(0.4)):
        assert np.array_equal(x, y)
    n = 0
    for q in range(len(GT)):
        qa, da = single.result_pairs(q, a)
        qb, db = multi.result_pairs(q, b)
        assert np.array_equal(qa, qb), q
        if len(da):
            ea, eb = single.fetch_entries(da), multi.fetch_entries(db)
            for f in DESC_FIELDS:
                assert np.array_equal(getattr(ea, f), getattr(eb, f)), f
        n += len(da)
        la, va = single.result_votes(q)
        lb, vb = multi.result_votes(q)
        assert _same_votes(la, va, lb, vb), q
    assert n > 0
    multi.close()
    single.close()


def test_errors(mods, world):
    _, manager, synth, _lib, _ = mods
    m, _, qs = world
    g = _new(manager, m)
    g.set_frame_filter([np.arange(10), np.arange(20), np.arange(30)])
    with pytest.raises(_lib.SgtdError) as ei:
        g.query_frames(qs.xyz, qs.label)             # 8 queries, 3 rows
    assert ei.value.status == -1
    d = g.BuildSingleScanSTD(qs.xyz[0], qs.label[0])
    with pytest.raises(_lib.SgtdError) as ei:
        g.candidate_selector(d)                     # a batch of one
    assert ei.value.status == -1
    g.query_frames(qs.xyz[:3], qs.label[:3])        # the right size works
    with pytest.raises(_lib.SgtdError) as ei:
        g.loop_frames(qs.xyz[:2], qs.label[:2])
    assert ei.value.status == -7
    assert g.current_frame_id_ == F                 # nothing was added
    L = g._L
    assert L.sgtd_set_frame_filter(g._h, 0, 0, np.ones(1, np.uint64).ctypes.data, 1) == -1
    assert L.sgtd_set_frame_filter(g._h, 0, 64, None, 1) == -1
    assert L.sgtd_set_frame_filter(g._h, 0, 64, None, -2) == -1
    g.set_frame_filter(None)
    g.loop_frames(qs.xyz[:2], qs.label[:2])
    g.close()


def test_prior_end_to_end(mods):
    _, manager, synth, _, ev = mods
    smap = synth.make_map(1500, 200, stream=314)
    q = synth.make_queries(smap, 96, stream=315)
    map_pose = np.stack([ev.pose_matrix(*p) for p in smap.pose])
    q_pose = np.stack([ev.pose_matrix(*p) for p in q.pose])
    prior = ev.frames_near(smap.pose[:, :2], q.pose[:, :2], 50.0)
    assert 5 < prior.sum(axis=1).mean() < 200
    mgr = _new(manager, smap)
    base = ev.evaluate_batch(mgr, map_pose, q.xyz, q.label, q_pose)
    filt = ev.evaluate_batch(mgr, map_pose, q.xyz, q.label, q_pose, allowed=prior)
    mgr.query_frames(q.xyz, q.label, allowed=prior)
    mgr.verify()
    _, bf, _ = mgr.search_loop()
    for i in range(len(bf)):
        if bf[i] >= 0:
            assert prior[i, bf[i]], i
    assert filt.score_num >= base.score_num and filt.total_num == base.total_num == 96
    assert base.score_num > 48
    mgr.close()
