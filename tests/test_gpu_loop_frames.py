"""Sequence loop detection (sgtd_loop_frames / STDescManager.loop_frames) against the reference's per-frame loop
build -> SearchLoop -> AddSTDescs, driven through the oracle: frame i is built with frame id i and selects against the
table the reference holds at step i — every frame added before it, minus the skip_near frames just before it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SEQ = 300
N_MAP = 150          # prebuilt map, then a session of as many frames
# (frames 25 m apart on the closed trajectory: it still revisits every place, and the oracle's host-side selects stay
# within seconds — at 2 m consecutive frames overlap almost entirely and a select returns 10^5 pairs)
SPACING = 25.0
VERIFY_SAMPLE = sorted(int(i) for i in np.random.default_rng(5).choice(N_SEQ, 64, replace=False))
ROUGH_FRAMES = (0, 25, 120, N_SEQ - 1)


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from sgtd_amd import _lib, manager, synth
    oracle.build_library()
    return oracle, manager, synth, _lib


@pytest.fixture(scope="module")
def seq(mods):
    """N_SEQ frames of one closed trajectory (it revisits places) and their oracle descriptors (frame ids 0..N_SEQ-1)"""
    oracle, _, synth, _ = mods
    m = synth.make_map(N_SEQ, 200, stream=211, spacing=SPACING)
    return m, _oracle_descs(oracle, m.xyz, m.label, 0)


@pytest.fixture(scope="module")
def ref(mods, seq):
    """the oracle's loop over the sequence, once per skip_near (verification and rough lists where the tests need them)"""
    oracle = mods[0]
    descs = seq[1]
    cache = {}

    def get(skip):
        if skip not in cache:
            cache[skip] = _oracle_loop(oracle, descs, skip, verify=VERIFY_SAMPLE if skip == 0 else (),
                                       rough=ROUGH_FRAMES if skip == 20 else ())
        return cache[skip]
    return get


@pytest.fixture(scope="module")
def session(mods):
    """N_MAP map frames, then a session of N_MAP frames from another stream over the same places (frame ids N_MAP..),
    with the oracle's loop over the session on top of the map"""
    oracle, _, synth, _ = mods
    mp = synth.make_map(N_MAP, 200, stream=223, spacing=SPACING)
    ss = synth.make_queries(mp, N_MAP, stream=224, frames=np.arange(N_MAP)[::-1])
    sdescs = _oracle_descs(oracle, ss.xyz, ss.label, N_MAP)
    sel, _, _ = _oracle_loop(oracle, sdescs, 0, map_xyz=mp.xyz, map_label=mp.label)
    return mp, ss, sel


def _oracle_descs(oracle, xyz, label, first):
    o = oracle.OracleManager()
    out = []
    for i in range(xyz.shape[0]):
        o.set_current_frame_id(first + i)
        out.append(o.build(xyz[i], label[i]))
    return out


def _oracle_loop(oracle, descs, skip, map_xyz=None, map_label=None, verify=(), rough=(), icp=0.4):
    """the oracle through the reference's loop: before frame i selects, the table holds the map (if any) and the frames
    j < i - skip.  -> per frame select(); for the frames in `verify` SearchLoop's choice and every candidate's score and
    pose; for the frames in `rough` rough_matches()"""
    o = oracle.OracleManager()
    if map_xyz is not None:
        o.add_frames(map_xyz, map_label)
    sel, ver, rgh = [], {}, {}
    added = 0
    for i, d in enumerate(descs):
        while added < i - skip:
            o.add(descs[added])
            added += 1
        r = o.select(d)
        sel.append(r)
        if i in rough:
            rgh[i] = o.rough_matches()
        if i in verify:
            cands = []
            best_s, best_k = 0.0, -1
            for k in range(len(r["cand_frame"])):
                s, t, rot, _ = o.verify(k, int(r["cand_off"][k + 1] - r["cand_off"][k]))
                cands.append((s, t, rot))
                if s > best_s:
                    best_s, best_k = s, k
            if best_s > icp:       # the first candidate with the strictly largest score (STDesc.cpp:105-146)
                choice = (best_k, int(r["cand_frame"][best_k]), best_s)
            else:
                choice = (None, -1, 0.0)
            ver[i] = (cands, choice)
    return sel, ver, rgh


def _same_as_oracle(g, res, sel, q0=0, pairs=True):
    """frames q0.. of the last loop batch (res: its BatchResult) against the oracle's selects, list for list"""
    for i, r in enumerate(sel):
        q = q0 + i
        nc = len(r["cand_frame"])
        assert int(res.n_cand[q]) == nc, q
        assert np.array_equal(res.cand_frame[q, :nc], r["cand_frame"]), q
        assert np.array_equal(res.cand_votes[q, :nc], r["cand_votes"]), q
        assert np.array_equal(res.pair_off[q, :nc + 1], r["cand_off"]), q
        if pairs:
            qi, de = g.result_pairs(q, res)
            assert np.array_equal(qi, r["q_idx"]) and np.array_equal(de, r["db_entry"]), q


@pytest.mark.parametrize("skip", [0, 50])
def test_sequence_equals_the_reference_loop(mods, seq, ref, skip):
    oracle, manager, _, _ = mods
    m, descs = seq
    sel = ref(skip)[0]
    g = manager.STDescManager()
    res = g.loop_frames(m.xyz, m.label, skip_near=skip)
    assert g.current_frame_id_ == N_SEQ and g.stats()["n_frames"] == N_SEQ
    assert np.array_equal(res.query_frame_id, np.arange(N_SEQ))
    _same_as_oracle(g, res, sel)
    # the query descriptors carry their own frame ids, and the table holds the descriptors the oracle built
    for q in (0, 137, N_SEQ - 1):
        d = g.result_query_descs(q)
        assert d.n == descs[q].n and np.all(d.frame == q) and np.array_equal(d.side, descs[q].side)
    # the entries the longest match lists name: the table is the frames' descriptors in insertion order
    q = max(range(N_SEQ), key=lambda i: len(sel[i]["db_entry"]))
    de = sel[q]["db_entry"]
    ent = g.fetch_entries(de)
    for name in ("side", "vertex", "frame", "node_id"):
        table = np.concatenate([getattr(d, name) for d in descs])
        assert np.array_equal(getattr(ent, name), table[de]), name
    assert len(de) > 0 and np.all(ent.frame.astype(np.int64) + skip < q)
    assert int(np.sum(res.n_cand > 0)) > N_SEQ // 4        # the trajectory revisits places: there are loops to find
    g.close()


def test_verify_and_search_loop_equal_the_reference(mods, seq, ref):
    oracle, manager, _, _ = mods
    m, descs = seq
    sample = VERIFY_SAMPLE
    _, ver, _ = ref(0)
    g = manager.STDescManager()
    res = g.loop_frames(m.xyz, m.label)
    g.verify()
    bc, bf, bs = g.search_loop()
    loops = 0
    for q in sorted(sample):
        cands, (k, f, s) = ver[q]
        score, rot, t = g.result_verify(q)
        for j, (o_s, o_t, o_rot) in enumerate(cands):
            assert score[j] == o_s, (q, j)
            if o_s >= 0:
                assert np.array_equal(t[j], o_t) and np.array_equal(rot[j], o_rot), (q, j)
        assert int(bf[q]) == f and float(bs[q]) == s, q
        if f >= 0:
            assert int(bc[q]) == k and f < q
            loops += 1
    assert loops > 0
    g.close()


def _chunked(manager, xyz, label, B, skip=0):
    """loop_frames called every B frames; per frame its candidates and match list"""
    g = manager.STDescManager()
    out = []
    for f0 in range(0, xyz.shape[0], B):
        res = g.loop_frames(xyz[f0:f0 + B], label[f0:f0 + B], skip_near=skip, batch=B)
        for q in range(xyz[f0:f0 + B].shape[0]):
            nc = int(res.n_cand[q])
            out.append((res.cand_frame[q, :nc].copy(), res.cand_votes[q, :nc].copy(), res.pair_off[q, :nc + 1].copy(),
                        *g.result_pairs(q, res)))
    g.close()
    return out


def test_chunking_composes_exactly(mods, seq):
    _, manager, _, _ = mods
    m, _ = seq
    F = 300
    xyz, label = m.xyz[:F], m.label[:F]
    ref = _chunked(manager, xyz, label, F, skip=3)
    for B in (1, 7, 64):
        got = _chunked(manager, xyz, label, B, skip=3)
        assert len(got) == F
        for q in range(F):
            assert all(np.array_equal(a, b) for a, b in zip(got[q], ref[q])), (B, q)
    # the manager's own chunking (batch=) returns the same candidate tables in one BatchResult
    g = manager.STDescManager()
    res = g.loop_frames(xyz, label, skip_near=3, batch=64)
    for q in range(F):
        nc = int(res.n_cand[q])
        assert np.array_equal(res.cand_frame[q, :nc], ref[q][0]) and np.array_equal(res.pair_off[q, :nc + 1], ref[q][2])
    g.close()


@pytest.mark.parametrize("finalized", [False, True])
def test_session_on_a_prebuilt_map(mods, session, finalized):
    """session frame i sees the map and the session frames before it; with finalize() the session's frames are appended
    to the tail segment"""
    _, manager, _, _ = mods
    mp, ss, sel = session
    g = manager.STDescManager()
    g.add_frames(mp.xyz, mp.label)
    if finalized:
        g.finalize()
    f0 = 0
    if finalized:           # a first chunk small enough to stay in the tail segment (a tail is merged past an eighth of the map)
        f0 = 8
        first = g.loop_frames(ss.xyz[:f0], ss.label[:f0])
        assert g.stats()["tail_entries"] > 0
        _same_as_oracle(g, first, sel[:f0])
    res = g.loop_frames(ss.xyz[f0:], ss.label[f0:])
    assert np.array_equal(res.query_frame_id, N_MAP + np.arange(f0, N_MAP))
    _same_as_oracle(g, res, sel[f0:])
    assert int(np.sum(res.n_cand > 0)) > N_MAP // 2 and np.any(res.cand_frame[res.n_cand > 0, 0] < N_MAP)
    g.close()


def test_rough_list_stays_below_the_bound(mods, seq, ref):
    _, manager, _, _ = mods
    m, _ = seq
    skip = 20
    _, _, rgh = ref(skip)
    g = manager.STDescManager()
    g.loop_frames(m.xyz, m.label, skip_near=skip)
    for q in ROUGH_FRAMES:
        gr, orr = g.result_rough(q), rgh[q]
        for key in ("q_idx", "cell", "db_entry", "frame", "dis"):
            np.testing.assert_array_equal(gr[key], orr[key], err_msg="%s %d" % (key, q))
        assert np.all(gr["frame"].astype(np.int64) + skip < q)
    assert len(g.result_rough(N_SEQ - 1)["frame"]) > 0
    g.close()


def test_errors_and_the_plain_path_afterwards(mods, seq):
    _, manager, _, _lib = mods
    m, _ = seq
    L = _lib.lib()
    g = manager.STDescManager()
    x = np.ascontiguousarray(m.xyz[:4], dtype=np.float32)
    lab = np.ascontiguousarray(m.label[:4], dtype=np.uint32)
    off = np.arange(5, dtype=np.int64) * 200
    P = lambda a: a.ctypes.data
    assert L.sgtd_loop_frames(g._h, P(x), P(lab), P(off), 4, -1, 0) == -1
    assert L.sgtd_loop_frames(g._h, P(x), P(lab), P(off), 0, 0, 0) == -1
    assert L.sgtd_loop_frames(g._h, None, P(lab), P(off), 4, 0, 0) == -1
    with pytest.raises(_lib.SgtdError):
        g.loop_frames(x, lab, skip_near=-1)
    assert g.current_frame_id_ == 0 and g.stats()["n_entries"] == 0      # nothing was added
    # a view borrows its owner's table: it cannot add frames
    owner = manager.STDescManager()
    owner.add_frames(m.xyz[:50], m.label[:50])
    owner.finalize()
    view = manager.STDescManager()
    view.attach_table(owner)
    assert L.sgtd_loop_frames(view._h, P(x), P(lab), P(off), 4, 0, 0) == -7
    view.close()
    # after a loop batch a plain query batch on the same handle equals one on a fresh handle with the same table
    g.loop_frames(m.xyz[:200], m.label[:200])
    fresh = manager.STDescManager()
    fresh.add_frames(m.xyz[:200], m.label[:200])
    qx, ql = m.xyz[200:232], m.label[200:232]
    a, b = g.query_frames(qx, ql), fresh.query_frames(qx, ql)
    for k in ("n_cand", "cand_frame", "cand_votes", "pair_off"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for q in (0, 31):
        assert all(np.array_equal(u, v) for u, v in zip(g.result_pairs(q, a), fresh.result_pairs(q, b)))
    # ... and a plain query over the table's own frames still only excludes the query's frame id (current_frame_id_)
    assert int(np.sum(a.n_cand > 0)) > 0
    for h in (g, fresh, owner):
        h.close()


def test_short_frames_and_first_frames_have_no_loop(mods, seq):
    _, manager, _, _ = mods
    m, _ = seq
    n_kp = [200, 200, 5, 200, 2, 200, 200, 0, 200, 200]
    xyz = np.concatenate([m.xyz[i, :n] for i, n in enumerate(n_kp)]).astype(np.float32)
    label = np.concatenate([m.label[i, :n] for i, n in enumerate(n_kp)]).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(n_kp)]).astype(np.int64)
    g = manager.STDescManager()
    res = g.loop_frames(xyz, label, kp_off=off)
    assert g.current_frame_id_ == len(n_kp)
    g.verify()
    _, bf, bs = g.search_loop()
    for q, n in enumerate(n_kp):
        if n < g.config_setting_["descriptor_near_num"] or q == 0:
            assert int(res.n_cand[q]) == 0 and int(bf[q]) == -1 and float(bs[q]) == 0.0, q
    assert np.all(bf < np.arange(len(n_kp)))
    g.close()


def test_multi_device_handle_is_refused(mods, seq):
    _, manager, _, _lib = mods
    g = manager.STDescManager(devices=[0, 0])
    m, _ = seq
    with pytest.raises(_lib.SgtdError, match="multi-device") as ei:
        g.loop_frames(m.xyz[:4], m.label[:4])
    assert ei.value.status == -6
    g.close()
