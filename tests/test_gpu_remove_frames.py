"""sgtd_remove_frames / STDescManager.remove_frames: after removing the frame set S a handle must answer every query and
inspection call as a handle whose caller never added S.  The yardstick is the oracle holding the survivors (added frame by
frame, in the original order, with the original frame ids, then set_current_frame_id), compared bit for bit: candidates,
full vote arrays, ordered match lists and their entries, the table dump, rough lists, candidate_verify and SearchLoop."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = 200
# (frames 25 m apart on the closed trajectory, as the loop-frames tests: it still revisits every place, and the oracle's
# host-side selects stay fast)
SPACING = 25.0
NQ = 8
DESC_FIELDS = ("side", "angle", "center", "vertex", "label", "frame", "node_id")


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from sgtd_amd import _lib, manager, synth
    oracle.build_library()
    return oracle, manager, synth, _lib


@pytest.fixture(scope="module")
def world(mods):
    """a map of F frames, its per-frame oracle descriptors (frame ids 0..F-1) and a query batch over it"""
    oracle, _, synth, _ = mods
    m = synth.make_map(F, 200, stream=307, spacing=SPACING)
    qs = synth.make_queries(m, NQ, stream=308)
    return m, _oracle_descs(oracle, m.xyz, m.label, 0), qs


def _oracle_descs(oracle, xyz, label, first):
    o = oracle.OracleManager()
    out = []
    for i in range(xyz.shape[0]):
        o.set_current_frame_id(first + i)
        out.append(o.build(xyz[i], label[i]))
    return out


def _to_manager_descs(manager, d):
    g = manager.Descs(d.n)
    for f in DESC_FIELDS:
        getattr(g, f)[...] = getattr(d, f)
    return g


def _oracle_with(oracle, descs, frames, current):
    """the oracle a caller gets who added only `frames` (in this order, original ids) and sits at frame `current`"""
    o = oracle.OracleManager()
    for f in frames:
        o.add(descs[f])
    o.set_current_frame_id(current)
    return o


def _survivors(removed, n=F):
    gone = set(int(f) for f in removed)
    return [f for f in range(n) if f not in gone]


def _entries_of(descs, frames):
    return sum(descs[f].n for f in frames)


def _same_entries(g, o, db_entry):
    if len(db_entry) == 0:
        return
    a, b = g.fetch_entries(db_entry), o.fetch_entries(db_entry)
    for f in DESC_FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f


def _same_dump(g, o):
    gk, goff, gid = g.table_dump()
    ok, ooff, oid = o.table_dump()
    assert np.array_equal(gk, ok) and np.array_equal(goff, ooff) and np.array_equal(gid, oid)


def _compare(g, o, qs, verify=True, rough=(0, 5), icp=0.4):
    """one query batch through the handle and the same queries through the oracle, compared bit for bit"""
    res = g.query_frames(qs.xyz, qs.label)
    if verify:
        g.verify()
        bc, bf, bs = g.search_loop(icp)
    n_lists = 0
    for q in range(qs.xyz.shape[0]):
        o.build(qs.xyz[q], qs.label[q], export=False)
        r = o.select()
        nc = len(r["cand_frame"])
        assert int(res.n_cand[q]) == nc, q
        assert np.array_equal(res.cand_frame[q, :nc], r["cand_frame"]), q
        assert np.array_equal(res.cand_votes[q, :nc], r["cand_votes"]), q
        assert np.array_equal(res.pair_off[q, :nc + 1], r["cand_off"]), q
        qi, de = g.result_pairs(q, res)
        assert np.array_equal(qi, r["q_idx"]) and np.array_equal(de, r["db_entry"]), q
        _same_entries(g, o, de)
        n_lists += len(de)
        lo, v = g.result_votes(q)
        ov = o.votes()
        assert np.array_equal(v.astype(np.float64), ov[lo:lo + len(v)]), q
        assert ov[:lo].sum() == 0 and ov[lo + len(v):].sum() == 0, q
        if verify:
            score, rot, t = g.result_verify(q)
            best_s, best_k = 0.0, -1
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
    for q in rough:
        o.build(qs.xyz[q], qs.label[q], export=False)
        o.select()
        gr, orr = g.result_rough(q), o.rough_matches()
        for k in ("q_idx", "cell", "db_entry", "frame", "dis"):
            assert np.array_equal(gr[k], orr[k]), (k, q)
    return res, n_lists


def _check_state(g, descs, survivors, current):
    st = g.stats()
    assert g.current_frame_id_ == current
    assert st["n_entries"] == _entries_of(descs, survivors)
    assert st["n_frames"] == len(survivors)
    # the cold store is the survivors' descriptors in insertion order
    if survivors:
        ent = g.fetch_entries(np.arange(st["n_entries"]))
        for f in DESC_FIELDS:
            assert np.array_equal(getattr(ent, f), np.concatenate([getattr(descs[s], f) for s in survivors])), f


REMOVALS = {
    "block": list(range(40, 104)),
    "scattered": sorted(int(x) for x in np.random.default_rng(11).choice(F, 37, replace=False)),
    # duplicates, ids beyond the table, ids far beyond any frame
    "dups_absent": [3, 3, 77, 77, 77, 150, F, F + 5, 19999, 2 ** 31, 2 ** 32 - 1, 151, 150],
}


@pytest.mark.parametrize("case", sorted(REMOVALS))
def test_removal_equals_never_added(mods, world, case):
    oracle, manager, _, _ = mods
    m, descs, qs = world
    removed = REMOVALS[case]
    survivors = _survivors(removed)
    g = manager.STDescManager()
    g.add_frames(m.xyz, m.label)
    g.query_frames(qs.xyz[:1], qs.label[:1])      # a finalized single-segment table with a batch behind it
    assert g.stats()["tail_entries"] == 0
    n = g.remove_frames(removed)
    assert n == _entries_of(descs, set(range(F)) - set(survivors))
    _check_state(g, descs, survivors, F)
    o = _oracle_with(oracle, descs, survivors, F)
    _same_dump(g, o)
    _, n_lists = _compare(g, o, qs)
    assert n_lists > 0
    # the removed frames receive no votes and name no candidate
    res = g.query_frames(qs.xyz, qs.label)
    assert not np.isin(res.cand_frame[res.cand_frame >= 0], removed).any()
    # removing them again, nothing or unknown ids changes nothing
    assert g.remove_frames(removed) == 0 and g.remove_frames([]) == 0 and g.remove_frames([F + 1]) == 0
    _check_state(g, descs, survivors, F)
    g.close()


def test_removal_from_main_segment_and_tail(mods, world):
    oracle, manager, _, _ = mods
    m, descs, qs = world
    g = manager.STDescManager()
    g.add_frames(m.xyz[:170], m.label[:170])
    g.finalize()
    g.add_frames(m.xyz[170:], m.label[170:])
    g.finalize()
    assert g.stats()["tail_entries"] > 0
    removed = list(range(20, 30)) + [100, 171, 172, 185] + list(range(195, F))
    survivors = _survivors(removed)
    g.remove_frames(removed)
    _check_state(g, descs, survivors, F)
    o = _oracle_with(oracle, descs, survivors, F)
    _compare(g, o, qs)
    assert g.stats()["tail_entries"] == 0            # the next finalize built one segment over the whole table
    _same_dump(g, o)
    g.close()


def test_add_frames_and_loop_frames_after_removal(mods, world):
    oracle, manager, synth, _ = mods
    m, descs, qs = world
    removed = list(range(60, 120))
    survivors = _survivors(removed)
    g = manager.STDescManager()
    g.add_frames(m.xyz[:150], m.label[:150])
    g.finalize()
    g.remove_frames(removed)
    # add_frames continues at the unchanged frame counter: the removed ids are not reused
    g.add_frames(m.xyz[150:], m.label[150:])
    o = _oracle_with(oracle, descs, [f for f in survivors if f < 150], 150)
    for f in range(150, F):
        o.add(descs[f])
    assert g.current_frame_id_ == o.current_frame_id == F
    _compare(g, o, qs, rough=(1,))
    _same_dump(g, o)
    # a session through loop_frames on top: frame i sees the survivors and the session frames before it
    ss = synth.make_queries(m, 40, stream=309, frames=np.arange(40) * 5)
    sdescs = _oracle_descs(oracle, ss.xyz, ss.label, F)
    g.remove_frames([0, 1, 2, 199])
    o = _oracle_with(oracle, descs, [f for f in survivors if f not in (0, 1, 2, 199)], F)
    res = g.loop_frames(ss.xyz, ss.label)
    for i, d in enumerate(sdescs):
        r = o.select(d)
        nc = len(r["cand_frame"])
        assert int(res.n_cand[i]) == nc and np.array_equal(res.cand_frame[i, :nc], r["cand_frame"]), i
        assert np.array_equal(res.cand_votes[i, :nc], r["cand_votes"]) and np.array_equal(res.pair_off[i, :nc + 1], r["cand_off"]), i
        o.add(d)
    assert int(np.sum(res.n_cand > 0)) > 0
    qi, de = g.result_pairs(39, res)
    assert np.array_equal(de, r["db_entry"]) and np.array_equal(qi, r["q_idx"])
    g.close()


def test_save_and_load_after_removal(mods, world, tmp_path):
    oracle, manager, _, _ = mods
    m, descs, qs = world
    removed = list(range(0, 64)) + [100, 130, 131]
    survivors = _survivors(removed)
    g = manager.STDescManager()
    g.add_frames(m.xyz, m.label)
    g.finalize()
    g.remove_frames(removed)
    g.save_table(tmp_path / "removed.tab")
    # the file a handle writes whose caller added only the survivors, one AddSTDescs per frame, at the same frame counter
    fresh = manager.STDescManager(first_frame_id=F - len(survivors))
    for f in survivors:
        fresh.AddSTDescs(_to_manager_descs(manager, descs[f]))
    assert fresh.current_frame_id_ == F
    fresh.save_table(tmp_path / "fresh.tab")
    with open(tmp_path / "removed.tab", "rb") as a, open(tmp_path / "fresh.tab", "rb") as b:
        assert a.read() == b.read()
    loaded = manager.STDescManager()
    loaded.load_table(tmp_path / "removed.tab")
    _check_state(loaded, descs, survivors, F)
    o = _oracle_with(oracle, descs, survivors, F)
    _compare(loaded, o, qs, rough=())
    _same_dump(loaded, o)
    for h in (g, fresh, loaded):
        h.close()


def test_remove_every_frame_then_add_again(mods, world):
    oracle, manager, _, _ = mods
    m, descs, qs = world
    g = manager.STDescManager()
    g.add_frames(m.xyz[:100], m.label[:100])
    g.finalize()
    assert g.remove_frames(np.arange(100)) == _entries_of(descs, range(100))
    st = g.stats()
    assert st["n_entries"] == 0 and st["n_frames"] == 0 and st["n_buckets"] == 0 and g.current_frame_id_ == 100
    keys, off, ids = g.table_dump()
    assert keys.shape == (0, 4) and list(off) == [0] and ids.size == 0
    res = g.query_frames(qs.xyz, qs.label)
    assert np.all(res.n_cand == 0)
    # an empty table takes frames again, from the unchanged frame counter on
    g.add_frames(m.xyz[100:], m.label[100:])
    o = _oracle_with(oracle, descs, range(100, F), F)
    _check_state(g, descs, list(range(100, F)), F)
    _compare(g, o, qs, rough=(2,))
    _same_dump(g, o)
    g.close()


def test_views_after_removal(mods, world):
    oracle, manager, _, _lib = mods
    m, descs, qs = world
    owner = manager.STDescManager()
    owner.add_frames(m.xyz, m.label)
    owner.finalize()
    view = manager.STDescManager()
    view.attach_table(owner)
    view.query_frames(qs.xyz, qs.label)
    # a call that removes nothing changes nothing: the view stays attached
    assert owner.remove_frames([F + 3]) == 0
    view.query_frames(qs.xyz, qs.label)
    # a view cannot remove frames
    with pytest.raises(_lib.SgtdError) as ei:
        view.remove_frames([1])
    assert ei.value.status == -7
    removed = list(range(10, 50))
    owner.remove_frames(removed)
    with pytest.raises(_lib.SgtdError) as ei:
        view.query_frames(qs.xyz, qs.label)
    assert ei.value.status == -7
    view.attach_table(owner)
    o = _oracle_with(oracle, descs, _survivors(removed), F)
    _compare(view, o, qs, rough=())
    view.close()
    owner.close()


def test_multi_device_handle(mods, world):
    _, manager, _, _ = mods
    m, descs, qs = world
    removed = list(range(30, 70)) + [129, 130, 131, 192]      # across the 64-frame shard blocks
    single = manager.STDescManager()
    multi = manager.STDescManager(devices=[0, 0, 0])
    for h in (single, multi):
        h.add_frames(m.xyz, m.label)
        h.finalize()
    assert multi.remove_frames(removed) == single.remove_frames(removed) == _entries_of(descs, removed)
    assert multi.current_frame_id_ == single.current_frame_id_ == F
    assert multi.stats()["n_entries"] == single.stats()["n_entries"]
    assert multi.stats()["n_frames"] == single.stats()["n_frames"] == F - len(removed)
    a, b = single.query_frames(qs.xyz, qs.label), multi.query_frames(qs.xyz, qs.label)
    for k in ("n_cand", "cand_frame", "cand_votes", "pair_off"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    n_lists = 0
    for q in range(NQ):
        qa, da = single.result_pairs(q, a)
        qb, db = multi.result_pairs(q, b)
        assert np.array_equal(qa, qb)
        assert np.all((db >> 40) < 3)                              # group entry ids: shard << 40 | local index
        if len(da):
            ea, eb = single.fetch_entries(da), multi.fetch_entries(db)
            for f in DESC_FIELDS:
                assert np.array_equal(getattr(ea, f), getattr(eb, f)), f
        n_lists += len(da)
        la, va = single.result_votes(q)
        lb, vb = multi.result_votes(q)
        full_a, full_b = np.zeros(F, np.int64), np.zeros(F, np.int64)
        full_a[la:la + len(va)] = va
        full_b[lb:lb + len(vb)] = vb
        assert np.array_equal(full_a, full_b), q
    assert n_lists > 0
    multi.close()
    single.close()


def test_many_tiles_against_a_rebuilt_table(mods):
    """F = 10 000 frames (tens of thousands of compaction tiles): remove 1 000 frames — 64-frame blocks and scattered ids —
    and compare with a handle built by sgtd_add of the survivors' fetched descriptors, one call per frame"""
    _, manager, synth, _lib = mods
    big = 10000
    m = synth.make_map(big, 200, stream=1)
    rng = np.random.default_rng(12)
    blocks = np.concatenate([np.arange(b * 64, b * 64 + 64) for b in rng.choice(big // 64, 10, replace=False)])
    rest = np.setdiff1d(np.arange(big), blocks)
    removed = np.sort(np.concatenate([blocks, rng.choice(rest, 1000 - len(blocks), replace=False)]))
    assert len(np.unique(removed)) == 1000
    g = manager.STDescManager()
    g.add_frames(m.xyz, m.label)
    g.finalize()
    before = g.stats()["n_entries"]
    n = g.remove_frames(removed)
    E = g.stats()["n_entries"]
    assert n > 0 and E == before - n and g.stats()["n_frames"] == big - 1000
    # every survivor's entries, frame by frame, from the compacted store into a fresh handle
    fr = np.zeros(E, np.uint32)
    soa = _lib.DescSoa()
    soa.frame = fr.ctypes.data
    idx = np.arange(E, dtype=np.int64)
    assert g._L.sgtd_fetch_entries(g._h, idx.ctypes.data, E, ctypes.byref(soa)) == 0
    cut = np.flatnonzero(np.diff(fr.astype(np.int64))) + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [E]])
    survivors = fr[starts]
    assert np.array_equal(survivors, np.setdiff1d(np.arange(big), removed))
    fresh = manager.STDescManager(first_frame_id=big - len(survivors))
    for a, b in zip(starts, ends):
        fresh.AddSTDescs(g.fetch_entries(np.arange(a, b)))
    assert fresh.current_frame_id_ == g.current_frame_id_ == big
    ka, oa, ia = g.table_dump()
    kb, ob, ib = fresh.table_dump()
    assert np.array_equal(ka, kb) and np.array_equal(oa, ob) and np.array_equal(ia, ib)
    qs = synth.make_queries(m, 2048, stream=2)
    ra, rb = g.query_frames(qs.xyz, qs.label), fresh.query_frames(qs.xyz, qs.label)
    for k in ("n_cand", "cand_frame", "cand_votes", "pair_off"):
        assert np.array_equal(getattr(ra, k), getattr(rb, k)), k
    assert int(np.sum(ra.n_cand > 0)) > 1000
    assert not np.isin(ra.cand_frame[ra.cand_frame >= 0], removed).any()
    fresh.close()
    g.close()
