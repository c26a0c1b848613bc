"""The passes over the match records (STDesc.cpp:404-453: votes, top-k, match lists) at their edges in every form, against
the oracle bit for bit: the full vote vector, M (stats()["last_M"]), the candidates, their votes, pair_off and every match
list's (q_idx, db_entry) in order; every form asserts stats()["select_form"], so a passing test proves which kernels ran.
Workloads: tests/_record_edges.py (tests/test_record_edges.py shows without a GPU that they reach their edges).

  descriptor cases   candidate_selector in the automatic mode (one query: the block form); SGTD_SELECT_MODE=2
                     (votes_topk_kernel + pairs_query_kernel<true>, select_form 2; the wide span builds: votes_kernel<false>
                     — one query is too small a batch for the tiled votes_query_kernel —, topk_kernel, cand_prefix_kernel
                     and the candidates' hash, select_form 1); SGTD_SELECT_MODE=1 (one query takes the block form anyway: the
                     same kernels as the automatic mode, on the wide spans block_count_kernel<false, .>; kept because the
                     knob must not change the answer); SGTD_WIDE_PAIRS=1; SGTD_BLOCK_CHUNK 32 and 64;
                     search_frame(lists_only=True); a three-shard handle on one GPU; set_deferred_lists + finish_lists(keep)
                     with the masks all, none, bit 0, the highest candidate, alternating; a frame filter that allows every
                     frame and one that drops the first and the last candidate's frames
  keypoint batches   query_frames at one query per CU and one below, SGTD_SELECT_MODE 1 and 2, maps stamped over more than
                     36 Ki and 120 000 frame ids (the tiled votes_query_kernel, candidates on both sides of its first tile's
                     edge), loop_frames with skip_near 0 and 2

stats() reports select_form and nothing about the compact words' width or the block chunk: the SGTD_WIDE_PAIRS and
SGTD_BLOCK_CHUNK forms prove the answer under the knob, not that the knob took effect (the launch code reads the first per
handle and the second per call).

None of these knobs is read once per process (SGTD_SELECT_MODE and SGTD_WIDE_PAIRS per handle, SGTD_BLOCK_CHUNK per call):
every form runs in the test's own process.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _record_edges as rec  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = [f.__name__ for f in rec.FAMILIES]
FORMS = {
    "auto": {}, "mode2": {"SGTD_SELECT_MODE": "2"}, "mode1": {"SGTD_SELECT_MODE": "1"}, "wide_pairs": {"SGTD_WIDE_PAIRS": "1"},
    "chunk32": {"SGTD_BLOCK_CHUNK": "32"}, "chunk64": {"SGTD_BLOCK_CHUNK": "64"}, "frame": {}, "multi": {},
    "deferred": {"SGTD_SELECT_MODE": "2"}, "filter": {}, "filter_mode2": {"SGTD_SELECT_MODE": "2"},
}
FIELDS = ("side", "label", "frame")

_CASES, _EXPECT = {}, {}


def family_cases(family):
    if family not in _CASES:
        _CASES[family] = rec.cases((family,))
    return _CASES[family]


def _oracle_answers(c, entries=None):
    """the oracle's answer per query of case c (entries: a mask over the table entries: a table of those alone)"""
    from oracle import oracle
    o = oracle.OracleManager(**c.config())
    if entries is None:
        c.load(o, oracle)
    else:
        side, label, frame = c.entry_arrays()
        d = c._descs(oracle, side[entries], label[entries], frame[entries])
        o.add(d)
    out = []
    for k in range(len(c.queries)):
        sel = o.select(c.query_descs(oracle, k))
        sel.update(votes=o.votes(), M=o.counters()["M"])
        ent = o.fetch_entries(sel["db_entry"])
        sel["entries"] = {f: getattr(ent, f).copy() for f in FIELDS}
        out.append(sel)
    return out


def expected(c):
    if c.name not in _EXPECT:
        _EXPECT[c.name] = _oracle_answers(c)
    return _EXPECT[c.name]


def mode2_form(c):
    """select_form of SGTD_SELECT_MODE=2 by the launch code: the lists by one workgroup per query unless the image word
    cannot hold the rank (64 candidates and 17 rank bits), votes and top-k fused while the span's histogram fits LDS"""
    if c.cn == rec.SGTD_MAX_CAND and c.info.get("bits") == 17:
        return 0
    return 1 if c.max_frame_n > 100000 else 2


def _check_votes(g, exp, tag):
    lo, v = g.result_votes(0)
    ov = exp["votes"]
    n = min(len(v), len(ov) - lo)
    np.testing.assert_array_equal(v[:n].astype(np.float64), ov[lo:lo + n], err_msg=tag)
    assert v[n:].sum() == 0 and ov[:lo].sum() == 0 and ov[lo + n:].sum() == 0, tag
    assert g.stats()["last_M"] == exp["M"], tag


def _check_set(g, exp, tag, multi=False, emap=None):
    res = g.results()
    nc = int(res.n_cand[0])
    assert nc == len(exp["cand_frame"]), tag
    np.testing.assert_array_equal(res.cand_frame[0, :nc], exp["cand_frame"], err_msg=tag)
    np.testing.assert_array_equal(res.cand_votes[0, :nc], exp["cand_votes"], err_msg=tag)
    np.testing.assert_array_equal(res.pair_off[0, :nc + 1], exp["cand_off"], err_msg=tag)
    assert np.all(res.pair_off[0, nc:] == exp["cand_off"][-1]), tag
    qi, de = g.result_pairs(0, res)
    np.testing.assert_array_equal(qi, exp["q_idx"], err_msg=tag)
    if multi:       # (the entry ids are the shards' own: the same entries)
        got = g.fetch_entries(de)
        for f in FIELDS:
            np.testing.assert_array_equal(getattr(got, f), exp["entries"][f], err_msg=tag + " " + f)
    else:
        np.testing.assert_array_equal(de if emap is None else emap[de], exp["db_entry"], err_msg=tag)
    _check_votes(g, exp, tag)


def _check_frame(g, mod, c, k, exp, tag):
    """search_frame(lists_only=True): the candidates and every pair of every list with its table entry"""
    cap = max(int(exp["cand_off"][-1]), 1)
    out = g.search_frame(c.query_descs(mod, k), capacity=cap, lists_only=True)
    assert out["status"] == 0, tag
    nc = len(exp["cand_frame"])
    assert out["n_cand"] == nc, tag
    np.testing.assert_array_equal(out["cand_frame"][:nc], exp["cand_frame"], err_msg=tag)
    np.testing.assert_array_equal(out["cand_votes"][:nc], exp["cand_votes"], err_msg=tag)
    np.testing.assert_array_equal(out["pair_off"][:nc + 1], exp["cand_off"], err_msg=tag)
    np.testing.assert_array_equal(out["inlier_q_idx"], exp["q_idx"], err_msg=tag)
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(out["entries"], f), exp["entries"][f], err_msg=tag + " " + f)
    _check_votes(g, exp, tag)


def _keep_tensor(mask):
    import torch
    return torch.tensor([mask - (1 << 64) if mask >= (1 << 63) else mask], dtype=torch.int64, device="cuda")


def _handle(manager, c, form):
    g = manager.STDescManager(devices=[0, 0, 0], **c.config()) if form == "multi" else manager.STDescManager(**c.config())
    if c.tail_at is not None:
        c.load(g, manager, 0, c.tail_at)
        g.candidate_selector(c.query_descs(manager, 0))            # (the table is built: what follows goes to a tail)
        c.load(g, manager, c.tail_at, None)
    else:
        c.load(g, manager)
    return g


def run_form(family, form):
    """every query of every case of the family through one form; returns the number of (case, query) pairs checked"""
    from sgtd_amd import manager
    n = 0
    for c in family_cases(family):
        if form == "multi" and not c.stamped:       # (a multi-device table takes one frame per call, ids 0, 1, 2, ...)
            continue
        want_form = mode2_form(c) if form in ("mode2", "deferred", "filter_mode2") else 0
        if form == "deferred" and want_form == 0:   # (the block form has written every list already)
            continue
        exp = expected(c)
        g = _handle(manager, c, form)
        for k in range(len(c.queries)):
            tag = "%s/%s/query%d" % (c.name, form, k)
            if form == "frame":
                _check_frame(g, manager, c, k, exp[k], tag)
            elif form == "deferred":
                g.set_deferred_lists(True)
                g.query_descs(c.query_descs(manager, k))
                for name, mask in rec.keep_masks(len(exp[k]["cand_frame"])).items():
                    g.finish_lists(_keep_tensor(mask))
                    _check_set(g, rec.masked(exp[k], mask), tag + "/" + name)
                g.finish_lists(None)
                _check_set(g, exp[k], tag + "/unmasked")
                g.set_deferred_lists(False)
            elif form in ("filter", "filter_mode2"):
                frames = np.unique(np.asarray(c.eframe))
                g.candidate_selector(c.query_descs(manager, k))
                _check_set(g, exp[k], tag + "/unfiltered")
                g.set_frame_filter(frames)
                g.candidate_selector(c.query_descs(manager, k))
                _check_set(g, exp[k], tag + "/all")
                g.set_frame_filter(None)
            else:
                g.candidate_selector(c.query_descs(manager, k))
                _check_set(g, exp[k], tag, multi=form == "multi")
            assert g.stats()["select_form"] == want_form, tag
            if c.tail_at is not None and k == 0 and form != "multi":      # (a sharded handle spreads the appended frames)
                assert g.stats()["tail_entries"] > 0, tag
            n += 1
        if form in ("filter", "filter_mode2") and len(exp[0]["cand_frame"]) >= 3:
            # the first and the last candidate's frames dropped: the answer of a handle that holds only the allowed frames
            # (tests/test_gpu_frame_filter.py), its entry ids mapped to the full table's
            drop = [int(exp[0]["cand_frame"][0]), int(exp[0]["cand_frame"][-1])]
            f = np.asarray(c.eframe)
            held = ~np.isin(f, drop)
            want = _oracle_answers(c, held)[0]
            assert not set(drop) & set(want["cand_frame"].tolist())
            emap = np.cumsum(held) - 1
            g.set_frame_filter(np.unique(f[held]))
            g.candidate_selector(c.query_descs(manager, 0))
            _check_set(g, want, c.name + "/" + form + "/dropped", emap=emap)
            assert g.stats()["select_form"] == want_form
            g.set_frame_filter(None)
            n += 1
        g.close()
    return n


# (the span family is caller-stamped frame ids from 1000 on: nothing a multi-device handle takes)
@pytest.mark.parametrize("form,family", [(fo, fa) for fo in FORMS for fa in FAMILIES if (fo, fa) != ("multi", "span")])
def test_every_form_equals_the_oracle(family, form, monkeypatch):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    assert run_form(family, form) >= 1


# ---- keypoint batches ----------------------------------------------------------------------------------------------
def _n_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _check_batch(g, res, sels, which, pairs_of):
    """query q of the batch is the oracle's select sels[which[q]]; the lists of the queries in pairs_of"""
    for q, w in enumerate(which):
        r = sels[w]
        nc = len(r["cand_frame"])
        assert int(res.n_cand[q]) == nc, q
        np.testing.assert_array_equal(res.cand_frame[q, :nc], r["cand_frame"], err_msg=str(q))
        np.testing.assert_array_equal(res.cand_votes[q, :nc], r["cand_votes"], err_msg=str(q))
        np.testing.assert_array_equal(res.pair_off[q, :nc + 1], r["cand_off"], err_msg=str(q))
    for q in pairs_of:
        r = sels[which[q]]
        qi, de = g.result_pairs(q, res)
        np.testing.assert_array_equal(qi, r["q_idx"], err_msg=str(q))
        np.testing.assert_array_equal(de, r["db_entry"], err_msg=str(q))
        lo, v = g.result_votes(q)
        ov = r["votes"]
        n = min(len(v), len(ov) - lo)
        np.testing.assert_array_equal(v[:n].astype(np.float64), ov[lo:lo + n], err_msg=str(q))
        assert ov[:lo].sum() == 0 and ov[lo + n:].sum() == 0


def _tiled_batch(off, xyz, label, n):
    """the distinct query frames (ragged: off) repeated to a batch of n frames -> (xyz, label, kp_off, which)"""
    nd = len(off) - 1
    which = np.arange(n) % nd
    xs = [xyz[off[w]:off[w + 1]] for w in which]
    ls = [label[off[w]:off[w + 1]] for w in which]
    kp = np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    return (np.ascontiguousarray(np.concatenate(xs), np.float32), np.ascontiguousarray(np.concatenate(ls), np.uint32), kp, which)


SPREAD_LO = 11


def _spread_ids(name, n):
    """ascending caller-stamped frame ids from SPREAD_LO in steps of 1300 / 4200, but for two neighbouring frames moved
    onto local frames VOTES_TILE_FRAMES - 1 and VOTES_TILE_FRAMES: the last frame of votes_query_kernel's first tile and
    the first of its second"""
    stride = {"spread36k": 1300, "spread120k": 4200}[name]
    ids = SPREAD_LO + np.arange(n) * stride
    k = int(np.searchsorted(ids, SPREAD_LO + rec.VOTES_TILE_FRAMES)) - 1
    ids[k - 1:k + 1] = SPREAD_LO + rec.VOTES_TILE_FRAMES - 1, SPREAD_LO + rec.VOTES_TILE_FRAMES
    assert np.all(np.diff(ids) > 0)
    return ids


def _kp_world(name):
    """(map loader, distinct queries (xyz, label, off), the oracle's selects with votes, config) of a keypoint workload"""
    if name in _EXPECT:
        return _EXPECT[name]
    from oracle import oracle
    from sgtd_amd import synth
    cfg = {}
    if name == "dup_frames":
        mx, ml, group, qx, ql = rec.dup_frames(synth)
        m_off = None
        q = (qx.reshape(-1, 3), ql.reshape(-1), np.arange(qx.shape[0] + 1, dtype=np.int64) * qx.shape[1])
    elif name == "tiny":
        (mx, ml, m_off), q = rec.tiny()
        cfg = dict(rec.TINY_CONFIG)
    else:       # ragged, spread36k, spread120k
        m = synth.make_map(30, 700 if name == "ragged" else 150, stream=21)
        mx, ml, m_off = m.xyz, m.label, None
        qs = synth.make_queries(m, 6 if name == "ragged" else 5, stream=21)
        sizes = [0, 1, 3, 25, 200, 700] if name == "ragged" else [150] * 5
        q = (np.concatenate([qs.xyz[i, :n] for i, n in enumerate(sizes)]), np.concatenate([qs.label[i, :n] for i, n in enumerate(sizes)]),
             np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
        if name.startswith("spread"):
            cfg = dict(max_frame_n=200000)
    stride = {"spread36k": 1300, "spread120k": 4200}.get(name)
    ids = _spread_ids(name, mx.shape[0]) if stride else None
    o = oracle.OracleManager(**cfg)
    n_map = len(m_off) - 1 if m_off is not None else mx.shape[0]
    for f in range(n_map):
        a, b = (m_off[f], m_off[f + 1]) if m_off is not None else (0, 0)
        fx, fl = (mx[a:b], ml[a:b]) if m_off is not None else (mx[f], ml[f])
        if stride:
            d = o.build(fx, fl)
            d.frame[:] = ids[f]
            o.add(d)
        else:
            o.build(fx, fl, export=False)
            o.add_last()
    sels, counts = [], []
    qx, ql, off = q
    for i in range(len(off) - 1):
        counts.append(o.build(qx[off[i]:off[i + 1]], ql[off[i]:off[i + 1]], export=False))
        r = o.select()
        r["votes"] = o.votes()
        sels.append(r)
    _EXPECT[name] = (mx, ml, m_off, ids, q, sels, counts, cfg)
    return _EXPECT[name]


def _kp_handle(manager, name):
    mx, ml, m_off, ids, q, sels, counts, cfg = _kp_world(name)
    g = manager.STDescManager(**cfg)
    if ids is not None:
        for f in range(mx.shape[0]):
            d = g.BuildSingleScanSTD(mx[f], ml[f])
            d.frame[:] = ids[f]
            g.AddSTDescs(d)
    else:
        g.add_frames(mx, ml, m_off)
    return g


KP_FORMS = {"at_cus": ({}, 0, 2), "below_cus": ({}, -1, 0), "mode1": ({"SGTD_SELECT_MODE": "1"}, 0, 0), "mode2": ({"SGTD_SELECT_MODE": "2"}, -1, 2)}


@pytest.mark.parametrize("name", ["dup_frames", "tiny", "ragged"])
@pytest.mark.parametrize("form", list(KP_FORMS))
def test_query_frames_forms_equal_the_oracle(name, form, monkeypatch):
    from sgtd_amd import manager
    env, dn, want_form = KP_FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mx, ml, m_off, ids, q, sels, counts, cfg = _kp_world(name)
    if name == "dup_frames":       # exact ties across frames: 1030 frames tied at the top, groups around the cut of 50
        top = sels[0]["votes"].max()
        assert int((sels[0]["votes"] == top).sum()) == rec.SGTD_TOPK_POOL + 6 and top >= 5
        assert [int((s["votes"] == s["votes"].max()).sum()) for s in sels[1:4]] == [49, 50, 51]
    if name == "tiny":             # the best frame of a query at 4, 5 and 6 votes, most queries without a candidate
        best = [int(s["votes"].max()) for s in sels]
        assert {4, 5, 6} <= set(best) and sum(len(s["cand_frame"]) == 0 for s in sels) >= 10
        assert all(s["votes"].max() > 0 for s in sels) and sum(len(s["cand_frame"]) > 0 for s in sels) >= 2
    if name == "ragged":           # empty queries beside one of one super-block and two of more
        assert counts[0] == 0 and 0 < counts[3] <= rec.PQ_DESCS < counts[4] < counts[5]
    nq = _n_cus() + dn
    g = _kp_handle(manager, name)
    bx, bl, kp, which = _tiled_batch(q[2], q[0], q[1], nq)
    res = g.query_frames(bx, bl, kp)
    assert g.stats()["select_form"] == want_form
    nd = len(q[2]) - 1
    _check_batch(g, res, sels, which, list(range(nd)) + list(range(nq - nd, nq)))
    g.close()


@pytest.mark.parametrize("name", ["spread36k", "spread120k"])
@pytest.mark.parametrize("mode", ["auto", "2"])
def test_spread_maps_take_the_tiled_votes(name, mode, monkeypatch):
    """a batch with nq * n_tiles >= n_cus / 4 below one query per CU: votes_query_kernel in tiles of 36 Ki frames, then
    topk_kernel and the block passes (select_form 0); SGTD_SELECT_MODE=2: the same votes and pairs_query_kernel (1)"""
    from sgtd_amd import manager
    if mode != "auto":
        monkeypatch.setenv("SGTD_SELECT_MODE", mode)
    mx, ml, m_off, ids, q, sels, counts, cfg = _kp_world(name)
    span = int(ids[-1] - ids[0]) + 1
    edge = [SPREAD_LO + rec.VOTES_TILE_FRAMES - 1, SPREAD_LO + rec.VOTES_TILE_FRAMES]
    assert all(set(edge) <= set(s["cand_frame"].tolist()) for s in sels)       # candidates on both sides of the tile edge
    n_tiles = (span + rec.VOTES_TILE_FRAMES - 1) // rec.VOTES_TILE_FRAMES
    assert span > (120000 if name == "spread120k" else rec.VOTES_TILE_FRAMES) and 2 <= n_tiles <= 8
    nq = max(_n_cus() // 4, 5)
    assert nq * n_tiles >= _n_cus() // 4 and nq < _n_cus()
    g = _kp_handle(manager, name)
    bx, bl, kp, which = _tiled_batch(q[2], q[0], q[1], nq)
    res = g.query_frames(bx, bl, kp)
    assert g.stats()["select_form"] == (0 if mode == "auto" else 1)
    assert all(len(s["cand_frame"]) > 0 for s in sels)
    _check_batch(g, res, sels, which, list(range(5)) + list(range(nq - 5, nq)))
    g.close()


@pytest.mark.parametrize("name,skip", [("dup", 0), ("dup", 2), ("tiny", 0)])
def test_loop_frames_on_duplicate_and_tiny_frames(name, skip):
    """the reference's per-frame loop.  dup: groups of bit-identical frames (60, 49, 50, 51 and 3 members, shuffled): exact
    vote ties among the frames before each one.  tiny: rec.tiny's map frames of 3 .. 6 keypoints and its first 16 once more, votes around 5"""
    from oracle import oracle
    from sgtd_amd import manager, synth
    cfg = {}
    if name == "dup":
        sizes = (60, 49, 50, 51, 3)
        base = synth.make_map(len(sizes), 24, stream=5)
        group = np.repeat(np.arange(len(sizes)), sizes)
        group = group[np.random.default_rng(5).permutation(len(group))]
        xyz, label = base.xyz[group].reshape(-1, 3).copy(), base.label[group].reshape(-1).copy()
        off = np.arange(len(group) + 1, dtype=np.int64) * 24
    else:
        (mx, ml, moff), (qx, ql, qoff) = rec.tiny()       # (the sequence: the map, then its first frames once more)
        xyz, label, off = np.concatenate([mx, qx]), np.concatenate([ml, ql]), np.concatenate([moff, moff[-1] + qoff[1:]])
        cfg = dict(rec.TINY_CONFIG)
    n = len(off) - 1
    ob = oracle.OracleManager(**cfg)
    descs = []
    for i in range(n):
        ob.set_current_frame_id(i)
        descs.append(ob.build(xyz[off[i]:off[i + 1]], label[off[i]:off[i + 1]]))
    o = oracle.OracleManager(**cfg)
    sels, added = [], 0
    for i, d in enumerate(descs):
        while added < i - skip:
            o.add(descs[added])
            added += 1
        r = o.select(d)
        r["best"] = int(o.votes().max())
        sels.append(r)
    if name == "dup":
        assert max(len(s["cand_frame"]) for s in sels) == 50 and any(len(s["cand_frame"]) == 0 for s in sels)
    else:
        assert {4, 5, 6} <= set(s["best"] for s in sels) and any(len(s["cand_frame"]) == 0 and s["best"] > 0 for s in sels)
        assert any(len(s["cand_frame"]) > 0 for s in sels)
    g = manager.STDescManager(**cfg)
    res = g.loop_frames(xyz, label, kp_off=off, skip_near=skip, batch=n)
    for q, r in enumerate(sels):
        nc = len(r["cand_frame"])
        assert int(res.n_cand[q]) == nc, q
        np.testing.assert_array_equal(res.cand_frame[q, :nc], r["cand_frame"], err_msg=str(q))
        np.testing.assert_array_equal(res.cand_votes[q, :nc], r["cand_votes"], err_msg=str(q))
        np.testing.assert_array_equal(res.pair_off[q, :nc + 1], r["cand_off"], err_msg=str(q))
    for q in (range(n) if name == "tiny" else list(range(0, n, 9)) + [n - 1]):
        qi, de = g.result_pairs(q, res)
        np.testing.assert_array_equal(qi, sels[q]["q_idx"], err_msg=str(q))
        np.testing.assert_array_equal(de, sels[q]["db_entry"], err_msg=str(q))
    g.close()
