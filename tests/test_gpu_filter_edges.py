"""The per-query restriction path (sgtd_set_frame_filter, sgtd_set_position_prior, sgtd_set_frame_poses: the filter pass
over the match records, the diagnostic compaction behind result_rough, the re-basing of the caller's rows, a sharded
handle's row slicing, the rows a prior makes and their caches) at its edges in every form, bit for bit against the
restatement of tests/_filter_edges.py (tests/test_filter_edges.py shows without a GPU that it equals the oracle of the
allowed frames, that the workloads reach their edges and that every mutant of the rule changes an expected answer).

  descriptor cases   every filter of every case, set with the raw sgtd_set_frame_filter arguments the case carries, in the
                     automatic mode, SGTD_SELECT_MODE 1 and 2, search_frame(lists_only=True, allowed=...), a three-shard
                     handle (the cases stamped 0, 1, 2, ...), a view with a filter of its own beside its owner's, a table
                     with a tail segment, deferred lists with finish_lists: the full vote vector, last_M, the candidates,
                     their votes, pair_off and every match list in order; result_rough for the rough family and the first
                     case of every other
  keypoint batches   query_frames with per-query rows, one shared row and rows from a range that starts above the table's
                     first frame, every query with an answer of its own, against the oracle of each query's allowed frames
  position priors    the rule's coordinate and radius edges in 2 and 3 dims on the stamped tables, frames without a pose,
                     the four row-count combinations of prior and filter, and the caches of prepare_filter and
                     prepare_prior in one sequence of batches — each against a second handle under set_frame_filter with
                     the rows test_position_prior_host.prior_rows gives
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _filter_edges as fe  # noqa: E402
import test_gpu_frame_filter as ff  # noqa: E402
import test_gpu_record_edges as tre  # noqa: E402
from test_position_prior_host import prior_rows  # noqa: E402

pytestmark = pytest.mark.gpu
rec = fe.rec

FAMILIES = [f.__name__ for f in fe.FAMILIES]
FORMS = {"auto": {}, "mode1": {"SGTD_SELECT_MODE": "1"}, "mode2": {"SGTD_SELECT_MODE": "2"}, "frame": {}, "multi": {},
         "view": {}, "tail": {}, "deferred": {"SGTD_SELECT_MODE": "2"}}
ROUGH_FORMS = ("auto", "mode2")
FIELDS = ("side", "label", "frame")

_CASES, _EXPECT = {}, {}


def family_cases(family):
    if family not in _CASES:
        _CASES[family] = fe.cases((family,))
    return _CASES[family]


def expected(c, f):
    """the restatement's answer of case c under filter f, with the table entries of its lists"""
    key = (c.name, f.name)
    if key not in _EXPECT:
        exp = fe.ref_filtered(c, 0, f)
        held = exp["held"]
        arrays = dict(zip(FIELDS, c.entry_arrays()))
        exp["entries"] = {k: arrays[k][held][exp["db_entry"]] for k in FIELDS}
        exp["emap"] = np.cumsum(held) - 1
        _EXPECT[key] = exp
    return _EXPECT[key]


def set_filter(g, f):
    """sgtd_set_frame_filter with the case's own arguments (pack_frame_rows would pick a tight range)"""
    from sgtd_amd.manager import _p
    g._check(g._L.sgtd_set_frame_filter(g._h, f.lo, f.n, _p(f.rows), f.rows.shape[0]))


def _check_set(g, exp, tag, multi=False):
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
        for k in FIELDS:
            np.testing.assert_array_equal(getattr(got, k), exp["entries"][k], err_msg=tag + " " + k)
    else:
        assert exp["held"][de].all(), tag + ": an entry of a frame that is not allowed"
        np.testing.assert_array_equal(exp["emap"][de], exp["db_entry"], err_msg=tag)
    tre._check_votes(g, exp, tag)


def _check_frame(g, mod, c, f, exp, tag):
    ids = c.frames()[fe.filt_allows(f, 0, c.frames())]
    out = g.search_frame(c.query_descs(mod, 0), capacity=max(int(exp["cand_off"][-1]), 1), lists_only=True, allowed=ids)
    assert out["status"] == 0, tag
    nc = len(exp["cand_frame"])
    assert out["n_cand"] == nc, tag
    np.testing.assert_array_equal(out["cand_frame"][:nc], exp["cand_frame"], err_msg=tag)
    np.testing.assert_array_equal(out["cand_votes"][:nc], exp["cand_votes"], err_msg=tag)
    np.testing.assert_array_equal(out["pair_off"][:nc + 1], exp["cand_off"], err_msg=tag)
    np.testing.assert_array_equal(out["inlier_q_idx"], exp["q_idx"], err_msg=tag)
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(out["entries"], k), exp["entries"][k], err_msg=tag + " " + k)
    tre._check_votes(g, exp, tag)


def _check_rough(g, exp, tag):
    got, want = g.result_rough(0), exp["rough"]
    for k in ("q_idx", "cell", "frame", "dis"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=tag + " rough " + k)
    assert exp["held"][got["db_entry"]].all(), tag
    np.testing.assert_array_equal(exp["emap"][got["db_entry"]], want["db_entry"], err_msg=tag + " rough db_entry")


def run_form(family, form):
    """every filter of every case of the family through one form; returns the number of (case, filter) pairs checked"""
    from sgtd_amd import manager
    n = 0
    for ci, c in enumerate(family_cases(family)):
        if form == "multi" and not c.stamped:       # (a multi-device table takes one frame per call, ids 0, 1, 2, ...)
            continue
        if form == "tail" and c.tail_at is None:
            continue
        want_form = tre.mode2_form(c) if form in ("mode2", "deferred") else 0
        owner = None
        if form == "multi":
            g = manager.STDescManager(devices=[0, 0, 0], **c.config())
            c.load(g, manager)
        elif form == "tail":
            g = manager.STDescManager(**c.config())
            c.load(g, manager, 0, c.tail_at)
            g.candidate_selector(c.query_descs(manager, 0))            # (the table is built: what follows goes to a tail)
            c.load(g, manager, c.tail_at, None)
        elif form == "view":
            owner = manager.STDescManager(**c.config())
            c.load(owner, manager)
            owner.finalize()
            set_filter(owner, c.filters[-1])
            g = manager.STDescManager(**c.config())
            g.attach_table(owner)
        else:
            g = manager.STDescManager(**c.config())
            c.load(g, manager)
        qd = c.query_descs(manager, 0)
        for fi, f in enumerate(c.filters):
            tag = "%s/%s/%s" % (c.name, f.name, form)
            exp = expected(c, f)
            if form == "frame":
                _check_frame(g, manager, c, f, exp, tag)
            elif form == "deferred":
                set_filter(g, f)
                g.set_deferred_lists(True)
                g.query_descs(qd)
                mask = rec.keep_masks(len(exp["cand_frame"]))["alternating"]
                g.finish_lists(tre._keep_tensor(mask))
                _check_set(g, dict(rec.masked(exp, mask), entries=None), tag + "/alternating")
                g.finish_lists(None)
                _check_set(g, exp, tag + "/unmasked")
                g.set_deferred_lists(False)
            else:
                set_filter(g, f)
                g.candidate_selector(qd)
                _check_set(g, exp, tag, multi=form == "multi")
            assert g.stats()["select_form"] == want_form, tag
            if form == "tail" and fi == 0:
                assert g.stats()["tail_entries"] > 0, tag
            if form in ROUGH_FORMS and (family == "rough" or (ci == 0 and fi == 0)):
                _check_rough(g, exp, tag)
            n += 1
        if owner is not None:      # the owner still answers under its own filter
            owner.candidate_selector(qd)
            _check_set(owner, expected(c, c.filters[-1]), c.name + "/owner")
            g.close()
            owner.close()
        else:
            g.close()
    return n


# (the bits and wide families are caller-stamped frame ids from 1000 on: nothing a multi-device handle takes, and they
# carry no tail)
@pytest.mark.parametrize("form,family", [(fo, fa) for fo in FORMS for fa in FAMILIES
                                          if not (fo in ("multi", "tail") and fa in ("bits", "wide"))])
def test_every_form_equals_the_restatement(family, form, monkeypatch):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    assert run_form(family, form) >= 1


# ---- keypoint batches: per-query rows --------------------------------------------------------------------------------
def _kp():
    """(map, queries, gt, filters, the oracle's descriptors per map frame, the batch: the 12 queries and an empty one)"""
    if "kp" not in _EXPECT:
        from oracle import oracle
        from sgtd_amd import synth
        oracle.build_library()
        m, qs, gt, filters = fe.kp_world(synth)
        ob = oracle.OracleManager()
        descs = []
        for i in range(fe.KP_FRAMES):
            ob.set_current_frame_id(fe.TABLE_LO + i)
            descs.append(ob.build(m.xyz[i], m.label[i]))
        xyz = np.ascontiguousarray(qs.xyz.reshape(-1, 3), np.float32)
        label = np.ascontiguousarray(qs.label.reshape(-1), np.uint32)
        off = np.concatenate([np.arange(fe.KP_QUERIES + 1) * fe.KP_POINTS, [fe.KP_QUERIES * fe.KP_POINTS]]).astype(np.int64)
        _EXPECT["kp"] = (m, qs, gt, filters, descs, (xyz, label, off))
    return _EXPECT["kp"]


def _kp_handle(manager, n=None, **kw):
    m = _kp()[0]
    g = manager.STDescManager(first_frame_id=fe.TABLE_LO, **kw)
    g.add_frames(m.xyz[:n], m.label[:n])
    g.finalize()
    return g


def _kp_oracle_answer(q, local_frames):
    """the oracle of the allowed frames for query q of the batch (q == KP_QUERIES: the empty query)"""
    from oracle import oracle
    m, qs, gt, filters, descs, (xyz, label, off) = _kp()
    o = oracle.OracleManager()
    for i in local_frames:
        o.add(descs[i])
    o.set_current_frame_id(fe.TABLE_LO + fe.KP_FRAMES)
    o.build(xyz[off[q]:off[q + 1]], label[off[q]:off[q + 1]], export=False)
    r = o.select()
    r["votes"] = o.votes()
    return r


@pytest.mark.parametrize("mode", ["auto", "2"])
@pytest.mark.parametrize("name", ["per_query", "shared", "above"])
def test_query_frames_rows_equal_the_oracle_of_each_query(name, mode, monkeypatch):
    from sgtd_amd import manager
    if mode != "auto":
        monkeypatch.setenv("SGTD_SELECT_MODE", mode)
    m, qs, gt, filters, descs, (xyz, label, off) = _kp()
    f = filters[name]
    nq = fe.KP_QUERIES + 1
    counts = np.array([d.n for d in descs])
    ids = fe.TABLE_LO + np.arange(fe.KP_FRAMES)
    g = _kp_handle(manager)
    set_filter(g, f)
    res = g.query_frames(xyz, label, off)
    assert g.result_votes(0)[0] == fe.TABLE_LO                   # (the table starts at first_frame_id)
    answers = []
    for q in range(nq):
        frames = np.nonzero(fe.filt_allows(f, q, ids))[0]
        r = _kp_oracle_answer(q, frames)
        nc = len(r["cand_frame"])
        assert int(res.n_cand[q]) == nc, q
        np.testing.assert_array_equal(res.cand_frame[q, :nc], r["cand_frame"], err_msg=str(q))
        np.testing.assert_array_equal(res.cand_votes[q, :nc], r["cand_votes"], err_msg=str(q))
        np.testing.assert_array_equal(res.pair_off[q, :nc + 1], r["cand_off"], err_msg=str(q))
        qi, de = g.result_pairs(q, res)
        np.testing.assert_array_equal(qi, r["q_idx"], err_msg=str(q))
        np.testing.assert_array_equal(ff._entry_map(counts, frames)(de), r["db_entry"], err_msg=str(q))
        lo, v = g.result_votes(q)
        assert ff._same_votes(lo, v, 0, r["votes"]), q
        answers.append((r["cand_frame"].tolist(), r["cand_votes"].tolist()))
    assert int(res.n_cand[nq - 1]) == 0 and off[nq] == off[nq - 1]                      # the query without a keypoint
    if name != "shared":                                                                # an answer of its own per query
        assert len({str(a) for a in answers[:fe.KP_QUERIES]}) == fe.KP_QUERIES
    assert sum(len(a[0]) > 0 for a in answers) >= 6
    g.close()


# ---- position priors ---------------------------------------------------------------------------------------------------
def _descriptor_pair(manager, c):
    p, f = manager.STDescManager(**c.config()), manager.STDescManager(**c.config())
    for g in (p, f):
        c.load(g, manager)
    return p, f


def _prior_against_filter(manager, c, p, f, has, t, center, radius, tag):
    """handle p under the prior (its poses set by the caller), handle f under the filter of the restatement's rows; ->
    the allowed mask over the table's frames"""
    with np.errstate(over="ignore"):
        allowed = prior_rows(t, has, np.asarray(center, np.float64)[None, :], np.array([radius], np.float64))[0]
    ids = c.frames()
    p.set_position_prior(np.asarray(center, np.float64), radius)
    set_filter(f, fe.make_filter("rule", c.table_lo, c.span, [ids[allowed]], garbage=False))
    qd = c.query_descs(manager, 0)
    p.query_descs(qd)
    f.query_descs(qd)
    ff._same_results(p, f, p.results(), f.results(), 1, verify=False)
    assert p.stats()["last_M"] == f.stats()["last_M"] == (fe.BOOST + 1) * int(allowed.sum()), tag
    lo, v = p.result_votes(0)
    got = np.zeros(len(ids), np.int64)
    inside = (ids - lo >= 0) & (ids - lo < len(v))
    got[inside] = v[(ids - lo)[inside]]
    np.testing.assert_array_equal(got > 0, allowed, err_msg=tag)
    return allowed


def test_prior_decides_its_edges_on_the_stamped_table():
    """every edge of PRIOR_EDGES on the table of span 129 from frame 1000 (span % 64 == 1), the edge pose in turn on local
    frames 0, 63, 64, 65 and 128: the edge frame's vote says which way the decision went"""
    from sgtd_amd import manager
    c = next(x for x in family_cases("bits") if x.info["span"] == 129)
    p, f = _descriptor_pair(manager, c)
    ids = c.frames()
    has = np.ones(len(ids), bool)
    for k, e in enumerate(fe.PRIOR_EDGES):
        t, loc = fe.prior_scene(len(ids), e, k)
        p.set_frame_poses(ids, fe.pose_rows(t))
        allowed = _prior_against_filter(manager, c, p, f, has, t, e[2], e[3], e[0])
        assert bool(allowed[loc]) is e[4], e[0]
    p.close()
    f.close()


@pytest.mark.parametrize("span", fe.WIDE_SPANS)
def test_prior_on_the_wide_tables(span):
    """the rows of a prior over 524 288 and 524 289 frames (the filter pass reads them from LDS and from memory), the edge
    pose on the table's last frame"""
    from sgtd_amd import manager
    c = next(x for x in family_cases("wide") if x.info["span"] == span)
    p, f = _descriptor_pair(manager, c)
    ids = c.frames()
    has = np.ones(len(ids), bool)
    for name in ("r3_exact", "r3_ulp_below", "nan_z_dims2", "overflow_r_inf"):
        e = next(x for x in fe.PRIOR_EDGES if x[0] == name)
        t, _ = fe.prior_scene(len(ids), e, 0)
        t[0], t[-1] = t[1], e[1]
        p.set_frame_poses(ids, fe.pose_rows(t))
        allowed = _prior_against_filter(manager, c, p, f, has, t, e[2], e[3], "%s/%d" % (name, span))
        assert bool(allowed[-1]) is e[4], name
    p.close()
    f.close()


def test_prior_frames_without_a_pose():
    """span 129 from frame 1000 under radius +inf: no pose at local 63 and at the last frame; none at 64; poses only for
    the first 100 frames (ids beyond what the handle holds poses for)"""
    from sgtd_amd import manager
    c = next(x for x in family_cases("bits") if x.info["span"] == 129)
    ids = c.frames()
    t = fe.prior_scene(len(ids), fe.PRIOR_EDGES[0], 0)[0]
    for name, missing in (("63_last", [63, 128]), ("64", [64]), ("short", list(range(100, 129)))):
        p, f = _descriptor_pair(manager, c)
        has = np.ones(len(ids), bool)
        has[missing] = False
        if name == "short":
            p.set_frame_poses(ids[has], fe.pose_rows(t[has]))
        else:
            p.set_frame_poses(ids, fe.pose_rows(t))
            p.set_frame_poses(ids[missing], None)
        allowed = _prior_against_filter(manager, c, p, f, has, t, (0.0, 0.0), np.inf, name)
        assert np.array_equal(allowed, has)
        p.close()
        f.close()


def _kp_poses():
    """poses of the keypoint world's frames: frame i at (10 i, 0, 0), frame 13 at (40, 0, 1)"""
    t = np.zeros((fe.KP_FRAMES, 3), np.float32)
    t[:, 0] = 10.0 * np.arange(fe.KP_FRAMES)
    t[13] = (40.0, 0.0, 1.0)
    return t


def _rows_filter(lo, n, allowed):
    """allowed: bool [rows, n] over the frames lo .. lo + n - 1"""
    return fe.make_filter("rule", lo, n, [lo + np.nonzero(a)[0] for a in allowed], garbage=False)


@pytest.mark.parametrize("prior_rows_n,filter_name", [(1, "shared"), (1, "per_query"), (0, "shared"), (0, "per_query")])
@pytest.mark.parametrize("dims", [2, 3])
def test_prior_and_filter_row_counts(prior_rows_n, filter_name, dims):
    """shared x shared, shared x per-query, per-query x shared, per-query x per-query (prior_rows_n 0: one prior row per
    query) on the keypoint table from frame 1000: a frame is allowed only where both allow it"""
    from sgtd_amd import manager
    m, qs, gt, filters, descs, (xyz, label, off) = _kp()
    nq = fe.KP_QUERIES + 1
    ids = fe.TABLE_LO + np.arange(fe.KP_FRAMES)
    t = _kp_poses()
    has = np.ones(fe.KP_FRAMES, bool)
    if prior_rows_n == 1:
        center, radius = np.array([75.0, 0.0, 0.0])[:dims], 46.0
    else:
        center = np.zeros((nq, dims))
        center[:, 0] = np.concatenate([t[gt, 0], [0.0]]) + 5.0
        radius = 36.0 + np.arange(nq)
    pr = prior_rows(t, has, np.atleast_2d(center), np.broadcast_to(np.asarray(radius, np.float64), (np.atleast_2d(center).shape[0],)))
    fl = filters[filter_name]
    fr = np.stack([fe.filt_allows(fl, q, ids) for q in range(fl.rows.shape[0])])
    both = np.broadcast_to(pr, (nq, fe.KP_FRAMES)) & np.broadcast_to(fr, (nq, fe.KP_FRAMES))
    assert both.sum() < min(np.broadcast_to(pr, both.shape).sum(), np.broadcast_to(fr, both.shape).sum()) and both.any(axis=1).sum() >= 8
    p, f = _kp_handle(manager), _kp_handle(manager)
    p.set_frame_poses(ids, fe.pose_rows(t))
    p.set_position_prior(center, radius)
    set_filter(p, fl)
    set_filter(f, _rows_filter(fe.TABLE_LO, fe.KP_FRAMES, both))
    rp, rf = p.query_frames(xyz, label, off), f.query_frames(xyz, label, off)
    ff._same_results(p, f, rp, rf, nq, verify=False)
    assert p.stats()["last_M"] == f.stats()["last_M"]
    assert int(np.sum(rp.n_cand > 0)) >= 4
    for q in range(nq):                  # no candidate outside what both allow
        assert both[q, rp.cand_frame[q, :rp.n_cand[q]] - fe.TABLE_LO].all(), q
    p.close()
    f.close()


def test_row_caches_follow_every_key():
    """one handle through a sequence of batches in which one key component of prepare_filter / prepare_prior changes at a
    time and every batch has another correct answer: a stale row set would show as the batch before"""
    from sgtd_amd import manager
    m, qs, gt, filters, descs, (xyz, label, off) = _kp()
    n0 = 12
    nq = fe.KP_QUERIES
    bx, bl, boff = xyz[:off[nq]], label[:off[nq]], off[:nq + 1]
    t = _kp_poses()
    ids = fe.TABLE_LO + np.arange(fe.KP_FRAMES)
    p, f = _kp_handle(manager, n0), _kp_handle(manager, n0)
    p.set_frame_poses(ids, fe.pose_rows(t))
    state = dict(have=np.arange(fe.KP_FRAMES) < n0, t=t.copy(), prev=None, prev_allowed=None)
    A = np.isin(np.arange(fe.KP_FRAMES), [0, 1, 2, 3, 4, 8, 9])
    B = np.isin(np.arange(fe.KP_FRAMES), [5, 6, 7, 12, 13])
    P1 = (np.array([35.0, 0.0]), 26.0)
    fa = fe.make_filter("A", fe.TABLE_LO - 1, fe.KP_FRAMES + 1, [ids[A]])
    fb = fe.make_filter("B", fe.TABLE_LO - 1, fe.KP_FRAMES + 1, [ids[B]])

    def step(tag, filt, prior, n=nq, differs=True):
        allowed = state["have"].copy()
        if filt is not None:
            allowed &= fe.filt_allows(filt, 0, ids)
        if prior is not None:
            allowed &= prior_rows(state["t"], np.ones(fe.KP_FRAMES, bool), prior[0][None, :], np.array([prior[1]]))[0]
        set_filter(f, _rows_filter(fe.TABLE_LO, fe.KP_FRAMES, allowed[None, :]))
        rp = p.query_frames(bx[:boff[n]], bl[:boff[n]], boff[:n + 1])
        rf = f.query_frames(bx[:boff[n]], bl[:boff[n]], boff[:n + 1])
        ff._same_results(p, f, rp, rf, n, verify=False)
        assert p.stats()["last_M"] == f.stats()["last_M"], tag
        if differs:
            assert not np.array_equal(allowed, state["prev_allowed"]), tag
            assert not np.array_equal(rp.cand_frame, state["prev"].cand_frame), tag
        state["prev"], state["prev_allowed"] = rp, allowed
        return allowed

    set_filter(p, fa)
    assert step("filter A", fa, None, differs=False)[[0, 4, 8]].all()
    p.set_position_prior(*P1)
    assert np.nonzero(step("prior + the same filter", fa, P1))[0].tolist() == [1, 2, 3, 4]
    p.set_position_prior(None)
    step("the same filter alone", fa, None)
    p.set_frame_filter(None)
    p.set_position_prior(*P1)
    assert np.nonzero(step("prior", None, P1))[0].tolist() == [1, 2, 3, 4, 5, 6]
    p.set_position_prior(None)
    set_filter(p, fb)
    step("filter B alone", fb, None)
    p.set_frame_filter(None)
    p.set_position_prior(*P1)
    step("the same prior again", None, P1)
    state["t"][3] = (500.0, 0.0, 0.0)
    p.set_frame_poses(ids[3:4], fe.pose_rows(state["t"][3:4]))
    assert np.nonzero(step("one pose moved", None, P1))[0].tolist() == [1, 2, 4, 5, 6]
    for g in (p, f):
        g.add_frames(m.xyz[n0:], m.label[n0:])
    state["have"][:] = True
    assert np.nonzero(step("the span grew", None, P1))[0].tolist() == [1, 2, 4, 5, 6, 13]
    for g in (p, f):
        g.remove_frames(ids[:3])
    state["have"][:3] = False
    assert np.nonzero(step("frame_lo moved", None, P1))[0].tolist() == [4, 5, 6, 13]
    assert p.result_votes(0)[0] == fe.TABLE_LO + 3
    step("another batch size", None, P1, n=5, differs=False)
    assert state["prev"].cand_frame.shape[0] == 5
    p.close()
    f.close()
