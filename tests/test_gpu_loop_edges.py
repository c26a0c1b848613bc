"""sgtd_loop_frames at the edge of its bound (the BOUND variants of the sweep, loop_bound_kernel) in every form of a loop
batch, against the oracle driven through the reference's loop build -> select -> add.  Workloads: tests/_loop_edges.py
(tests/test_loop_edges.py shows without a GPU that they are sharp).  Compared bit for bit, frame by frame: the candidates,
their votes, pair_off, the ordered match lists, the whole vote array (result_votes: a frame outside the bound gets no
vote) and, for two frames of every workload, result_rough.

  forms   one_call; batch1 (one frame per sgtd_loop_frames call); straddle (chunks that put a twin and its source on either
          side of a chunk boundary); mode1 / mode2 (SGTD_SELECT_MODE); rec_cap (SGTD_REC_CAP=1024: the batch overflows and
          re-runs, and the re-run applies the bound again); verify (verify + search_loop against the oracle's); for the
          session on a prebuilt map also tail (the session stays in the tail segment) and tail_merged (SGTD_TAIL_MAX=1).
          The narrow and the wide key configuration are workloads of their own (bound, bound_wide).  Every environment
          variable used here is read when a handle is created.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _loop_edges as le  # noqa: E402

pytestmark = pytest.mark.gpu

S_ALL = le.all_sessions()
FORMS = {"one_call": {}, "batch1": {}, "straddle": {}, "mode1": {"SGTD_SELECT_MODE": "1"}, "mode2": {"SGTD_SELECT_MODE": "2"},
         "rec_cap": {"SGTD_REC_CAP": "1024"}, "verify": {}, "tail": {}, "tail_merged": {"SGTD_TAIL_MAX": "1"}}
STRADDLE = dict(bound=7, bound_wide=7, tied=9, first_large=5, short=9, removed_head=4, removed_hole=4, on_map=3)
COMBOS = [(n, k, f) for n, s in S_ALL.items() for k in s.skips for f in FORMS
          if not (f in ("tail", "tail_merged") and (s.M == 0 or s.removed))]
_MEMO = {}


def _oracle():
    from oracle import oracle
    oracle.build_library()
    return oracle


def rough_frames(s):
    return (max(t for t in s.twins if t >= s.M) - s.M, s.F - 1)


def expected(name, skip):
    """the oracle's loop over the workload, once per skip_near (rough lists of two frames, verification of every frame)"""
    if (name, skip) not in _MEMO:
        s = S_ALL[name]
        _MEMO[(name, skip)] = s.oracle_loop(_oracle(), skip, rough=rough_frames(s), verify=range(s.F))
    return _MEMO[(name, skip)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def check_chunk(g, res, want, tag):
    """the frames of the last loop batch (res: its BatchResult) against the oracle's selects"""
    for q, r in enumerate(want):
        t = "%s frame +%d" % (tag, q)
        nc = len(r["cand_frame"])
        assert int(res.n_cand[q]) == nc, t
        np.testing.assert_array_equal(res.cand_frame[q, :nc], r["cand_frame"], err_msg=t)
        np.testing.assert_array_equal(res.cand_votes[q, :nc], r["cand_votes"], err_msg=t)
        np.testing.assert_array_equal(res.pair_off[q, :nc + 1], r["cand_off"], err_msg=t)
        qi, de = g.result_pairs(q, res)
        np.testing.assert_array_equal(qi, r["q_idx"], err_msg=t)
        np.testing.assert_array_equal(de, r["db_entry"], err_msg=t)
        lo, v = g.result_votes(q)
        assert {int(lo + k): int(v[k]) for k in np.flatnonzero(v)} == r["votes"], t


def prepared(manager, s, form):
    """the handle as the session finds it: the map added, finalized for the tail forms, its removed frames taken out"""
    g = manager.STDescManager(**s.manager_cfg())
    if s.M:
        x, l, off = s.ragged(0, s.M)
        g.add_frames(x, l, kp_off=off)
        if form in ("tail", "tail_merged") or s.removed:
            g.finalize()
        if s.removed:
            assert g.remove_frames([s.first + m for m in s.removed]) > 0
    assert g.current_frame_id_ == s.c
    return g


def run_form(name, skip, form):
    from sgtd_amd import manager
    s = S_ALL[name]
    want = expected(name, skip)
    tag = "%s/skip%d/%s" % (name, skip, form)
    g = prepared(manager, s, form)
    B = {"batch1": 1, "straddle": STRADDLE[name], "tail": 2, "tail_merged": 2}.get(form, s.F)
    for f0 in range(0, s.F, B):
        n = min(B, s.F - f0)
        x, l, off = s.ragged(s.M + f0, s.M + f0 + n)
        res = g.loop_frames(x, l, kp_off=off, skip_near=skip, batch=n)
        assert np.array_equal(res.query_frame_id, s.c + f0 + np.arange(n)), tag
        check_chunk(g, res, want[f0:f0 + n], "%s chunk %d" % (tag, f0))
        if form == "tail" and f0 == 0:
            assert g.stats()["tail_entries"] > 0, tag
        if form == "tail_merged":
            g.sync()
            assert g.stats()["tail_entries"] == 0, tag
        if form == "rec_cap" and sum(sum(r["votes"].values()) for r in want) > 1024:
            assert g.stats()["overflowed"] == 1, tag
    st = g.stats()
    assert g.current_frame_id_ == s.c + s.F, tag
    assert st["n_entries"] == sum(d.n for i, d in enumerate(s.descs(_oracle())) if i not in s.removed), tag
    if form == "one_call":
        for q in rough_frames(s):
            got, ref = g.result_rough(q), want[q]["rough"]
            for key in ("q_idx", "cell", "db_entry", "frame"):
                np.testing.assert_array_equal(got[key], ref[key], err_msg="%s rough %s %d" % (tag, key, q))
            np.testing.assert_array_equal(_bits(got["dis"]), _bits(ref["dis"]), err_msg="%s rough dis %d" % (tag, q))
            assert np.all(got["frame"].astype(np.int64) + skip < s.c + q), tag
    if form == "verify":
        g.verify()
        bc, bf, bs = g.search_loop()
        for q in range(s.F):
            cands, (k, f, sc) = want[q]["verify"]
            score, rot, t = g.result_verify(q)
            for j, (o_s, o_t, o_rot) in enumerate(cands):
                assert score[j] == o_s, (tag, q, j)
                if o_s >= 0:
                    assert np.array_equal(t[j], o_t) and np.array_equal(rot[j], o_rot), (tag, q, j)
            assert int(bf[q]) == f and float(bs[q]) == sc, (tag, q)
            if f >= 0:
                assert int(bc[q]) == k, (tag, q)
    g.close()
    return want


@pytest.mark.parametrize("name, skip, form", COMBOS, ids=["%s-skip%d-%s" % c for c in COMBOS])
def test_every_form_equals_the_reference_loop(name, skip, form, monkeypatch):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    run_form(name, skip, form)


def test_the_twins_show_exactly_below_their_distance():
    """what the workloads are for, read off the oracle's loops the GPU forms are compared with: a twin's source is a
    candidate when skip_near is below the twins' distance and gets no vote from it otherwise"""
    for name, s in S_ALL.items():
        for skip in s.skips:
            want = expected(name, skip)
            for t, src in s.twins.items():
                if t < s.M:
                    continue
                r, fid = want[t - s.M], s.first + src
                if skip < t - src and src not in s.removed:
                    assert fid in r["cand_frame"].tolist() and r["votes"][fid] >= 100, (name, skip, t)
                else:
                    assert fid not in r["votes"], (name, skip, t)
    # tied twins: equal votes, the lower frame first, and search_loop's choice is the first of the two
    r = expected("tied", 0)[14]
    assert r["cand_frame"][:2].tolist() == [3, 9] and r["cand_votes"][0] == r["cand_votes"][1]
    cands, (k, f, sc) = r["verify"]
    assert cands[0][0] == cands[1][0] and (k, f) == ((0, 3) if sc > 0 else (None, -1))


def test_a_session_past_the_frame_limit_changes_nothing():
    """a session that would pass max_frame_n returns SGTD_ERR_FRAME_LIMIT; the frame counter, the entries and a plain
    query batch are then those of a handle that never made the call"""
    from sgtd_amd import manager
    s = S_ALL["on_map"]
    cfg = dict(s.manager_cfg(), max_frame_n=s.c + s.F - 2)
    hs = []
    for _ in range(2):
        g = manager.STDescManager(**cfg)
        x, l, off = s.ragged(0, s.M)
        g.add_frames(x, l, kp_off=off)
        hs.append(g)
    g, fresh = hs
    x, l, off = s.ragged(s.M, s.M + s.F)
    with pytest.raises(manager.SgtdError) as ei:
        g.loop_frames(x, l, kp_off=off, skip_near=1, batch=s.F)
    assert ei.value.status == -5
    assert g.current_frame_id_ == fresh.current_frame_id_ == s.c
    assert g.stats()["n_entries"] == fresh.stats()["n_entries"] and g.stats()["n_frames"] == fresh.stats()["n_frames"]
    x, l, off = s.ragged(s.M, s.M + 4)
    a, b = g.query_frames(x, l, kp_off=off), fresh.query_frames(x, l, kp_off=off)
    for k in ("n_cand", "cand_frame", "cand_votes", "pair_off"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert int(a.n_cand[0]) > 0                              # session frame 0 copies map frame 1
    for q in range(4):
        assert all(np.array_equal(u, v) for u, v in zip(g.result_pairs(q, a), fresh.result_pairs(q, b)))
    # ... and the handle still takes a session that fits
    x, l, off = s.ragged(s.M, s.M + s.F - 2)
    res = g.loop_frames(x, l, kp_off=off, skip_near=1, batch=s.F)
    check_chunk(g, res, expected("on_map", 1)[:s.F - 2], "after the refused session")
    for h in hs:
        h.close()
