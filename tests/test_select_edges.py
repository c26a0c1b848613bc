"""The workloads of tests/test_gpu_select_edges.py, checked without a GPU: a plain f64 restatement of candidate_selector
(tests/_select_edges.py) equals the oracle on every query set, and the workloads really reach the selection's edges —
matches and misses within ulps of the threshold, entries within an ulp of a slice boundary, gate ties, runs that must
and must not take the overflow slice, cell 0 probed twice, marker queries with matches, sides past 65535."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _select_edges as se  # noqa: E402


@pytest.fixture(scope="module", params=se.ROUGHS, ids=lambda r: "rough%g" % r)
def case(request, oracle_mod):
    """(workload, restatement answers, oracle answers, audit) of one rough value"""
    wl = se.workload(request.param)
    ref = wl.ref_table()
    o = oracle_mod.OracleManager(rough_dis_threshold=wl.rough)
    wl.load(o, oracle_mod)
    acc = oracle_mod.OrcAudit()
    ours, theirs = [], []
    for k in range(len(wl.sets)):
        side, label, _ = wl.sets[k]
        ours.append(se.ref_select(ref, side, label, se.QUERY_FRAME, wl.rough))
        sel = o.select(wl.query_descs(oracle_mod, k))
        sel.update(votes=o.votes(), M=o.counters()["M"], rough=o.rough_matches())
        theirs.append(sel)
        o.audit_select_query(acc)
    return wl, ours, theirs, acc.as_dict()


def test_restatement_equals_the_oracle(case):
    wl, ours, theirs, _ = case
    for k, (a, b) in enumerate(zip(ours, theirs)):
        where = (wl.rough, k, wl.sets[k][2])
        np.testing.assert_array_equal(a["votes"], b["votes"], err_msg=str(where))
        assert a["M"] == b["M"], where
        for key, ok in (("q_idx", "q_idx"), ("cell", "cell"), ("db_entry", "db_entry")):
            np.testing.assert_array_equal(a["rough"][("q_idx", "cell", "db_entry").index(key)], b["rough"][ok], err_msg=str(where))
        for key in ("cand_frame", "cand_votes", "cand_off", "q_idx", "db_entry"):
            np.testing.assert_array_equal(a[key], b[key], err_msg="%s %s" % (where, key))


def _thr(q, rough):
    return float(se.norm3(q)) * rough


def test_threshold_is_reached_within_ulps_on_both_sides(case):
    wl, ours, theirs, acc = case
    assert acc["min_margin_ulps"] <= 1.0
    assert acc["near_calls"] >= 20
    side, _, _ = wl.ref_table().arrays()
    below = above = 0
    for k in wl.tags["shell"]:
        qs = wl.sets[k][0][:-1]
        for q in qs:
            thr = _thr(q, wl.rough)
            ulp = np.spacing(thr)
            d = se.norm3(side - q)
            below += int(np.sum((d < thr) & (d >= thr - 4 * ulp)))
            above += int(np.sum((d >= thr) & (d <= thr + 4 * ulp)))
    assert below >= 5 and above >= 5, (below, above)


def test_slice_boundaries_and_runs_are_reached(case):
    wl, ours, theirs, _ = case
    side, frame, buckets = wl.ref_table().arrays()
    near = 0
    for v in side[:, 1]:
        y = v + 0.5
        near += abs(y * 2 - round(y * 2)) <= 2 * np.spacing(y * 2)
    for v in side[:, 2]:
        y = v + 0.5
        near += abs(y * 3 - round(y * 3)) <= 2 * np.spacing(y * 3)
    assert near >= 20
    # runs of one frame in one bucket with two sub-cells: some that must take the overflow slice, some that must not,
    # and runs of 47 / 48 / 49 members
    must = must_not = 0
    lengths = set()
    for idx in buckets.values():
        for f in np.unique(frame[idx]):
            run = idx[frame[idx] == f]
            if len(run) < 2:
                continue
            lengths.add(len(run))
            subs = [se.sub_cell(side[g]) for g in run]
            if len(set(subs)) < 2:
                continue
            close = any(not (se.norm3(side[a] - side[b]) > se.run_limit(wl.rough, side[a], side[b]))
                        for x, a in enumerate(run) for y, b in enumerate(run) if y > x and subs[x] != subs[y])
            must += close or len(run) > se.RUN_MAX
            must_not += not close and len(run) <= se.RUN_MAX
    assert must >= 3 and must_not >= (3 if wl.rough < 0.3 else 2 if wl.rough < 1 else 0), (must, must_not)
    if wl.rough <= 0.03:
        assert {47, 48, 49} <= lengths
    # a query matching both members of a close pair in the order insertion gives them (the higher sub-cell first)
    both = 0
    for k in wl.tags["runs"]:
        a, b = ours[k], theirs[k]
        rq, re_ = a["rough"][0], a["rough"][2]
        for i in np.unique(rq):
            e = re_[rq == i]
            if len(e) >= 2 and len(set(frame[e])) < len(e):
                both += 1
    assert both >= 2


def test_gate_ties_cell_zero_and_markers_are_reached(case):
    wl, ours, theirs, acc = case
    assert acc["min_gate_margin"] == 0.0                 # ||side - centre|| == 1.5 exactly
    side, frame, buckets = wl.ref_table().arrays()
    # gate ties next to a bucket (the cell that fails the gate at exactly 1.5 holds an entry within reach)
    ties = 0
    for k in wl.tags["gate"]:
        for q, lab in zip(*wl.sets[k][:2]):
            for x in (-1, 0, 1):
                for y in (-1, 0, 1):
                    for z in (-1, 0, 1):
                        p = (se.c_int(q[0] + x), se.c_int(q[1] + y), se.c_int(q[2] + z))
                        d = [q[j] - (p[j] + 0.5) for j in range(3)]
                        if (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] == 2.25 and (se.label_code(lab),) + p in buckets:
                            ties += 1
    assert ties >= 10
    # cell 0 probed twice: one query descriptor, one entry, two records (cells x = -1 and 0)
    twice = 0
    for k in wl.tags["cells"] + wl.tags["envelope"]:
        rq, rc, re_ = ours[k]["rough"]
        pairs = list(zip(rq.tolist(), re_.tolist()))
        twice += len(pairs) - len(set(pairs))
    assert twice >= 10
    # marker queries (a side at or past 2^cbits - 1 of the configs: 15, 31, 63, 127, 255) with matches, a side past
    # 65535 with matches in the legitimate cells, negative sides with matches
    for lim, want in ((15, 10), (255, 5), (65535, 3)):
        got = 0
        for k in wl.tags["envelope"]:
            qs = wl.sets[k][0]
            rq = ours[k]["rough"][0]
            got += len(np.unique(rq[np.any(qs[rq] >= lim, axis=1)]))
        assert got >= want, (lim, got)
    neg = 0
    for k in wl.tags["envelope"] + wl.tags["cells"]:
        qs = wl.sets[k][0]
        rq = ours[k]["rough"][0]
        neg += int(np.sum(np.any(qs[rq] < 0, axis=1) | np.any(np.signbit(qs[rq]), axis=1)))
    assert neg >= 3


def test_candidates_are_decided_by_the_edges(case):
    """the booster design works: every family has candidates, and frames with no edge match stay below five votes"""
    wl, ours, _, _ = case
    for fam, ks in wl.tags.items():
        if fam == "slices" and wl.rough >= 1:            # (the reach of every query is far beyond its own cell)
            continue
        assert sum(len(ours[k]["cand_frame"]) for k in ks) >= 2, fam
        for k in ks:
            v = ours[k]["votes"][:wl.next_frame]
            assert np.all(v >= se.BOOST)
    if wl.rough == 0.03:
        assert len(wl.sets[wl.tags["big"][0]][0]) > 8192
