"""sgtd_overlap and sgtd_align_keypoints on the edge workloads of tests/_keypoint_edges.py, in every form of the calls,
against the numpy restatements (tests/_overlap_ref.py, tests/_align_ref.py).  tests/test_keypoint_edges.py shows on the
CPU that the workloads keep their promises and that mutants of the rule are caught by them.

One batch is verified and its start poses are read back (sgtd_result_verify / sgtd_result_refined return them to the
bit); workload i is built from the pose of one verified candidate of query i, its frame keypoints are handed to that
candidate's frame (every other frame has none stored) and its query keypoints are query i's.  A run is one (radius,
iterations) of both passes over the whole batch; a workload is compared in the runs it lists.

What is compared how.  The before-figures against the restatement under the start pose and against sgtd_result_overlap,
to the bit.  The after-figures and the assignment against the restatement evaluated at the pose the device returned, to
the bit.  n_fits, n_corr, stop, the assignment and the moments against the restatement's own run, exactly; the pose to
max |dR| <= 1e-9, |dt| <= 1e-9 (1 + |cp| + |cw|).  Nothing is skipped: the restatement's run from the device's start
pose must keep every decision after the first fit 1e-3 m^2 from its threshold and fit no collinear set, or the test
fails.  Every promise of a workload is asserted again on the device's own numbers.  No expectation is taken from the
device: the other forms (more than 4096 slots: the frame-ordered dispatch; three shards; a view) must give the bits of
the single handle, which is compared with the restatement."""
import numpy as np
import pytest

import _align_ref as al
import _keypoint_edges as ke
import _overlap_ref as ov

pytestmark = pytest.mark.gpu

F, NQ, SPACING = 300, 96, 12.0
NB = 80              # queries of the plain batch: 4000 (query, candidate) slots, below the ordered dispatch's 4096
TOL = 1e-9
INT_KEYS = ("n_fits", "n_corr", "stop")
DBL_KEYS = ("overlap_before", "rms_before", "overlap_after", "rms_after")


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, evaluate, manager, synth
    return manager, synth, _lib, evaluate


@pytest.fixture(scope="module")
def world(mods):
    _, synth, _, ev = mods
    m = synth.make_map(F, 200, stream=411, spacing=SPACING)
    qs = synth.make_queries(m, NQ, stream=412)
    rows = np.stack([ev.pose_row(*p) for p in m.pose])
    return m, qs, rows


def _new(manager, m, rows, **kw):
    g = manager.STDescManager(**kw)
    g.add_frames(m.xyz, m.label)
    g.finalize()
    g.set_frame_poses(np.arange(len(rows)), rows)
    return g


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)]))


def _start_poses(g, q, refined):
    score, rot, t = g.result_verify(q)
    if refined:
        r = g.result_refined(q)
        rot, t = r["rot"], r["t"]
    return score, rot, t


def _batch(g, qs, nq, refined):
    res = g.query_frames(qs.xyz[:nq], qs.label[:nq])
    g.verify()
    if refined:
        g.refine_poses(1)
    return res


def _build(g, res, refined, large=True):
    """[(workload or None, q, k, frame, R, t)]: workload i from the start pose of a verified candidate of query i"""
    bl = ke.builders()
    assert len(bl) <= NB
    poses = {}

    def verified(q):
        score, rot, t = _start_poses(g, q, refined)
        poses[q] = (rot, t)
        return [(k, int(res.cand_frame[q, k])) for k in range(int(res.n_cand[q])) if score[k] >= 0]
    out = []
    for i, ((name, build), (q, k, f)) in enumerate(zip(bl, ke.place(len(bl), verified))):
        R, t = poses[q][0][k].copy(), poses[q][1][k].copy()
        wl = build(R, t, i)
        assert wl.name == name
        out.append((wl if large or not wl.large else None, q, k, f, R, t))
    return out


def _store(g, placed):
    """the workloads' frame keypoints, and no others"""
    g.set_frame_keypoints(None, None)
    live = [p for p in placed if p[0] is not None]
    off = np.concatenate([[0], np.cumsum([len(p[0].f_lab) for p in live])])
    g.set_frame_keypoints([p[3] for p in live], np.concatenate([p[0].f_xyz for p in live]), np.concatenate([p[0].f_lab for p in live]), off)


def _query_arrays(placed, nq):
    sets = {p[1]: p[0] for p in placed if p[0] is not None}
    xyz = [sets[q].q_xyz if q in sets else np.zeros((0, 3), np.float32) for q in range(nq)]
    lab = [sets[q].q_lab if q in sets else np.zeros(0, np.uint32) for q in range(nq)]
    return np.concatenate(xyz), np.concatenate(lab), np.concatenate([[0], np.cumsum([len(x) for x in lab])])


def _all_runs(placed):
    return sorted({run for p in placed if p[0] is not None for run in p[0].runs})


def _run(g, run, refined, arrays):
    """both passes over the batch -> fetch(q, k): everything the calls hand out for one slot"""
    radius, iterations = run
    kw = dict(zip(("xyz", "label", "kp_off"), arrays)) if arrays is not None else {}
    g.overlap(radius, refined=refined, **kw)
    g.align_keypoints(radius, iterations=iterations, refined=refined, **kw)
    cache = {}

    def fetch(q, k):
        if q not in cache:
            cache[q] = (g.result_aligned(q), g.result_overlap(q))
        a, o = cache[q]
        out = {key: np.array(a[key][k]) for key in a}
        out.update({"o_" + key: np.array(o[key][k]) for key in o})
        out["pairs"] = g.result_aligned_pairs(q, k)
        return out
    return fetch


def _same_raw(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) if a[k].dtype.kind == "i" else _same_bits(a[k], b[k]) for k in a)


def _figures(raw, which):
    c = raw["counts_" + which]
    return dict(n_query_kp=int(c[0]), n_frame_kp=int(c[1]), n_hit_query=int(c[2]), n_hit_frame=int(c[3]), overlap=raw["overlap_" + which],
                rms=raw["rms_" + which])


def _as_result(raw):
    return dict(before=_figures(raw, "before"), after=_figures(raw, "after"), assign=raw["pairs"], n_fits=int(raw["n_fits"]),
                n_corr=int(raw["n_corr"]), stop=int(raw["stop"]))


def _compare(raw, wl, R, t, run):
    """one slot against the restatement; nothing is skipped"""
    w = (wl.name, run)
    radius, iterations = run
    exp = ke.reference(wl, R, t, radius, iterations)
    assert exp["late_margin"] >= ke.MARGIN and not exp["collinear"], (w, exp["late_margin"])
    assert raw["pairs"].shape == wl.q_lab.shape, w
    for key in ov.KEYS:                                # sgtd_result_overlap is the before-result
        assert ov.same_value(exp["before"][key], _figures(raw, "before")[key]), (w, "before", key, exp["before"][key], _figures(raw, "before")[key])
        assert ov.same_value(exp["before"][key], raw["o_" + key]), (w, "overlap", key)
    after, asg = al.evaluate(raw["rot"], raw["t"], wl.q_xyz, wl.q_lab, wl.f_xyz, wl.f_lab, radius)
    for key in ov.KEYS:
        assert ov.same_value(after[key], _figures(raw, "after")[key]), (w, "after", key, after[key], _figures(raw, "after")[key])
    assert np.array_equal(raw["pairs"], asg), w
    for key in INT_KEYS:
        assert int(raw[key]) == exp[key], (w, key, int(raw[key]), exp[key])
    assert _same_bits(raw["moments"], exp["moments"]), (w, "moments")
    assert np.array_equal(raw["pairs"], exp["assign"]), w
    if exp["n_fits"] == 0:
        assert _same_bits(raw["rot"], R) and _same_bits(raw["t"], t), w          # the start pose stands
    else:
        cp, cw = exp["moments"][:3], exp["moments"][3:6]
        assert np.abs(raw["rot"] - exp["rot"]).max() <= TOL, w
        assert np.abs(raw["t"] - exp["t"]).max() <= TOL * (1 + np.linalg.norm(cp) + np.linalg.norm(cw)), w


def _check_choices(g, res, nq, bounds_aligned, gates):
    """sgtd_search_loop_aligned and sgtd_search_loop_overlap against their restated rules on the handle's own results"""
    per_q = [(g.result_verify(q)[0], g.result_aligned(q), g.result_overlap(q)["overlap"]) for q in range(nq)]
    chosen = {}
    for bounds in bounds_aligned:
        bc, bf, br, bo = g.search_loop_aligned(*bounds)
        for q, (score, r, _) in enumerate(per_q):
            want = al.search_loop_aligned(score, r["overlap_after"], r["rms_after"], r["stop"], int(res.n_cand[q]), res.cand_frame[q], *bounds)
            assert (int(bc[q]), int(bf[q])) == want[:2] and ov.same_value(want[2], br[q]) and ov.same_value(want[3], bo[q]), (bounds, q)
        chosen[("aligned", bounds[0])] = bc
    for gate in gates:
        bc, bf, bs, bo = g.search_loop_overlap(gate, icp_threshold=0.0)
        for q, (score, _, o) in enumerate(per_q):
            want = ov.search_loop_overlap(score, o, int(res.n_cand[q]), res.cand_frame[q], 0.0, gate)
            assert (int(bc[q]), int(bf[q])) == want[:2] and ov.same_value(want[2], bs[q]) and ov.same_value(want[3], bo[q]), (gate, q)
        chosen[("overlap", gate)] = bc
    return chosen


@pytest.fixture(scope="module")
def base(mods, world):
    """the single handle with explicit query keypoints: every workload in every run it lists, compared with the restatement
    -> (handle, placed, {(name, run): what the calls handed out})"""
    manager, _, _, _ = mods
    m, qs, rows = world
    g = _new(manager, m, rows)
    res = _batch(g, qs, NB, False)
    assert NB * g.config_setting_["candidate_num"] < 4096
    placed = _build(g, res, False)
    _store(g, placed)
    arrays = _query_arrays(placed, NB)
    raws = {}
    by_name = {p[0].name: p for p in placed}
    for run in _all_runs(placed):
        fetch = _run(g, run, False, arrays)
        for wl, q, k, f, R, t in placed:
            if run in wl.runs:
                raws[(wl.name, run)] = fetch(q, k)
        # the choice on a candidate whose overlap sits exactly on min_overlap: threshold/query has 1 hit of 8 at r1, none at r0
        wl, q, k, _, _, _ = by_name["threshold/query"]
        if run in wl.runs or run == (1.0, 3):
            up = float(np.nextafter(0.125, 1.0))
            chosen = _check_choices(g, res, NB, [(0.0, 0.0), (0.125, 0.0), (up, 0.0), (0.4, 0.2)], [0.125, up, 0.4])
            if run in wl.runs:
                inside = bool(wl.info["m"] <= np.float64(run[0]) * np.float64(run[0]))
                assert int(chosen[("aligned", 0.125)][q]) == (k if inside else -1) and int(chosen[("aligned", up)][q]) == -1, run
                assert int(chosen[("overlap", 0.125)][q]) == (k if inside and g.result_verify(q)[0][k] > 0 else -1), run
                assert int(chosen[("overlap", up)][q]) == -1, run
    yield g, res, placed, raws
    g.close()


def test_explicit_keypoints_on_a_single_handle(base):
    """form 1: every workload against the restatement, and every promise on the device's own numbers"""
    g, res, placed, raws = base
    n = 0
    for wl, q, k, f, R, t in placed:
        for run in wl.runs:
            _compare(raws[(wl.name, run)], wl, R, t, run)
            n += 1
        wl.promise({run: _as_result(raws[(wl.name, run)]) for run in wl.runs})
    stops = {(run[1], int(raws[(name, run)]["stop"])) for name, run in raws}
    print("%d workloads, %d comparisons, none skipped; (iterations, stop) seen %s" % (len(placed), n, sorted(stops)))
    assert {(1, 0), (2, 0), (3, 2), (5, 2), (5, 1), (3, 1)} <= stops
    assert ke.overlap_lds_bytes(ke.MAX_KP) > 65536 and ke.align_lds_bytes(ke.MAX_KP) > 65536       # what the launches of this form asked for


def _other_form(g, nq, base, qs, refined=False):
    """the base's workloads on another handle or batch: the same start poses, the same bits"""
    _, _, placed, raws = base
    res = _batch(g, qs, nq, refined)
    for wl, q, k, f, R, t in placed:
        score, rot, tt = _start_poses(g, q, refined)
        assert int(res.cand_frame[q, k]) == f and _same_bits(rot[k], R) and _same_bits(tt[k], t), (wl.name, q, k)
    _store(g, placed)
    arrays = _query_arrays(placed, nq)
    n = 0
    for run in _all_runs(placed):
        fetch = _run(g, run, refined, arrays)
        for wl, q, k, f, R, t in placed:
            if run in wl.runs:
                assert _same_raw(fetch(q, k), raws[(wl.name, run)]), (wl.name, run)
                n += 1
    assert n == len(raws) >= len(placed)
    return n


def test_frame_ordered_dispatch(mods, world, base):
    """form 4: 96 queries, 4800 (query, candidate) slots: the workgroups run in the order of the candidates' frames"""
    manager, _, _, _ = mods
    m, qs, rows = world
    g = _new(manager, m, rows)
    assert NQ * g.config_setting_["candidate_num"] >= 4096
    _other_form(g, NQ, base, qs)
    g.close()


def test_three_shard_handle(mods, world, base):
    """form 5: three shards on the one GPU"""
    manager, _, _, _ = mods
    m, qs, rows = world
    g = _new(manager, m, rows, devices=[0, 0, 0])
    _other_form(g, NB, base, qs)
    g.close()


def test_view(mods, world, base):
    """form 6: a view of the base handle's table, with a store and results of its own"""
    manager, _, _, _ = mods
    _, qs, _ = world
    v = manager.STDescManager()
    v.attach_table(base[0])
    _other_form(v, NB, base, qs)
    v.close()


def test_refined_start_poses(mods, world):
    """form 3: the workloads built around sgtd_refine_poses' poses (the 65535-keypoint ones aside), SGTD_*_REFINED"""
    manager, _, _, _ = mods
    m, qs, rows = world
    g = _new(manager, m, rows)
    res = _batch(g, qs, NB, True)
    placed = [p for p in _build(g, res, True, large=False) if p[0] is not None]
    _store(g, placed)
    arrays = _query_arrays(placed, NB)
    raws = {}
    for run in _all_runs(placed):
        fetch = _run(g, run, True, arrays)
        raws.update({(p[0].name, run): fetch(p[1], p[2]) for p in placed if run in p[0].runs})
    for wl, q, k, f, R, t in placed:
        for run in wl.runs:
            _compare(raws[(wl.name, run)], wl, R, t, run)
        wl.promise({run: _as_result(raws[(wl.name, run)]) for run in wl.runs})
    assert len(placed) == len(ke.builders()) - 3
    g.close()


def test_the_batchs_own_keypoints(mods, world):
    """form 2: no explicit keypoints: workloads planted around the world's own query keypoints (sgtd_query_frames' batch)"""
    manager, _, _, _ = mods
    m, qs, rows = world
    nq = 16
    g = _new(manager, m, rows)
    res = _batch(g, qs, nq, False)
    poses = {}

    def verified(q):
        score, rot, t = _start_poses(g, q, False)
        poses[q] = (rot, t)
        return [(k, int(res.cand_frame[q, k])) for k in range(int(res.n_cand[q])) if score[k] >= 0]
    placed = []
    for q, k, f in ke.place(nq, verified):
        R, t = poses[q][0][k].copy(), poses[q][1][k].copy()
        placed.append((ke.own_keypoints(R, t, q, qs.xyz[q], qs.label[q]), q, k, f, R, t))
    _store(g, placed)
    fetch = _run(g, (0.5, 3), False, None)
    for wl, q, k, f, R, t in placed:
        raw = fetch(q, k)
        _compare(raw, wl, R, t, (0.5, 3))
        wl.promise({(0.5, 3): _as_result(raw)})
    g.close()


def test_store_sequence(base):
    """the 65535-keypoint frames are stored, then forgotten: the longest stored frame, and with it the dynamic LDS and the
    offsets of the hit bytes and of the assignment, shrink between two runs; every other workload's results stay"""
    g, res, placed, raws = base
    run = (1.0, 3)
    arrays = _query_arrays(placed, NB)
    big = [p for p in placed if len(p[0].f_lab) == ke.MAX_KP]
    assert len(big) == 2 and max(len(p[0].f_lab) for p in placed if p not in big) == 3 * ke.TILE + 3
    assert ke.align_lds_bytes(3 * ke.TILE + 3) < 65536 < ke.align_lds_bytes(ke.MAX_KP)
    g.set_frame_keypoints([p[3] for p in big], None)
    fetch = _run(g, run, False, arrays)
    n = 0
    for wl, q, k, f, R, t in placed:
        if run not in wl.runs:
            continue
        raw = fetch(q, k)
        if len(wl.f_lab) == ke.MAX_KP:
            assert tuple(raw["counts_after"]) == (8, -1, 0, 0) and (int(raw["n_fits"]), int(raw["stop"])) == (0, 1) and (raw["pairs"] == -1).all()
            assert int(raw["o_n_frame_kp"]) == -1 and _same_bits(raw["rot"], R)
        else:
            assert _same_raw(raw, raws[(wl.name, run)]), wl.name
            n += 1
    assert n >= 50
    _store(g, placed)                                  # and stored again: the first run's bits
    fetch = _run(g, run, False, arrays)
    for wl, q, k, f, R, t in placed:
        if run in wl.runs:
            assert _same_raw(fetch(q, k), raws[(wl.name, run)]), wl.name
