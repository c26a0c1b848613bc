"""sgtd_set_frame_poses / sgtd_set_position_prior / sgtd_result_world_poses on the device.  Under a position prior each
query must be answered exactly as under sgtd_set_frame_filter with the rows the prior's rule gives on the host
(test_position_prior_host.prior_rows).  Yardsticks are those of test_gpu_frame_filter.py: a second handle under the
equivalent filter, and the oracle that added only the allowed frames, compared bit for bit (candidates, full vote
arrays, ordered match lists, candidate_verify, SearchLoop's choice, sgtd_search_frame and the rough list)."""
import numpy as np
import pytest

import test_gpu_frame_filter as ff
from test_position_prior_host import prior_rows

pytestmark = pytest.mark.gpu

F, GT = ff.F, ff.GT
NQ = len(GT)
RADIUS = 150.0


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from sgtd_amd import _lib, evaluate, manager, synth
    oracle.build_library()
    return oracle, manager, synth, _lib, evaluate


@pytest.fixture(scope="module")
def world(mods):
    """the map of test_gpu_frame_filter.py, its poses as f32 rows (z spread so that dims 3 differs from dims 2)"""
    oracle, _, synth, _, ev = mods
    m = synth.make_map(F, 200, stream=311, spacing=ff.SPACING)
    qs = synth.make_queries(m, NQ, stream=312, frames=GT)
    descs = []
    o = oracle.OracleManager()
    for i in range(F):
        o.set_current_frame_id(i)
        descs.append(o.build(m.xyz[i], m.label[i]))
    rows = np.stack([ev.pose_row(*p) for p in m.pose])
    rows[:, 11] = np.random.default_rng(41).uniform(-120.0, 120.0, F).astype(np.float32)
    return m, descs, qs, rows


def _t(rows):
    return rows[:, [3, 7, 11]]


def _centers(qs, rows, dims):
    """each query's prior: its true (x, y) and, for dims 3, the z of the frame it re-observes"""
    c = np.zeros((NQ, dims))
    c[:, :2] = qs.pose[:, :2]
    if dims == 3:
        c[:, 2] = rows[GT, 11].astype(np.float64) + 30.0
    return c


def _host(rows, center, radius, has=None):
    has = np.ones(len(rows), bool) if has is None else has
    center = np.atleast_2d(np.asarray(center, np.float64))
    return prior_rows(_t(rows), has, center, np.broadcast_to(np.asarray(radius, np.float64), (center.shape[0],)))


def _posed(manager, m, rows, **kw):
    g = ff._new(manager, m, **kw)
    g.set_frame_poses(np.arange(F), rows)
    return g


def _ids(allowed):
    return [np.flatnonzero(a) for a in allowed]


def _same_candidates(ra, rb):
    for k in ("n_cand", "cand_frame", "cand_votes", "pair_off"):
        assert np.array_equal(getattr(ra, k), getattr(rb, k)), k


def _same_rough(a, b, qsel):
    for q in qsel:
        x, y = a.result_rough(q), b.result_rough(q)
        for k in ("q_idx", "cell", "frame", "dis", "db_entry"):
            assert np.array_equal(x[k], y[k]), (k, q)


@pytest.mark.parametrize("dims", [2, 3])
def test_equals_filter_shared_and_per_query(mods, world, dims):
    oracle, manager, _, _, _ = mods
    m, descs, qs, rows = world
    p, f = _posed(manager, m, rows), ff._new(manager, m)
    cen = _centers(qs, rows, dims)
    # one prior for the whole batch, then one per query
    for center, radius in ((cen[0], 2.5 * RADIUS), (cen, RADIUS)):
        allowed = _host(rows, center, radius)
        assert 0 < allowed.sum(axis=1).min() and allowed.sum(axis=1).max() < F
        p.set_position_prior(center, radius)
        f.set_frame_filter(_ids(allowed)[0] if allowed.shape[0] == 1 else _ids(allowed))
        rp, rf = p.query_frames(qs.xyz, qs.label), f.query_frames(qs.xyz, qs.label)
        ff._same_results(p, f, rp, rf, NQ)
        assert int(np.sum(rp.n_cand > 0)) >= 4
        _same_rough(p, f, (0, 5))
    if dims == 2:
        # the oracle of the allowed frames, for the per-query batch
        rp = p.query_frames(qs.xyz, qs.label)
        p.verify()
        bc, bf, bs = p.search_loop(0.4)
        ff._check_against_oracle(oracle, descs, p, rp, bc, bf, bs, qs, _ids(_host(rows, cen, RADIUS)), rough=(1,))
    p.close()
    f.close()


def test_edge_cases(mods, world):
    _, manager, _, _, _ = mods
    m, _, qs, rows = world
    rows = rows.copy()
    p, f, u = _posed(manager, m, rows), ff._new(manager, m), ff._new(manager, m)
    ru = u.query_frames(qs.xyz, qs.label)
    # frame GT[0] at exactly the radius: a 3-4-5 offset from the center
    c = rows[GT[0], [3, 7]].astype(np.float64) - np.array([3.0, 4.0])
    allowed = _host(rows, c, 5.0)
    assert allowed[0, GT[0]]
    p.set_position_prior(c, 5.0)
    f.set_frame_filter(_ids(allowed)[0])
    rp, rf = p.query_frames(qs.xyz, qs.label), f.query_frames(qs.xyz, qs.label)
    ff._same_results(p, f, rp, rf, NQ)
    lo, v = p.result_votes(0)
    assert v[GT[0] - lo] > 0 and GT[0] in rp.cand_frame[0, :rp.n_cand[0]]
    # no pose (forgotten) and a NaN translation: never allowed, not even by radius +inf
    rows[GT[1], 3] = np.nan
    p.set_frame_poses([GT[1]], rows[GT[1]][None])
    p.set_frame_poses([GT[2]], None)
    has = np.ones(F, bool)
    has[GT[2]] = False
    allowed = _host(rows, c, np.inf, has)
    assert allowed.sum() == F - 2 and not allowed[0, GT[1]] and not allowed[0, GT[2]]
    p.set_position_prior(c, np.inf)
    f.set_frame_filter(_ids(allowed)[0])
    rp, rf = p.query_frames(qs.xyz, qs.label), f.query_frames(qs.xyz, qs.label)
    ff._same_results(p, f, rp, rf, NQ)
    for q in (1, 2):
        lo, v = p.result_votes(q)
        lu, vu = u.result_votes(q)
        assert v[GT[q] - lo] == 0 and vu[GT[q] - lu] > 0, q
    # +inf with every pose set: the unrestricted answer
    p.set_frame_poses(np.arange(F), world[3])
    p.set_position_prior(np.zeros(3), np.inf)
    ff._same_results(p, u, p.query_frames(qs.xyz, qs.label), ru, NQ)
    for x in (p, f, u):
        x.close()


def test_prior_and_filter_together(mods, world):
    _, manager, _, _, _ = mods
    m, _, qs, rows = world
    p, f = _posed(manager, m, rows), ff._new(manager, m)
    cen = _centers(qs, rows, 2)
    allowed = _host(rows, cen, RADIUS)
    shared = np.zeros(F, bool)
    shared[ff.SHARED] = True
    both = allowed & shared[None, :]
    assert both.sum() < allowed.sum() and both.sum(axis=1).max() > 0
    p.set_position_prior(cen, RADIUS)
    p.set_frame_filter(ff.SHARED)
    f.set_frame_filter(_ids(both))
    ff._same_results(p, f, p.query_frames(qs.xyz, qs.label), f.query_frames(qs.xyz, qs.label), NQ)
    # a per-query filter and a shared prior
    per_q = [ff.WINDOWS[w] for w in ff.WIN]
    wide = _host(rows, cen[1], 3 * RADIUS)[0]
    p.set_position_prior(cen[1], 3 * RADIUS)
    p.set_frame_filter(per_q)
    f.set_frame_filter([np.intersect1d(w, np.flatnonzero(wide)) for w in per_q])
    ff._same_results(p, f, p.query_frames(qs.xyz, qs.label), f.query_frames(qs.xyz, qs.label), NQ)
    # clearing the filter leaves the prior; clearing the prior leaves the filter
    p.set_frame_filter(None)
    f.set_frame_filter(np.flatnonzero(wide))
    ff._same_results(p, f, p.query_frames(qs.xyz, qs.label), f.query_frames(qs.xyz, qs.label), NQ)
    p.set_frame_filter(ff.SHARED)
    p.set_position_prior(None)
    f.set_frame_filter(ff.SHARED)
    ff._same_results(p, f, p.query_frames(qs.xyz, qs.label), f.query_frames(qs.xyz, qs.label), NQ)
    p.close()
    f.close()


@pytest.mark.parametrize("lists_only", [False, True])
def test_search_frame_with_prior(mods, world, lists_only):
    _, manager, _, _, _ = mods
    m, _, qs, rows = world
    g = _posed(manager, m, rows)
    cen = _centers(qs, rows, 2)
    n_found = 0
    for q in range(NQ):
        allowed = _ids(_host(rows, cen[q], RADIUS))[0]
        d = g.BuildSingleScanSTD(qs.xyz[q], qs.label[q])
        a = g.search_frame(d, capacity=1 << 16, lists_only=lists_only, prior=(cen[q], RADIUS))
        b = g.search_frame(d, capacity=1 << 16, lists_only=lists_only, allowed=allowed)
        assert a["status"] == 0 and b["status"] == 0
        for k in ("n_cand", "cand_frame", "cand_votes", "pair_off", "score", "rot", "t", "inlier_off", "inlier_q_idx", "n_inliers"):
            assert np.array_equal(a[k], b[k]), (q, k)
        for k in ff.DESC_FIELDS:
            assert np.array_equal(getattr(a["entries"], k), getattr(b["entries"], k)), (q, k)
        n_found += a["n_cand"] > 0
    assert n_found >= 5
    # the keyword forms leave nothing behind
    assert getattr(g, "_prior", None) is None
    g.close()


def test_three_shard_handle(mods, world):
    _, manager, _, _, _ = mods
    m, _, qs, rows = world
    single, multi = _posed(manager, m, rows), _posed(manager, m, rows, devices=[0, 0, 0])
    cen = _centers(qs, rows, 3)
    for h in (single, multi):
        h.set_position_prior(cen, RADIUS)
    a, b = single.query_frames(qs.xyz, qs.label), multi.query_frames(qs.xyz, qs.label)
    _same_candidates(a, b)
    assert int(np.sum(a.n_cand > 0)) >= 4
    single.verify()
    multi.verify()
    for x, y in zip(single.search_loop(0.4), multi.search_loop(0.4)):
        assert np.array_equal(x, y)
    for q in range(NQ):
        qa, da = single.result_pairs(q, a)
        qb, db = multi.result_pairs(q, b)
        assert np.array_equal(qa, qb), q
        if len(da):
            ea, eb = single.fetch_entries(da), multi.fetch_entries(db)
            for k in ff.DESC_FIELDS:
                assert np.array_equal(getattr(ea, k), getattr(eb, k)), k
        la, va = single.result_votes(q)
        lb, vb = multi.result_votes(q)
        assert ff._same_votes(la, va, lb, vb), q
        wa, wb = single.result_world_poses(q), multi.result_world_poses(q)
        assert np.array_equal(wa.view(np.uint32), wb.view(np.uint32)), q
    # a 3-shard handle agrees with the equivalent filter as well (the prior reaches every shard)
    f = ff._new(manager, m, devices=[0, 0, 0])
    f.set_frame_filter(_ids(_host(rows, cen, RADIUS)))
    _same_candidates(f.query_frames(qs.xyz, qs.label), b)
    for h in (f, multi, single):
        h.close()


def test_lifecycle(mods, world, tmp_path):
    _, manager, _, _lib, _ = mods
    m, _, qs, rows = world
    cen = _centers(qs, rows, 2)
    allowed = _host(rows, cen, RADIUS)
    ref = ff._new(manager, m)
    ref.set_frame_filter(_ids(allowed))
    r_ref = ref.query_frames(qs.xyz, qs.label)
    # poses set before add_frames take effect
    g = manager.STDescManager()
    g.set_frame_poses(np.arange(F), rows)
    g.set_position_prior(cen, RADIUS)
    g.add_frames(m.xyz, m.label)
    g.finalize()
    _same_candidates(g.query_frames(qs.xyz, qs.label), r_ref)
    # sgtd_remove_frames leaves poses and prior in force (global ids)
    gone = np.arange(0, 40)
    g.remove_frames(gone)
    ref.remove_frames(gone)
    ref.set_frame_filter([np.setdiff1d(a, gone) for a in _ids(allowed)])
    r_ref = ref.query_frames(qs.xyz, qs.label)
    _same_candidates(g.query_frames(qs.xyz, qs.label), r_ref)
    # so does sgtd_load_table (the table file holds no poses)
    ref.save_table(tmp_path / "t.tab")
    g.load_table(tmp_path / "t.tab")
    _same_candidates(g.query_frames(qs.xyz, qs.label), r_ref)
    # a view has poses and a prior of its own
    v = manager.STDescManager()
    v.attach_table(g)
    v.set_position_prior(cen, RADIUS)
    rv = v.query_frames(qs.xyz, qs.label)
    assert np.all(rv.n_cand == 0)
    v.set_frame_poses(np.arange(F), rows)
    _same_candidates(v.query_frames(qs.xyz, qs.label), r_ref)
    v.set_position_prior(None)
    assert int(np.sum(v.query_frames(qs.xyz, qs.label).n_cand)) > int(np.sum(r_ref.n_cand))
    _same_candidates(g.query_frames(qs.xyz, qs.label), r_ref)     # (the owner's prior is untouched)
    v.close()
    # errors: a batch-size mismatch, loop_frames under a prior, ids beyond max_frame_n
    with pytest.raises(_lib.SgtdError) as ei:
        g.query_frames(qs.xyz[:3], qs.label[:3])
    assert ei.value.status == -1
    d = g.BuildSingleScanSTD(qs.xyz[0], qs.label[0])
    with pytest.raises(_lib.SgtdError) as ei:
        g.candidate_selector(d)
    assert ei.value.status == -1
    g.set_position_prior(cen[0], RADIUS)
    with pytest.raises(_lib.SgtdError) as ei:
        g.loop_frames(qs.xyz[:2], qs.label[:2])
    assert ei.value.status == -7
    assert g.current_frame_id_ == F
    L = g._L
    big = np.array([g.config_setting_["max_frame_n"]], np.uint32)
    assert L.sgtd_set_frame_poses(g._h, big.ctypes.data, rows[:1].ctypes.data, 1) == -5
    c, r = np.zeros(2), np.ones(1)
    assert L.sgtd_set_position_prior(g._h, c.ctypes.data, r.ctypes.data, 1, 4) == -1
    assert L.sgtd_set_position_prior(g._h, c.ctypes.data, (-r).ctypes.data, 1, 2) == -1
    assert L.sgtd_set_position_prior(g._h, np.array([np.nan, 0.0]).ctypes.data, r.ctypes.data, 1, 2) == -1
    assert L.sgtd_set_position_prior(g._h, None, r.ctypes.data, 1, 2) == -1
    assert L.sgtd_set_frame_poses(g._h, None, rows.ctypes.data, 3) == -1
    g.set_position_prior(None)
    g.loop_frames(qs.xyz[:2], qs.label[:2])
    for x in (g, ref):
        x.close()


def _world_f32(M12, rel_rot, rel_t):
    """include/sgtd_accel.h's composition restated in numpy f32, one rounding per operation in the stated order"""
    M = np.asarray(M12, np.float32).reshape(3, 4)
    R = np.asarray(rel_rot, np.float64).astype(np.float32)
    t = np.asarray(rel_t, np.float64).astype(np.float32)
    w = np.zeros((3, 4), np.float32)
    for i in range(3):
        for j in range(3):
            w[i, j] = np.float32(np.float32(M[i, 0] * R[0, j]) + np.float32(M[i, 1] * R[1, j])) + np.float32(M[i, 2] * R[2, j])
        w[i, 3] = np.float32(np.float32(np.float32(M[i, 0] * t[0]) + np.float32(M[i, 1] * t[1])) + np.float32(M[i, 2] * t[2])) + M[i, 3]
    return w.reshape(12)


def test_world_poses(mods, world):
    _, manager, _, _, ev = mods
    m, _, qs, rows = world
    g = _posed(manager, m, rows)
    no_pose = int(GT[3])
    g.set_frame_poses([no_pose], None)
    res = g.query_frames(qs.xyz, qs.label)
    g.verify()
    map4 = np.stack([ev.matrix_from_row(r) for r in rows])
    n_checked = n_nan = 0
    for q in range(NQ):
        w = g.result_world_poses(q)
        assert w.shape == (g.config_setting_["candidate_num"], 12) and w.dtype == np.float32
        score, rot, t = g.result_verify(q)
        for k in range(w.shape[0]):
            fr = int(res.cand_frame[q, k]) if k < res.n_cand[q] else -1
            if k >= res.n_cand[q] or score[k] < 0 or fr == no_pose:
                assert np.isnan(w[k]).all(), (q, k)
                n_nan += k < res.n_cand[q]
                continue
            want = _world_f32(rows[fr], rot[k], t[k])
            assert np.array_equal(w[k].view(np.uint32), want.view(np.uint32)), (q, k)
            nt = np.eye(4, dtype=np.float32)
            nt[:3, :3] = rot[k].astype(np.float32)
            nt[:3, 3] = t[k].astype(np.float32)
            acc = (map4[fr] @ nt).astype(np.float32)      # evaluate.account's composition
            assert np.allclose(w[k].reshape(3, 4), acc[:3], rtol=0, atol=1e-4), (q, k)
            n_checked += 1
    assert n_checked >= 8 and n_nan >= 1
    # candidate_num rows even for a query without candidates; before a verification: SGTD_ERR_INVALID
    g.query_frames(qs.xyz, qs.label)
    from sgtd_amd import _lib
    with pytest.raises(_lib.SgtdError):
        g.result_world_poses(0)
    g.close()


def test_metrics_equal_frames_near(mods):
    _, manager, synth, _, ev = mods
    smap = synth.make_map(1500, 200, stream=314)
    q = synth.make_queries(smap, 96, stream=315)
    rows = np.stack([ev.pose_row(*p) for p in smap.pose])
    map_pose = np.stack([ev.matrix_from_row(r) for r in rows])
    q_pose = np.stack([ev.pose_matrix(*p) for p in q.pose])
    allowed = ev.frames_near(rows[:, [3, 7]], q.pose[:, :2], 50.0)
    assert 5 < allowed.sum(axis=1).mean() < 200
    mgr = ff._new(manager, smap)
    mgr.set_frame_poses(np.arange(len(rows)), rows)
    a = ev.evaluate_batch(mgr, map_pose, q.xyz, q.label, q_pose, allowed=allowed)
    b = ev.evaluate_batch(mgr, map_pose, q.xyz, q.label, q_pose, prior=(q.pose[:, :2], 50.0))
    assert a.summary() == b.summary()
    assert b.score_num > 48
    mgr.close()


def test_rows_at_scale_10000_frames(mods):
    _, manager, synth, _, ev = mods
    big, nq = 10000, 2048
    m = synth.make_map(big, 200, stream=1)
    qs = synth.make_queries(m, nq, stream=316)
    rows = np.stack([ev.pose_row(*p) for p in m.pose])
    allowed = ev.frames_near(rows[:, [3, 7]], qs.pose[:, :2], 50.0)
    assert allowed.sum(axis=1).min() > 0
    p, f = ff._new(manager, m), ff._new(manager, m)
    p.set_frame_poses(np.arange(big), rows)
    p.set_position_prior(qs.pose[:, :2], 50.0)
    f.set_frame_filter(allowed)
    rp, rf = p.query_frames(qs.xyz, qs.label), f.query_frames(qs.xyz, qs.label)
    _same_candidates(rp, rf)
    assert p.stats()["last_M"] == f.stats()["last_M"]
    assert int(np.sum(rp.n_cand > 0)) > nq // 2
    for q in (0, 777, nq - 1):
        lp, vp = p.result_votes(q)
        lf, vf = f.result_votes(q)
        assert ff._same_votes(lp, vp, lf, vf), q
    # a repeated batch reuses the rows; a new prior replaces them
    _same_candidates(p.query_frames(qs.xyz, qs.label), rf)
    p.set_position_prior(qs.pose[0, :2], 50.0)
    f.set_frame_filter(np.flatnonzero(allowed[0]))
    _same_candidates(p.query_frames(qs.xyz, qs.label), f.query_frames(qs.xyz, qs.label))
    p.close()
    f.close()
