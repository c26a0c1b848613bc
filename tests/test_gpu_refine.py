"""sgtd_refine_poses on the device against the numpy restatement of the rule in include/sgtd_accel.h
(tests/_refine_ref.py), fed with what the library hands out: sgtd_result_pairs, sgtd_result_inliers, sgtd_fetch_entries,
sgtd_result_query_descs and sgtd_result_verify.

What is compared how.  n_pairs, the moments (cp, cw, H) and rmse_verify are sums in a fixed order: bit for bit.  The
rotation comes from the device's one-sided Jacobi SVD and from numpy.linalg.svd: to rounding (max |dR| <= 1e-9,
|dt| <= 1e-9 (1 + |cp| + |cw|), the gate SURVEY.md §8f row 1 set for the verify solver), candidates with collinear
inliers (second singular value of H below 1e-6 of the first) left out of that comparison alone and at most 1 % of the
verified ones.  rmse is a sum in the fixed order of residuals under the refined pose; since that pose agrees between
the two SVDs to rounding only, its bits are checked against the restatement's residual sum evaluated at the pose the
device returned (and its value against the restatement's own pose to 1e-9).

The world (300 frames 12 m apart, 96 queries, candidate_num 50) was checked on the CPU with OracleManager.verify and
the restatement before it was chosen: 2585 verified candidates, none collinear, inlier sets of 4 to 4374 pairs, about
half of them above the 896 pairs the kernel keeps in LDS (both of its paths run), 4800 workgroups (the frame-ordered
dispatch).  The median translation error of SearchLoop's choice fell from 0.38 m to 0.006 m there (test 7's expectation,
also 0.36 m -> 0.006 m on a map 2 m apart)."""
import ctypes

import numpy as np
import pytest

import _refine_ref as rr
import _verify_edges as ve

pytestmark = pytest.mark.gpu

F, NQ, SPACING = 300, 96, 12.0
TOL = 1e-9


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from sgtd_amd import _lib, evaluate, manager, synth
    return oracle, manager, synth, _lib, evaluate


@pytest.fixture(scope="module")
def world(mods):
    _, _, synth, _, ev = mods
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


def _expected(g, res, q, iterations):
    """the restatement for every verified candidate of query q -> {k: result}, fed with the library's own outputs"""
    qi, de = g.result_pairs(q, res)
    score, rot, t = g.result_verify(q)
    out = {}
    if not len(de):
        return out, score
    qd, ent = g.result_query_descs(q), g.fetch_entries(de)
    for k in range(int(res.n_cand[q])):
        if score[k] < 0:
            continue
        lo, hi = int(res.pair_off[q, k]), int(res.pair_off[q, k + 1])
        s0 = np.zeros(hi - lo, bool)
        s0[g.result_inliers(q, k, hi - lo)] = True
        p, w = rr.correspondences(qd.vertex, qi[lo:hi], ent.vertex[lo:hi])
        out[k] = dict(rr.refine(p, w, s0, iterations, rot[k], t[k]), p=p, w=w, score=score[k])
    return out, score


def _compare(got, exp, cn, where, stats):
    """got: STDescManager.result_refined's dict; exp: _expected's"""
    for k in range(cn):
        if k not in exp:
            assert not got["rot"][k].any() and not got["t"][k].any(), (where, k)
            assert np.isnan(got["rmse"][k]) and np.isnan(got["rmse_verify"][k]) and np.isnan(got["moments"][k]).all(), (where, k)
            assert got["n_pairs"][k] == 0, (where, k)
            continue
        e = exp[k]
        R, t = got["rot"][k], got["t"][k]
        assert got["n_pairs"][k] == e["n_pairs"], (where, k)
        assert np.array_equal(_bits(got["moments"][k]), _bits(e["moments"])), (where, k)
        assert np.array_equal(_bits(got["rmse_verify"][k]), _bits(e["rmse_verify"])), (where, k)
        assert np.array_equal(_bits(got["rmse"][k]), _bits(rr.rmse(R, t, e["p"], e["w"], e["set"]))), (where, k)
        assert abs(got["rmse"][k] - e["rmse"]) <= TOL * (1 + e["rmse"]), (where, k)
        # a rotation, whatever the inliers' geometry
        assert np.abs(R.T @ R - np.eye(3)).sum(axis=1).max() <= 1e-12 and np.linalg.det(R) > 0, (where, k)
        stats["verified"] += 1
        stats["lds"] += e["n_pairs"] <= 896
        stats["stop_" + str(e["stop"])] = stats.get("stop_" + str(e["stop"]), 0) + 1
        if rr.collinear(e["H"]):
            stats["collinear"] += 1
            continue
        assert np.abs(R - e["rot"]).max() <= TOL, (where, k)
        assert np.abs(t - e["t"]).max() <= TOL * (1 + np.linalg.norm(e["cp"]) + np.linalg.norm(e["cw"])), (where, k)


def _stats():
    return {"verified": 0, "collinear": 0, "lds": 0}


def _snapshot(g, res, nq):
    """everything sgtd_refine_poses must leave alone, as bit patterns"""
    L, cn = g._L, g.config_setting_["candidate_num"]
    out = [np.concatenate([np.asarray(x).astype(np.float64) for x in g.search_loop(0.4)])]
    for q in range(nq):
        score, rot, t = g.result_verify(q)
        out += [score, rot.ravel(), t.ravel(), g.result_world_poses(q).astype(np.float64).ravel()]
        cap = int(res.pair_off[q, cn])
        off, qi, de = np.zeros(cn + 1, np.int64), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int64)
        n = ctypes.c_int64(0)
        assert L.sgtd_result_inlier_pairs(g._h, q, off.ctypes.data, qi.ctypes.data, de.ctypes.data, cap, ctypes.byref(n)) == 0
        out += [off.astype(np.float64), qi[:n.value].astype(np.float64), de[:n.value].astype(np.float64)]
        for k in range(int(res.n_cand[q])):
            if score[k] >= 0:
                out.append(g.result_inliers(q, k, int(res.pair_off[q, k + 1] - res.pair_off[q, k])).astype(np.float64))
    return [_bits(x) for x in out]


def _same_refined(a, b, where=None):
    for key in ("rot", "t", "rmse", "rmse_verify", "moments"):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), (where, key)
    assert np.array_equal(a["n_pairs"], b["n_pairs"]), where


@pytest.fixture(scope="module")
def batch(mods, world):
    """one handle, the batch verified once; tests refine it again and again (the call is repeatable)"""
    _, manager, _, _, _ = mods
    m, qs, rows = world
    g = _new(manager, m, rows)
    res = g.query_frames(qs.xyz, qs.label)
    g.verify()
    yield g, res
    g.close()


def test_moments_pose_and_least_squares_one_iteration(batch):
    """tests 1-3 and 5: sums to the bit, the pose to rounding, rmse <= rmse_verify, and nothing else moves"""
    g, res = batch
    cn = g.config_setting_["candidate_num"]
    before = _snapshot(g, res, NQ)
    g.refine_poses(1)
    after = _snapshot(g, res, NQ)
    assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))
    st = _stats()
    for q in range(NQ):
        got = g.result_refined(q)
        exp, score = _expected(g, res, q, 1)
        _compare(got, exp, cn, q, st)
        for k, e in exp.items():
            assert got["n_pairs"][k] == score[k], (q, k)
            assert got["rmse"][k] <= got["rmse_verify"][k] * (1 + 1e-12), (q, k)
    print("one iteration:", st)
    assert st["verified"] >= 1000 and st["collinear"] <= 0.01 * st["verified"]
    assert st["lds"] >= 100 and st["verified"] - st["lds"] >= 100      # both of the kernel's paths ran


def test_three_iterations(batch):
    """test 4: three rounds equal the restatement's; sgtd_result_inliers still returns sgtd_verify's set"""
    g, res = batch
    cn = g.config_setting_["candidate_num"]
    before = _snapshot(g, res, NQ)
    g.refine_poses(3)
    after = _snapshot(g, res, NQ)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    st = _stats()
    grew = 0
    for q in range(0, NQ, 2):
        got = g.result_refined(q)
        exp, _ = _expected(g, res, q, 3)
        _compare(got, exp, cn, q, st)
        grew += sum(e["n_pairs"] > e["score"] for e in exp.values())
    print("three iterations:", st, "sets that grew:", grew)
    # (on this world sgtd_verify's set already holds every pair within 3 m of the refined pose: the CPU check found every
    # candidate stopping on an unchanged set; sets that change are test_stop_rules_on_constructed_candidates' business)
    assert st["verified"] >= 500 and st["collinear"] <= 0.01 * st["verified"]


def _few_scenario():
    """verify accepts four pairs (all within 3 m of pair 0's motion, the identity); their least-squares motion leaves
    pair 1 more than 3 m off: the second set has three pairs and the loop stops"""
    rng = np.random.default_rng(7)
    qv = np.stack([ve.f32(ve._triangle(rng, rng.uniform(-15, 15, 3))) for _ in range(6)])
    shift = np.array([[0, 0, 0], [-2.9, 0, 0], [2.9, 0, 0], [2.9, 0, 0], [60.0, 40.0, 0], [-70.0, 10.0, 5.0]])
    return ve.Scenario("few", qv, qv + shift[:, None, :])


def _noisy_scenario(n=300, sigma=0.9):
    """a rigid motion with metres of noise on every table vertex: the three-point pose of the verification is well off,
    its inlier set partial, and the set changes from iteration to iteration as the pose settles"""
    rng = np.random.default_rng(11)
    sc = ve.rigid("noisy/n%d" % n, rng, ve.ROTATIONS["r37"], np.array([4.0, -6.0, 1.5]), n, n_anchor=n, deltas=[0.0], spread=25.0)
    sc.ev = ve.f32(sc.ev + rng.normal(0.0, sigma, sc.ev.shape))
    sc.ec = sc.ev.mean(axis=1)
    return sc


def _scenarios():
    rng = np.random.default_rng(3)
    R, t = ve.ROTATIONS["r37"], np.array([4.0, -6.0, 1.5])
    return [_few_scenario(),
            ve.rigid("same/n40", rng, R, t, 40, n_anchor=40, deltas=[0.0]),
            ve.rigid("same/n1000", rng, R, t, 1000, n_anchor=1000, deltas=[0.0], spread=4.0),
            ve.rigid("probes/n65", rng, R, t, 65, n_anchor=6),
            _noisy_scenario(300), _noisy_scenario(2000, 1.1)]


def test_stop_rules_on_constructed_candidates(mods):
    """test 4's stop rules: a set of fewer than 4 pairs, an unchanged set — each on a candidate built for it, and lists
    below and above the kernel's LDS capacity"""
    _, manager, _, _, _ = mods
    scen = _scenarios()
    wl = ve.Workload(scen)
    g = manager.STDescManager()
    wl.load(g, manager)
    g.finalize()
    res = g.candidate_selector(wl.query_descs(manager, 0))
    batch_res = g.results()
    g.verify()
    cn = g.config_setting_["candidate_num"]
    assert int(batch_res.n_cand[0]) == len(scen)
    stops = {}
    for it in (1, 2, 3, 6):
        g.refine_poses(it)
        got = g.result_refined(0)
        exp, _ = _expected(g, batch_res, 0, it)
        assert len(exp) == len(scen)
        st = _stats()
        _compare(got, exp, cn, it, st)
        for k, e in exp.items():
            stops[(scen[int(batch_res.cand_frame[0, k])].tag, it)] = (e["stop"], e["n_pairs"], e["fits"])
    assert stops[("few", 1)] == (None, 4, 1) and stops[("few", 3)] == ("few", 4, 1)
    assert stops[("same/n40", 3)] == ("same", 40, 1) and stops[("same/n1000", 2)] == ("same", 1000, 1)
    # sets that change: they grow as the pose settles, then stop on an unchanged set after a third fit
    for tag in ("noisy/n300", "noisy/n2000"):
        assert stops[(tag, 1)][1] < stops[(tag, 2)][1] and stops[(tag, 2)][2] == 2 and stops[(tag, 3)][2] == 3, tag
    assert stops[("noisy/n300", 6)][0] == "same" and stops[("noisy/n300", 6)][2] == 3
    assert stops[("noisy/n2000", 1)][1] > 896 and stops[("noisy/n300", 3)][1] < 896      # beyond and within the LDS image
    assert res is not None
    g.close()


def test_states_and_invalidation(mods, world):
    """test 6: call order, invalidation by a new verification and by a new batch, q outside the batch"""
    _, manager, _, _lib, _ = mods
    m, qs, rows = world
    g = _new(manager, m, rows)

    def status(call, *a):
        with pytest.raises(_lib.SgtdError) as ei:
            call(*a)
        return ei.value.status

    assert status(g.refine_poses) == -7                      # no batch
    res = g.query_frames(qs.xyz[:8], qs.label[:8])
    assert status(g.refine_poses) == -7                      # no verification yet
    g.verify()
    assert status(g.result_refined, 0) == -7                 # results before sgtd_refine_poses
    assert status(g.result_refined_world_poses, 0) == -7
    g.refine_poses(2)
    a = g.result_refined(3)
    assert status(g.result_refined, 8) == -1 and g._L.sgtd_result_refined(g._h, -1, None, None, None, None, None) == -1
    assert g._L.sgtd_refine_poses(g._h, 0) == -1
    _same_refined(a, g.result_refined(3))                    # (a bad call changes nothing)
    g.verify()                                               # a new verification drops the refined results
    assert status(g.result_refined, 3) == -7
    g.refine_poses(2)
    _same_refined(a, g.result_refined(3))
    g.query_frames(qs.xyz[:8], qs.label[:8])                 # so does a new batch
    assert status(g.result_refined, 3) == -7 and status(g.refine_poses) == -7
    g.verify()
    g.refine_poses(2)
    _same_refined(a, g.result_refined(3))
    assert res is not None
    g.close()


def test_search_frame_masked_view(mods, world):
    """test 6: after sgtd_search_frame (flags 0) the refit equals the batch path's; sgtd_verify_masked's masked
    candidates have no result; a view refines independently of its owner"""
    import torch
    _, manager, _, _, _ = mods
    m, qs, rows = world
    g = _new(manager, m, rows)
    nq = 6
    res = g.query_frames(qs.xyz[:nq], qs.label[:nq])
    g.verify()
    g.refine_poses(2)
    full = [g.result_refined(q) for q in range(nq)]
    world_full = [g.result_refined_world_poses(q) for q in range(nq)]
    assert sum(int((f["n_pairs"] > 0).sum()) for f in full) >= 50
    # the one-frame call
    for q in (0, 3):
        d = g.BuildSingleScanSTD(qs.xyz[q], qs.label[q])
        r = g.search_frame(d, capacity=1 << 17)
        assert r["status"] == 0
        g.refine_poses(2)
        _same_refined(full[q], g.result_refined(0), q)
        assert np.array_equal(world_full[q].view(np.uint32), g.result_refined_world_poses(0).view(np.uint32))
    # masked verification: every second candidate
    res = g.query_frames(qs.xyz[:nq], qs.label[:nq])
    mask = 0x5555555555555555
    keep = torch.full((nq,), mask, dtype=torch.int64, device="cuda")
    g.verify_masked(keep)
    torch.cuda.synchronize()
    g.refine_poses(2)
    for q in range(nq):
        r = g.result_refined(q)
        wp = g.result_refined_world_poses(q)
        for k in range(g.config_setting_["candidate_num"]):
            if (mask >> k) & 1:
                for key in ("rot", "t", "rmse", "rmse_verify", "moments"):
                    assert np.array_equal(_bits(r[key][k]), _bits(full[q][key][k])), (q, k, key)
                assert r["n_pairs"][k] == full[q]["n_pairs"][k]
                assert np.array_equal(wp[k].view(np.uint32), world_full[q][k].view(np.uint32))
            else:
                assert r["n_pairs"][k] == 0 and np.isnan(r["rmse"][k]) and np.isnan(r["moments"][k]).all() and not r["rot"][k].any()
                assert np.isnan(wp[k]).all()
    # a view: its own batch, its own refined results; the owner's stay
    g.query_frames(qs.xyz[:nq], qs.label[:nq])
    g.verify()
    g.refine_poses(2)
    v = manager.STDescManager()
    v.attach_table(g)
    v.set_frame_poses(np.arange(F), rows)
    v.query_frames(qs.xyz[nq:2 * nq], qs.label[nq:2 * nq])
    v.verify()
    from sgtd_amd import _lib
    with pytest.raises(_lib.SgtdError) as ei:
        v.result_refined(0)
    assert ei.value.status == -7                             # (the owner's refinement is not the view's)
    v.refine_poses(1)
    mine = [v.result_refined(q) for q in range(nq)]
    for q in range(nq):
        _same_refined(full[q], g.result_refined(q), q)
    g.query_frames(qs.xyz[nq:2 * nq], qs.label[nq:2 * nq])
    g.verify()
    g.refine_poses(1)
    for q in range(nq):
        _same_refined(mine[q], g.result_refined(q), q)
        _same_refined(mine[q], v.result_refined(q), q)
    # the owner's table changes: the view's calls return SGTD_ERR_STATE until it is attached again
    g.add_frames(m.xyz[:1], m.label[:1])
    with pytest.raises(_lib.SgtdError) as ei:
        v.refine_poses(1)
    assert ei.value.status == -7
    v.close()
    g.close()
    assert res is not None


def test_three_shard_handle(mods, world):
    """test 6: three shards on the one GPU give the single handle's refined poses, moments and world poses bit for bit"""
    _, manager, _, _, _ = mods
    m, qs, rows = world
    nq = 24
    single, multi = _new(manager, m, rows), _new(manager, m, rows, devices=[0, 0, 0])
    a, b = single.query_frames(qs.xyz[:nq], qs.label[:nq]), multi.query_frames(qs.xyz[:nq], qs.label[:nq])
    assert np.array_equal(a.cand_frame, b.cand_frame) and np.array_equal(a.n_cand, b.n_cand)
    from sgtd_amd import _lib
    for h in (single, multi):
        h.verify()
        with pytest.raises(_lib.SgtdError) as ei:
            h.result_refined(0)
        assert ei.value.status == -7
        h.refine_poses(3)
    n = 0
    for q in range(nq):
        ra, rb = single.result_refined(q), multi.result_refined(q)
        _same_refined(ra, rb, q)
        wa, wb = single.result_refined_world_poses(q), multi.result_refined_world_poses(q)
        assert np.array_equal(wa.view(np.uint32), wb.view(np.uint32)), q
        n += int((ra["n_pairs"] > 0).sum())
        assert np.array_equal(np.isnan(wa[:, 0]), ra["n_pairs"] == 0)
    assert n >= 200
    for h in (single, multi):
        h.close()


def test_it_helps(mods):
    """test 7: 256 queries at synth.make_queries' default noise; the median translation error of SearchLoop's choice
    with the refined world pose is no larger than with sgtd_verify's"""
    _, manager, synth, _, ev = mods
    m = synth.make_map(400, 200, stream=421)
    qs = synth.make_queries(m, 256, stream=422)
    rows = np.stack([ev.pose_row(*p) for p in m.pose])
    g = _new(manager, m, rows)
    g.query_frames(qs.xyz, qs.label)
    g.verify()
    bc, bf, _ = g.search_loop()
    g.refine_poses(1)
    err = {"verify": [], "refined": []}
    for q in range(256):
        if bf[q] < 0:
            continue
        gt = ev.pose_matrix(*qs.pose[q])
        for name, w in (("verify", g.result_world_poses(q)), ("refined", g.result_refined_world_poses(q))):
            err[name].append(ev.compute_adj_rpe(gt, ev.matrix_from_row(w[int(bc[q])])))
    tv, tr = np.median([e[0] for e in err["verify"]]), np.median([e[0] for e in err["refined"]])
    rv, rf = np.median([e[1] for e in err["verify"]]), np.median([e[1] for e in err["refined"]])
    print("loops %d  median translation error: verify %.6f m, refined %.6f m; rotation: verify %.6f deg, refined %.6f deg"
          % (len(err["verify"]), tv, tr, rv, rf))
    assert len(err["verify"]) >= 200
    assert tr <= tv
    # evaluate_batch(refine=1) accounts the same refined poses; refine=0 is today's accounting
    m0 = ev.evaluate_batch(g, np.stack([ev.matrix_from_row(r) for r in rows]), qs.xyz, qs.label,
                           np.stack([ev.pose_matrix(*p) for p in qs.pose]))
    m1 = ev.evaluate_batch(g, np.stack([ev.matrix_from_row(r) for r in rows]), qs.xyz, qs.label,
                           np.stack([ev.pose_matrix(*p) for p in qs.pose]), refine=1)
    assert m0.detected == m1.detected and np.array_equal(m0.STD_num, m1.STD_num)
    assert np.median(m1.t_errors) <= np.median(m0.t_errors)
    g.close()
