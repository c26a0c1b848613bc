"""sgtd_overlap on the device against the numpy restatement of the rule in include/sgtd_accel.h (tests/_overlap_ref.py),
fed with the poses the library returned (sgtd_result_verify, sgtd_result_refined).  Every output of every candidate is
compared: the four counts as integers, overlap and rms as bit patterns (NaN = NaN).

The world is tests/test_gpu_refine.py's (300 frames 12 m apart, 200 keypoints, 96 queries, candidate_num 50: 4800
workgroups, so the frame-ordered dispatch runs).  Checked on the CPU with OracleManager.verify and the restatement
before the queries were fixed (radius 1.0): test_it_discriminates' docstring has the figures."""
import numpy as np
import pytest

import _overlap_ref as ov

pytestmark = pytest.mark.gpu

F, NQ, SPACING = 300, 96, 12.0
TILE = 1024          # SGTD_OVERLAP_TILE


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
    g.add_frames(m.xyz, m.label, keep_keypoints=True)
    g.finalize()
    g.set_frame_poses(np.arange(len(rows)), rows)
    return g


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _status(_lib, call, *a, **kw):
    with pytest.raises(_lib.SgtdError) as ei:
        call(*a, **kw)
    return ei.value.status


def _poses(g, q, refined):
    score, rot, t = g.result_verify(q)
    if refined:
        r = g.result_refined(q)
        rot, t = r["rot"], r["t"]
    return score, rot, t


def _check_query(g, res, q, radius, refined, q_xyz, q_label, frame_kp, where, tally=None):
    """every output of every candidate of query q against the restatement; frame_kp(f) -> (xyz, label) or (None, None)"""
    cn = g.config_setting_["candidate_num"]
    got = g.result_overlap(q)
    score, rot, t = _poses(g, q, refined)
    for k in range(cn):
        if k >= int(res.n_cand[q]) or not score[k] >= 0:
            exp = ov.NO_RESULT
        else:
            fx, fl = frame_kp(int(res.cand_frame[q, k]))
            exp = ov.overlap(rot[k], t[k], q_xyz, q_label, fx, fl, radius)
            if tally is not None:
                tally.append(exp)
        for key in ov.KEYS:
            assert ov.same_value(exp[key], got[key][k]), (where, q, k, key, exp[key], got[key][k])
    return got


def _same_overlap(a, b, where=None):
    for key in ov.KEYS[:4]:
        assert np.array_equal(a[key], b[key]), (where, key)
    for key in ov.KEYS[4:]:
        assert np.array_equal(_bits(a[key]), _bits(b[key])), (where, key)


@pytest.fixture(scope="module")
def batch(mods, world):
    """one handle, the batch verified and refitted once; tests run the overlap pass again and again (it is repeatable)"""
    manager, _, _, _ = mods
    m, qs, rows = world
    g = _new(manager, m, rows)
    res = g.query_frames(qs.xyz, qs.label)
    g.verify()
    g.refine_poses(1)
    yield g, res
    g.close()


@pytest.mark.parametrize("radius, refined", [(0.5, False), (1.0, False), (0.5, True), (1.0, True)])
def test_parity_bit_for_bit(batch, world, radius, refined):
    """test 1: the batch's own keypoints, both radii, both poses; 4800 workgroups in candidate-frame order"""
    g, res = batch
    m, qs, _ = world
    assert NQ * g.config_setting_["candidate_num"] >= 4096
    g.overlap(radius, refined=refined)
    tally = []
    for q in range(NQ):
        _check_query(g, res, q, radius, refined, qs.xyz[q], qs.label[q], lambda f: (m.xyz[f], m.label[f]), (radius, refined), tally)
    hits = np.array([e["n_hit_query"] for e in tally])
    print("radius %.1f refined %d: %d verified candidates, hits median %d, range %d..%d" % (radius, refined, len(tally), np.median(hits),
                                                                                            hits.min(), hits.max()))
    assert len(tally) >= 1000 and hits.max() >= 150 and hits.min() < 50
    if (radius, refined) == (1.0, False):      # (the CPU check found 9 candidates whose two hit counts differ)
        assert any(e["n_hit_frame"] != e["n_hit_query"] for e in tally)


def _snapshot(g, res, nq):
    """everything sgtd_verify and sgtd_refine_poses hand out, as bit patterns"""
    out = [np.concatenate([np.asarray(x).astype(np.float64) for x in g.search_loop(0.4)])]
    for q in range(nq):
        score, rot, t = g.result_verify(q)
        r = g.result_refined(q)
        out += [score, rot.ravel(), t.ravel(), g.result_world_poses(q).astype(np.float64).ravel(),
                g.result_refined_world_poses(q).astype(np.float64).ravel(), r["rot"].ravel(), r["t"].ravel(), r["rmse"], r["rmse_verify"],
                r["moments"].ravel(), r["n_pairs"].astype(np.float64)]
        for k in range(int(res.n_cand[q])):
            if score[k] >= 0:
                out.append(g.result_inliers(q, k, int(res.pair_off[q, k + 1] - res.pair_off[q, k])).astype(np.float64))
    return [_bits(x) for x in out]


def _constructed_frames(rng, ids):
    """keypoint sets by frame id mod 6: none stored, 0 keypoints, 1 keypoint, exactly one tile, one tile plus one, and a
    set whose labels the queries do not have -> {id: (xyz, label) or (None, None)}"""
    out = {}
    for f in ids:
        kind = f % 6
        n = (0, 0, 1, TILE, TILE + 1, 300)[kind]
        xyz = np.stack([rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), rng.uniform(-2, 2, n)], axis=1).astype(np.float32)
        lab = rng.integers(0, 2, n).astype(np.uint32) + (np.uint32(1000) if kind == 5 else np.uint32(0))
        out[int(f)] = (None, None) if kind == 0 else (xyz, lab)
    return out


def test_edges_on_constructed_frames(mods, world):
    """test 2: query frames of 0, 1, 255, 256, 257 and 600 keypoints given explicitly, against map frames of 0 keypoints,
    1 keypoint, one tile, one tile plus one, foreign labels and no stored keypoints; radius 0; two radii one ulp apart
    around an observed m_i; a NaN query coordinate"""
    manager, _, _, _ = mods
    m, qs, rows = world
    rng = np.random.default_rng(2)
    sizes = [0, 1, 255, 256, 257, 600]
    nq = len(sizes)
    g = _new(manager, m, rows)
    frames = _constructed_frames(rng, range(F))
    g.set_frame_keypoints(None, None)                              # (forget what add_frames kept)
    ids = [f for f in range(F) if frames[f][0] is not None]
    off = np.concatenate([[0], np.cumsum([len(frames[f][1]) for f in ids])])
    g.set_frame_keypoints(ids, np.concatenate([frames[f][0] for f in ids]), np.concatenate([frames[f][1] for f in ids]), off)
    res = g.query_frames(qs.xyz[:nq], qs.label[:nq])
    g.verify()
    q_off = np.concatenate([[0], np.cumsum(sizes)])
    n_all = int(q_off[-1])
    q_xyz = np.stack([rng.uniform(-30, 30, n_all), rng.uniform(-30, 30, n_all), rng.uniform(-2, 2, n_all)], axis=1).astype(np.float32)
    q_lab = rng.integers(0, 2, n_all).astype(np.uint32)
    q_xyz[q_off[5] + 300, 1] = np.nan                               # a NaN coordinate in the 600-keypoint query
    part = lambda a, q: a[q_off[q]:q_off[q + 1]]
    kinds = set()
    for radius in (2.0, 0.0):
        g.overlap(radius, xyz=q_xyz, label=q_lab, kp_off=q_off)
        tally = []
        for q in range(nq):
            got = _check_query(g, res, q, radius, False, part(q_xyz, q), part(q_lab, q), lambda f: frames[f], radius, tally)
            score = g.result_verify(q)[0]
            kinds |= {(sizes[q], int(res.cand_frame[q, k]) % 6) for k in range(int(res.n_cand[q])) if score[k] >= 0}
            assert (got["n_query_kp"][score >= 0] == sizes[q]).all()
        hits = sum(e["n_hit_query"] for e in tally)
        print("constructed frames, radius %.1f: %d candidates, %d query hits" % (radius, len(tally), hits))
        assert (hits > 0) if radius else (hits == 0)
    # every query size met every kind of frame (CPU-side count of what the device was asked)
    assert {k for _, k in kinds} == set(range(6)) and {s for s, _ in kinds} == set(sizes), sorted(kinds)
    # the NaN keypoint never hits, whatever the radius
    score, rot, t = g.result_verify(5)
    k5 = [k for k in range(int(res.n_cand[5])) if score[k] >= 0 and int(res.cand_frame[5, k]) % 6 in (3, 4)]
    assert k5
    part5 = (part(q_xyz, 5), part(q_lab, 5))
    at2 = {k: ov.overlap(rot[k], t[k], *part5, *frames[int(res.cand_frame[5, k])], 2.0) for k in k5}
    k = max(k5, key=lambda c: at2[c]["n_hit_query"])               # the long-frame candidate with the most hits
    e = at2[k]
    assert e["n_hit_query"] >= 1
    big = ov.overlap(rot[k], t[k], *part5, *frames[int(res.cand_frame[5, k])], 1e6)
    assert big["n_hit_query"] == 599 and not big["hit_query"][300]
    g.overlap(1e6, xyz=q_xyz, label=q_lab, kp_off=q_off)
    assert g.result_overlap(5)["n_hit_query"][k] == 599
    # two radii one ulp apart around an observed m_i: the count moves by exactly that keypoint
    hit_m = np.sort(e["m"][e["hit_query"]])
    mi = hit_m[len(hit_m) // 2]
    r0 = np.sqrt(mi)
    while r0 * r0 >= mi:
        r0 = np.nextafter(r0, 0.0)
    while np.nextafter(r0, np.inf) ** 2 < mi:
        r0 = np.nextafter(r0, np.inf)
    r1 = np.nextafter(r0, np.inf)
    assert r0 * r0 < mi <= r1 * r1
    counts = []
    for radius in (r0, r1):
        g.overlap(float(radius), xyz=q_xyz, label=q_lab, kp_off=q_off)
        got = _check_query(g, res, 5, radius, False, part(q_xyz, 5), part(q_lab, 5), lambda f: frames[f], ("ulp", radius))
        counts.append(int(got["n_hit_query"][k]))
    assert counts[1] - counts[0] == int(np.count_nonzero((e["m"] > r0 * r0) & (e["m"] <= r1 * r1))) >= 1
    assert counts[1] - counts[0] == 1
    g.close()


def test_states_and_invalidation(mods, world, batch):
    """test 3: call order, the refined flag before a refit, a batch without keypoints, invalidation, replacement, and
    nothing sgtd_verify / sgtd_refine_poses hand out moves"""
    manager, _, _lib, _ = mods
    m, qs, rows = world
    g = _new(manager, m, rows)
    st = lambda call, *a, **kw: _status(_lib, call, *a, **kw)
    assert st(g.overlap, 1.0) == -7                                 # no batch
    res = g.query_frames(qs.xyz[:8], qs.label[:8])
    assert st(g.overlap, 1.0) == -7                                 # no verification yet
    assert st(g.search_loop_overlap, 0.4) == -7
    g.verify()
    assert st(g.result_overlap, 0) == -7                            # results before sgtd_overlap
    assert st(g.overlap, 1.0, refined=True) == -7                   # the refined pose before a refit
    assert st(g.search_loop_overlap, 0.4) == -7
    bc, bf, bs, bo = g.search_loop_overlap(0.0)                     # no gate: no overlap results needed
    assert np.isnan(bo).all() and np.array_equal(bc, g.search_loop()[0])
    g.refine_poses(1)
    before = _snapshot(g, res, 8)
    g.overlap(1.0)
    a = g.result_overlap(3)
    g.overlap(1.0, refined=True)
    b = g.result_overlap(3)
    assert not np.array_equal(_bits(a["rms"]), _bits(b["rms"]))     # a later call replaces the results
    g.overlap(0.5)
    c = g.result_overlap(3)
    assert (c["n_hit_query"] <= a["n_hit_query"]).all() and (c["n_hit_query"] < a["n_hit_query"]).any()
    g.overlap(1.0)
    _same_overlap(a, g.result_overlap(3))
    after = _snapshot(g, res, 8)
    assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after))
    assert st(g.result_overlap, 8) == -1 and g._L.sgtd_result_overlap(g._h, -1, None, None, None, None, None, None) == -1
    for bad in (float("nan"), -1.0, float("inf")):
        assert g._L.sgtd_overlap(g._h, bad, 0, None, None, None) == -1
    assert g._L.sgtd_overlap(g._h, 1.0, 2, None, None, None) == -1
    assert g._L.sgtd_overlap(g._h, 1.0, 0, qs.xyz.ctypes.data, None, None) == -1
    big = np.array([0, 70000] + [70000] * 7, np.int64)
    assert g._L.sgtd_overlap(g._h, 1.0, 0, qs.xyz.ctypes.data, qs.label.ctypes.data, big.ctypes.data) == -1
    _same_overlap(a, g.result_overlap(3))                           # (a bad call changes nothing)
    g.verify()                                                      # a new verification drops the results
    assert st(g.result_overlap, 3) == -7 and st(g.search_loop_overlap, 0.4) == -7
    g.overlap(1.0)
    _same_overlap(a, g.result_overlap(3))
    g.query_frames(qs.xyz[:8], qs.label[:8])                        # so does a new batch
    assert st(g.result_overlap, 3) == -7 and st(g.overlap, 1.0) == -7
    # a batch of descriptors has no keypoints of its own
    d = g.BuildSingleScanSTD(qs.xyz[3], qs.label[3])
    g.candidate_selector(d)
    g.verify()
    assert st(g.overlap, 1.0) == -7
    g.overlap(1.0, xyz=qs.xyz[3:4], label=qs.label[3:4])
    _same_overlap(a, g.result_overlap(0))
    # the store: errors, forgetting, overwriting
    ids = np.arange(2, dtype=np.uint32)
    assert g._L.sgtd_set_frame_keypoints(g._h, ids.ctypes.data, big.ctypes.data, qs.xyz.ctypes.data, qs.label.ctypes.data, 1) == -1
    far = np.array([g.config_setting_["max_frame_n"]], np.uint32)
    off1 = np.array([0, 1], np.int64)
    assert g._L.sgtd_set_frame_keypoints(g._h, far.ctypes.data, off1.ctypes.data, qs.xyz.ctypes.data, qs.label.ctypes.data, 1) == -5
    g.overlap(1.0, xyz=qs.xyz[3:4], label=qs.label[3:4])
    _same_overlap(a, g.result_overlap(0))
    score = g.result_verify(0)[0]
    k = int(np.argmax(score))
    f = int(g.results().cand_frame[0, k])
    g.set_frame_keypoints([f], None)                                # forget one frame
    g.overlap(1.0, xyz=qs.xyz[3:4], label=qs.label[3:4])
    r = g.result_overlap(0)
    assert r["n_frame_kp"][k] == -1 and r["n_hit_query"][k] == 0 and np.isnan(r["overlap"][k]) and r["n_query_kp"][k] == 200
    g.set_frame_keypoints([f], m.xyz[f:f + 1], m.label[f:f + 1])    # and store it again
    g.overlap(1.0, xyz=qs.xyz[3:4], label=qs.label[3:4])
    _same_overlap(a, g.result_overlap(0))
    g.set_frame_keypoints(None, None)                               # forget all
    g.overlap(1.0, xyz=qs.xyz[3:4], label=qs.label[3:4])
    r = g.result_overlap(0)
    assert (r["n_frame_kp"] == -1).all() and (r["n_hit_query"][score >= 0] == 0).all()
    g.close()


def test_search_frame_masked_view_loop(mods, world):
    """test 4: a sgtd_search_frame batch with explicit keypoints, sgtd_verify_masked, a view, a sgtd_loop_frames batch"""
    import torch
    manager, _, _lib, _ = mods
    m, qs, rows = world
    g = _new(manager, m, rows)
    nq, cn = 6, g.config_setting_["candidate_num"]
    frame_kp = lambda f: (m.xyz[f], m.label[f])
    res = g.query_frames(qs.xyz[:nq], qs.label[:nq])
    g.verify()
    g.overlap(1.0)
    full = [_check_query(g, res, q, 1.0, False, qs.xyz[q], qs.label[q], frame_kp, "full") for q in range(nq)]
    assert sum(int((f["n_frame_kp"] > 0).sum()) for f in full) >= 50
    for q in (0, 3):                                                # the one-frame call
        d = g.BuildSingleScanSTD(qs.xyz[q], qs.label[q])
        assert g.search_frame(d, capacity=1 << 17)["status"] == 0
        assert _status(_lib, g.overlap, 1.0) == -7
        g.overlap(1.0, xyz=qs.xyz[q:q + 1], label=qs.label[q:q + 1])
        _same_overlap(full[q], g.result_overlap(0), q)
    res = g.query_frames(qs.xyz[:nq], qs.label[:nq])                # masked verification: every second candidate
    mask = 0x5555555555555555
    keep = torch.full((nq,), mask, dtype=torch.int64, device="cuda")
    g.verify_masked(keep)
    torch.cuda.synchronize()
    g.overlap(1.0)
    for q in range(nq):
        r = g.result_overlap(q)
        for k in range(cn):
            for key in ov.KEYS:
                want = full[q][key][k] if (mask >> k) & 1 else ov.NO_RESULT[key]
                assert ov.same_value(want, r[key][k]), (q, k, key)
    # a view: its own store, its own results
    g.query_frames(qs.xyz[:nq], qs.label[:nq])
    g.verify()
    g.overlap(1.0)
    v = manager.STDescManager()
    v.attach_table(g)
    res_v = v.query_frames(qs.xyz[nq:2 * nq], qs.label[nq:2 * nq])
    v.verify()
    assert _status(_lib, v.result_overlap, 0) == -7                 # (the owner's pass is not the view's)
    v.overlap(1.0)                                                  # the view has no keypoints stored
    for q in range(nq):
        r, score = v.result_overlap(q), v.result_verify(q)[0]
        assert (r["n_frame_kp"][score >= 0] == -1).all() and (r["n_query_kp"][score >= 0] == 200).all()
    v.set_frame_keypoints(np.arange(F), m.xyz, m.label)
    v.overlap(1.0)
    for q in range(nq):
        _check_query(v, res_v, q, 1.0, False, qs.xyz[nq + q], qs.label[nq + q], frame_kp, "view")
        _same_overlap(full[q], g.result_overlap(q), q)
    g.add_frames(m.xyz[:1], m.label[:1])                            # the owner's table changes
    assert _status(_lib, v.overlap, 1.0) == -7
    v.close()
    g.close()
    # sequence loop detection: every frame against the frames before it
    g = manager.STDescManager()
    n = 48
    res = g.loop_frames(m.xyz[:n], m.label[:n], batch=n)
    g.set_frame_keypoints(np.arange(n), m.xyz[:n], m.label[:n])
    g.verify()
    g.overlap(1.0)
    tally = []
    for q in range(n):
        _check_query(g, res, q, 1.0, False, m.xyz[q], m.label[q], frame_kp, "loop", tally)
    assert len(tally) >= 20 and max(e["n_hit_query"] for e in tally) > 20
    g.close()


def test_three_shard_handle(mods, world):
    """test 4: three shards on the one GPU give the single handle's results bit for bit, and the same gated choice"""
    manager, _, _lib, _ = mods
    m, qs, rows = world
    nq = 24
    single, multi = _new(manager, m, rows), _new(manager, m, rows, devices=[0, 0, 0])
    a, b = single.query_frames(qs.xyz[:nq], qs.label[:nq]), multi.query_frames(qs.xyz[:nq], qs.label[:nq])
    assert np.array_equal(a.cand_frame, b.cand_frame) and np.array_equal(a.n_cand, b.n_cand)
    for h in (single, multi):
        h.verify()
        assert _status(_lib, h.result_overlap, 0) == -7
        assert _status(_lib, h.overlap, 1.0, refined=True) == -7
        h.refine_poses(1)
    for radius, refined, explicit in ((1.0, False, False), (0.5, True, False), (1.0, True, True)):
        for h in (single, multi):
            if explicit:
                h.overlap(radius, refined=refined, xyz=qs.xyz[:nq], label=qs.label[:nq])
            else:
                h.overlap(radius, refined=refined)
        n = 0
        for q in range(nq):
            ra, rb = single.result_overlap(q), multi.result_overlap(q)
            _same_overlap(ra, rb, (radius, refined, q))
            n += int((ra["n_hit_query"] > 0).sum())
        assert n >= 200
        for gate in (0.0, 0.4):
            for x, y in zip(single.search_loop_overlap(gate), multi.search_loop_overlap(gate)):
                assert np.array_equal(_bits(x), _bits(y)), gate
    for h in (single, multi):
        h.close()


def test_search_loop_overlap(batch, world):
    """test 5: no gate = sgtd_search_loop on every query; a positive gate = the rule applied in numpy to result_overlap"""
    g, res = batch
    g.overlap(1.0)
    bc0, bf0, bs0 = g.search_loop()
    bc, bf, bs, bo = g.search_loop_overlap(0.0)
    assert np.array_equal(bc, bc0) and np.array_equal(bf, bf0) and np.array_equal(_bits(bs), _bits(bs0))
    for gate in (-1.0, 0.25, 0.4, 0.9):
        bc, bf, bs, bo = g.search_loop_overlap(gate, icp_threshold=0.4)
        moved = 0
        for q in range(NQ):
            score = g.result_verify(q)[0]
            o = g.result_overlap(q)["overlap"]
            want = ov.search_loop_overlap(score, o, int(res.n_cand[q]), res.cand_frame[q], 0.4, gate)
            assert (int(bc[q]), int(bf[q])) == want[:2] and ov.same_value(want[2], bs[q]) and ov.same_value(want[3], bo[q]), (gate, q)
            moved += int(bc[q]) != int(bc0[q])
        print("min_overlap %.2f: %d of %d choices differ from sgtd_search_loop's" % (gate, moved, NQ))
        assert (moved == 0) if gate <= 0 else True
    assert (g.search_loop_overlap(0.9)[0] < 0).any()                # a gate nobody passes rejects


def test_it_discriminates(batch, world):
    """test 6, radius 1.0, sgtd_verify's pose: the median n_hit_query of the verified candidates whose frame lies within
    12 m of the query's true position exceeds that of the candidates farther than 40 m, and the verified candidate for
    gt_frame has overlap >= 0.4.
    CPU check of this world with OracleManager.verify and the restatement, all 96 queries, before the set was fixed:
    203 candidates within 12 m with a median of 161 hits of 200, 1738 beyond 40 m with a median of 32; gt_frame is a
    verified candidate of all 96 queries and 93 of them have overlap >= 0.4.  The other three (queries 8, 33 and 67:
    0.32, 0.395 and 0.26) are candidates whose three-point pose is off by a good part of the radius; they are kept in
    the test with the CPU's values, so the set is all 96 queries: 93 at or above 0.4 and these three as found there."""
    g, res = batch
    m, qs, _ = world
    g.overlap(1.0)
    near, far, gt = [], [], []
    for q in range(NQ):
        score = g.result_verify(q)[0]
        r = g.result_overlap(q)
        for k in range(int(res.n_cand[q])):
            if score[k] < 0:
                continue
            f = int(res.cand_frame[q, k])
            d = float(np.hypot(m.pose[f][0] - qs.pose[q][0], m.pose[f][1] - qs.pose[q][1]))
            if d <= 12.0:
                near.append(int(r["n_hit_query"][k]))
            elif d > 40.0:
                far.append(int(r["n_hit_query"][k]))
            if f == int(qs.gt_frame[q]):
                gt.append((q, float(r["overlap"][k])))
    print("within 12 m: %d candidates, median %d hits; beyond 40 m: %d, median %d; gt_frame verified for %d queries, smallest overlap %.3f"
          % (len(near), np.median(near), len(far), np.median(far), len(gt), min(o for _, o in gt)))
    assert len(near) >= 50 and len(far) >= 50
    assert np.median(near) > np.median(far)
    assert len(gt) == NQ
    assert {q: o for q, o in gt if not o >= 0.4} == {8: 0.32, 33: 0.395, 67: 0.26}
