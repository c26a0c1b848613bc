"""The cloud store on the device (sgtd_set_frame_clouds) and the registration against it (sgtd_register_stored,
sgtd_register_stored_loops): the results are those of sgtd_register_clouds on [the call's clouds] + [the named frames' stored
clouds], bit for bit (pose, fitness, costs, counts, iterations, status, every match and d2, the sources' covariances) — against
the numpy restatement (tests/_register_ref.py) and against a direct sgtd_register_clouds call; the pair rows of the loops form
are register_pairs' rule restated in numpy over the verification's results."""
import ctypes as C

import numpy as np
import pytest

import _register_edges as rx
import _register_ref as ref
import _stored_edges as sx

pytestmark = pytest.mark.gpu

EYE = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, evaluate, ingest, manager, synth
    return manager, synth, _lib, evaluate, ingest


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the planted scene ----
def test_planted_scene(mods):
    h = mods[0].STDescManager()
    s, t, Rm, tm = ref.planted_scene(300, 7)
    near = ref.near_start(Rm, tm)
    h.set_frame_clouds([5], [t], k_neighbors=10)
    info = h.frame_clouds_info()
    assert (info["n_frames"], info["n_points"], info["k_neighbors"], info["plane_eps"]) == (1, 400, 10, 1e-3) and info["device_bytes"] >= 400 * 84
    got, _ = sx.check(h, [s], {5: t}, [0, 0], [5, 5], np.array([EYE, near]), "planted", k_neighbors=10, max_corr_dist=2.0)
    assert got["status"].tolist() == [ref.CONVERGED, ref.CONVERGED] and got["n_matched"].tolist() == [300, 300]
    # the stored cloud: the points as given, the restatement's covariances
    sx.same_cloud(h, 5, t, ref.covariances(t.astype(np.float64), 10, 1e-3)[0])
    assert h.frame_cloud(4) is None
    # init None is the identity
    alone = sx.run(h, [s], [0], [5], None, k_neighbors=10, max_corr_dist=2.0)
    assert ref.same(alone["pose"][0], got["pose"][0]) and alone["iterations"][0] == got["iterations"][0]
    h.close()


# ---- a mixed batch ----
def _mixed():
    """several queries against several frames, test_gpu_register.py::_mixed's kinds of pairs: an empty source, a frame
    stored with zero points, a one-point cloud on either side, a NaN coordinate on either side, a target 100 m away,
    clouds of fewer points than k"""
    rng = np.random.default_rng(31)
    s, t, Rm, tm = ref.planted_scene(400, 12)
    cut = lambda base, n: base[rng.permutation(len(base))[:n]].copy()      # noqa: E731
    calls = [cut(s, 260), cut(s, 90), cut(s, 0), cut(s, 1), cut(s, 129), cut(s, 5)]
    calls[4][17, 1] = np.nan
    stored = {2: cut(t, 300), 7: cut(t, 150), 11: cut(t, 0), 13: cut(t, 1), 19: cut(t, 75), 23: cut(t, 6),
              17: (t[:200].astype(np.float64) + [100.0, 0.0, 0.0]).astype(np.float32)}
    stored[19][40, 2] = np.nan
    near = ref.near_start(Rm, tm)
    src, tgt, init = [], [], []
    for a in range(len(calls)):
        for k, f in enumerate(sorted(stored)):
            src.append(a)
            tgt.append(f)
            init.append(near if (a + k) % 2 else EYE)
    return calls, stored, src, tgt, np.array(init)


def test_mixed_batch_and_each_pair_alone(mods):
    h = mods[0].STDescManager()
    calls, stored, src, tgt, init = _mixed()
    opt = dict(k_neighbors=8, max_corr_dist=1.0)
    sx.store(h, stored, k_neighbors=8)
    got, direct = sx.check(h, calls, stored, src, tgt, init, "mixed", **opt)
    status = dict(zip(zip(src, tgt), got["status"].tolist()))
    assert status[(2, 2)] == ref.NO_POINTS and status[(0, 11)] == ref.NO_POINTS and status[(0, 17)] == ref.NO_CORRESPONDENCE
    assert ref.CONVERGED in got["status"] or ref.ITERATION_LIMIT in got["status"]
    for f, c in stored.items():
        sx.same_cloud(h, f, c, direct["cov"][len(calls) + sorted(stored).index(f)])
    # each pair alone: the same bits as in the batch
    for k in range(len(src)):
        one = sx.run(h, calls, [src[k]], [tgt[k]], init[k:k + 1], **opt)
        for f in sx.FIELDS:
            assert ref.same(one[f][0], got[f][k]), (k, f)
        assert np.array_equal(one["matches"][0][0], got["matches"][k][0]) and ref.same(one["matches"][0][1], got["matches"][k][1])
        assert ref.same(one["cov"][src[k]], got["cov"][src[k]])
    h.close()


# ---- independence ----
def test_independence_views_and_shards(mods):
    """the stored call's results and sgtd_register_clouds' / sgtd_register_voxels' do not touch each other; a pending
    batch is still there afterwards; a view with a store of its own and a multi-device handle give the plain handle's bits"""
    manager, synth = mods[:2]
    s, t, Rm, tm = ref.planted_scene(200, 4)
    s2, t2, _, _ = ref.planted_scene(150, 9)
    near = ref.near_start(Rm, tm)[None]
    opt = dict(k_neighbors=10, max_corr_dist=2.0)
    single, multi, view = manager.STDescManager(), manager.STDescManager(devices=[0, 0]), manager.STDescManager()
    m = synth.make_map(12, 80, stream=5)
    single.add_frames(m.xyz, m.label)
    view.attach_table(single)
    before = single.query_frames(m.xyz[:3], m.label[:3])
    single.set_frame_clouds([8], [t], k_neighbors=10)
    dense = rx.run(single, [s2, t2], [0], [1], None, **opt)
    pts, off = rx.pack([s2, t2])
    single.register_voxels(pts, off, [0, 1], [1], None, [0], [0], k_neighbors=10)
    voxel = single.result_voxel_registered()
    want = sx.run(single, [s], [0], [8], near, **opt)
    # the other calls' results are what they were
    again = single.result_registered()
    for f in rx.FIELDS:
        assert ref.same(again[f], dense[f]), f
    assert ref.same(single.register_covariances(1), dense["cov"][1]) and np.array_equal(single.register_matches(0)[0], dense["matches"][0][0])
    again = single.result_voxel_registered()
    assert all(ref.same(again[f], voxel[f]) for f in voxel)
    # and the other way round
    rx.run(single, [t2, s2], [1], [0], None, **opt)
    single.register_voxels(pts, off, [0, 1], [0], None, [1], [0], k_neighbors=10)
    again = sx.getters(single, single.result_stored_registered(), 1)
    sx.compare(again, want, [0], "after the other calls")
    # later set calls do not change the results either
    single.set_frame_clouds([9], [s2], k_neighbors=10)
    sx.compare(sx.getters(single, single.result_stored_registered(), 1), want, [0], "after a set call")
    # the batch is still there
    after = single.results()
    assert np.array_equal(before.cand_frame, after.cand_frame) and np.array_equal(before.n_cand, after.n_cand)
    # a view has a store of its own; a multi-device handle keeps it on its first device
    assert view.frame_cloud(8) is None and view.frame_clouds_info()["n_frames"] == 0
    for h in (view, multi):
        h.set_frame_clouds([8], [t], k_neighbors=10)
        sx.compare(sx.run(h, [s], [0], [8], near, **opt), want, [0], "view / shards")
        sx.same_cloud(h, 8, t, single.frame_cloud(8)[1])
    # the loops form is not a multi-device handle's
    qoff = np.array([0, len(s)], np.int64)
    assert multi._L.sgtd_register_stored_loops(multi._h, None, _ptr(s), 3, _ptr(qoff), 4, 0, 0) == -6
    assert b"multi-device" in multi._L.sgtd_last_error(multi._h)
    view.close()
    multi.close()
    single.close()


def test_stage_times(mods):
    h = mods[0].STDescManager()
    s, t, _, _ = ref.planted_scene(300, 7)
    h.set_frame_clouds([1], [t], k_neighbors=10)
    plain = sx.run(h, [s], [0], [1], None, k_neighbors=10, max_corr_dist=2.0)
    assert h.stored_register_stage_ms() == (0.0, 0.0, 0.0, 0.0)
    h.set_timing(True)
    try:
        timed = sx.run(h, [s], [0], [1], None, k_neighbors=10, max_corr_dist=2.0)
        ms = h.stored_register_stage_ms()
    finally:
        h.set_timing(False)
    assert all(v > 0.0 for v in ms) and ms[3] >= max(ms[:3])
    sx.compare(timed, plain, [0], "timed")
    h.close()


# ---- the loops form ----
def _rows(h, res, nq, cn, start, max_per_query, has_cloud):
    """the rule of sgtd_register_stored_loops restated over result_verify / result_refined -> [(query, cand, frame, init)]"""
    want = []
    for q in range(nq):
        score, rot, t = h.result_verify(q)
        if start == "refined":
            r = h.result_refined(q)
            rot, t = r["rot"], r["t"]
        ok = sorted((c for c in range(int(res.n_cand[q])) if score[c] >= 0), key=lambda c: (-score[c], c))[:min(max_per_query, cn)]
        want += [(q, c, int(res.cand_frame[q, c]), np.concatenate([rot[c].reshape(9), t[c]])) for c in ok if has_cloud(int(res.cand_frame[q, c]))]
    return want


def test_register_loops_stored(mods):
    import torch
    manager, synth, _, evaluate, ingest = mods
    cfg = {"min_seg": [20] * 32}
    p, l, off, _ = synth.make_posed_scans(20, 6000, stream=33, spacing=2.0, n_blobs=60, sensor_range=40.0, sigma=(0.05, 0.12))
    h = manager.STDescManager()
    cn = h.config_setting_["candidate_num"]
    h.add_scans(p, l, off, cfg)
    h.add_scans(p[off[3]:off[4]], l[off[3]:off[4]], np.array([0, 6000], np.int64), cfg)      # frame 20 repeats scan 3: a tie
    rng = np.random.default_rng(6)
    picks = [3, 9, 15]
    qp = np.concatenate([p[off[f]:off[f + 1]] for f in picks]).copy()
    qp[:, :3] += rng.normal(0.0, 0.01, (len(qp), 3)).astype(np.float32)
    ql = np.concatenate([l[off[f]:off[f + 1]] for f in picks])
    qo = np.arange(4, dtype=np.int64) * 6000
    res = h.query_scans(qp, ql, qo, cfg)
    assert np.all(res.n_cand > 0)
    # every frame's thinned cloud but 4 and 10 is stored
    map_clouds = {f: ingest.voxel_downsample(p[off[f]:off[f + 1], :3], 0.25) for f in range(20) if f not in (4, 10)}
    map_clouds[20] = map_clouds[3].copy()
    h.set_frame_clouds(list(map_clouds), [map_clouds[f] for f in map_clouds], k_neighbors=10)
    thin = [ingest.voxel_downsample(qp[qo[q]:qo[q + 1], :3], 0.25) for q in range(3)]
    assert all(50 < len(c) < 2000 for c in thin)
    tq = np.concatenate(thin)
    to = np.concatenate([[0], np.cumsum([len(c) for c in thin])]).astype(np.int64)
    opt = dict(k_neighbors=10, max_iterations=5, max_corr_dist=3.0)
    with pytest.raises(manager.SgtdError) as err:
        h.register_loops_stored(tq, to, **opt)                        # before verify()
    assert err.value.status == -7
    h.verify()
    with pytest.raises(manager.SgtdError) as err:
        h.register_loops_stored(tq, to, start="refined", **opt)      # refine_poses has not run on this batch
    assert err.value.status == -7
    # what the cases below rely on
    score0 = h.result_verify(0)[0][:int(res.n_cand[0])]
    ok0 = score0[score0 >= 0]
    verified = [int((h.result_verify(q)[0][:int(res.n_cand[q])] >= 0).sum()) for q in range(3)]
    print("verified candidates per query:", verified, "scores of query 0:", np.sort(ok0)[::-1][:6])
    assert len(np.unique(ok0)) < len(ok0), "no tie among query 0's verified candidates"
    assert max(verified) > 4, "no query has more verified candidates than 4"
    taken4 = _rows(h, res, 3, cn, "verify", 4, lambda f: True)
    assert any(w[2] in (4, 10) for w in taken4), "no taken candidate's frame is without a cloud"
    before = h.results()
    for start in ("verify", "refined"):
        if start == "refined":
            h.refine_poses()
        for mpq in (0, 1, 4, cn + 1):
            out = h.register_loops_stored(tq if mpq != 1 else torch.from_numpy(tq).cuda(), to, max_per_query=mpq, start=start, **opt)
            want = _rows(h, res, 3, cn, start, mpq, lambda f: f in map_clouds)
            what = (start, mpq)
            assert len(want) >= (3 if mpq >= 4 else 0), "the batch has too few verified candidates to say anything"
            assert out["query"].tolist() == [w[0] for w in want] and out["cand"].tolist() == [w[1] for w in want], what
            assert out["frame"].tolist() == [w[2] for w in want], what
            assert ref.same(out["init"], np.array([w[3] for w in want], np.float64).reshape(-1, 12)), what
            assert not set(out["frame"].tolist()) & {4, 10}
            sx.getters(h, out, 3)
            # the results: register_loops on the same dict of clouds, and a direct register_clouds call on those pairs
            loops = h.register_loops(tq, to, map_clouds, max_per_query=mpq, start=start, **opt)
            for f in ("query", "cand", "frame", "init") + rx.FIELDS:
                assert ref.same(out[f], loops[f]), (what, f)
            if want:
                frames = sorted(set(w[2] for w in want))
                direct = rx.run(h, thin + [map_clouds[f] for f in frames], [w[0] for w in want], [3 + frames.index(w[2]) for w in want],
                                np.array([w[3] for w in want]), **opt)
                sx.compare(out, direct, [w[0] for w in want], "loops %s %d" % what)
            else:
                assert out["pose"].shape == (0, 12)
            rows = out["query"] == 0
            if rows.any():
                k, frame, fit = evaluate.choose_registered(out["frame"][rows], out["fitness"][rows], best_fitness=0.0)
                assert k == -1 or fit == np.nanmin(out["fitness"][rows])
    # the batch is untouched
    after = h.results()
    assert np.array_equal(before.cand_frame, after.cand_frame) and np.array_equal(before.n_cand, after.n_cand)
    # a masked verification: the masked candidates never appear
    res = h.query_scans(qp, ql, qo, cfg)
    mask = 0x5555555555555555
    keep = torch.full((3,), mask, dtype=torch.int64, device="cuda")
    h.verify_masked(keep)
    torch.cuda.synchronize()
    out = h.register_loops_stored(tq, to, max_per_query=cn, **opt)
    want = _rows(h, res, 3, cn, "verify", cn, lambda f: f in map_clouds)
    assert len(want) >= 1 and all((mask >> w[1]) & 1 for w in want)
    assert out["query"].tolist() == [w[0] for w in want] and out["cand"].tolist() == [w[1] for w in want]
    assert all((mask >> int(c)) & 1 for c in out["cand"])
    h.close()
