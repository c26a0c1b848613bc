"""sgtd_register_clouds on the device against the numpy restatement of the rule in include/sgtd_accel.h
(tests/_register_ref.py): every array of every getter is compared bit for bit: pose, fitness, costs, counts, iterations,
status, covariances, matches and d2 (NaNs equal whatever their payload).  The handles here need no table, except for
register_loops."""
import ctypes as C

import numpy as np
import pytest

import _register_edges as rx
import _register_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, evaluate, ingest, manager, synth
    return manager, synth, _lib, evaluate, ingest


@pytest.fixture(scope="module")
def g(mods):
    h = mods[0].STDescManager()
    yield h
    h.close()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the planted scene ----
@pytest.mark.parametrize("n,k", [(300, 10), (600, 20)])
def test_planted_scene(g, n, k):
    s, t, Rm, tm = ref.planted_scene(n, 7)
    near = ref.near_start(Rm, tm)
    eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    got, want = rx.check(g, [s, t], [0, 0], [1, 1], np.array([eye, near]), "planted %d" % n, k_neighbors=k, max_corr_dist=2.0)
    assert got["status"].tolist() == [ref.CONVERGED, ref.CONVERGED] and got["n_matched"].tolist() == [n, n]
    for row, start in zip(got["pose"], (eye, near)):
        before, after = ref.pose_error(start, Rm, tm), ref.pose_error(row, Rm, tm)
        assert after[0] < 0.25 * before[0] and after[1] < 0.25 * before[1]      # (the bounds proper: test_register_host.py)
    # init_pose NULL is the identity
    alone, _ = rx.check(g, [s, t], [0], [1], None, "identity", k_neighbors=k, max_corr_dist=2.0)
    assert ref.same(alone["pose"][0], got["pose"][0]) and alone["iterations"][0] == got["iterations"][0]


def test_self_registration(g):
    s, _, _, _ = ref.planted_scene(300, 3)
    got, _ = rx.check(g, [s], [0], [0], None, "self", k_neighbors=10)
    assert got["status"].tolist() == [ref.CONVERGED] and got["iterations"].tolist() == [1] and got["fitness"][0] == 0.0
    assert np.array_equal(got["pose"][0], np.concatenate([np.eye(3).reshape(9), np.zeros(3)]))
    assert got["matches"][0][0].tolist() == list(range(300))


# ---- a mixed batch ----
def _mixed():
    rng = np.random.default_rng(31)
    sizes = [260, 300, 90, 150, 40, 129, 0, 75]
    s, t, Rm, tm = ref.planted_scene(400, 12)
    clouds = []
    for k, n in enumerate(sizes):
        base = s if k % 2 == 0 else t
        clouds.append(base[rng.permutation(len(base))[:n]])
    clouds.append((t[:200].astype(np.float64) + [100.0, 0.0, 0.0]).astype(np.float32))      # cloud 8: 100 m away
    near = ref.near_start(Rm, tm)
    eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    odd = [1, 3, 5, 7]
    src, tgt, init = [], [], []
    for k in range(40):
        if k % 10 == 6:
            a, b = (6, 1) if k < 20 else (0, 6)             # no points, on either side
        elif k % 10 == 8:
            a, b = 0, 8                                     # nothing within max_corr_dist
        elif k % 10 == 3:
            a, b = 1, 1 if k < 20 else 3                    # cloud 1 as source and target, of itself and of another
        else:
            a, b = [0, 2, 4][k % 3], odd[k % 4]             # cloud 0 the source of many pairs
        src.append(a)
        tgt.append(b)
        init.append(near if k % 2 else eye)
    return clouds, src, tgt, np.array(init)


def test_mixed_batch_and_each_pair_alone(g):
    clouds, src, tgt, init = _mixed()
    opt = dict(k_neighbors=8, max_corr_dist=1.0)
    want_status = set()
    for limit in (1, 2, 64):
        got, want = rx.check(g, clouds, src, tgt, init, "mixed, max_iterations %d" % limit, max_iterations=limit, **opt)
        want_status |= set(got["status"].tolist())
        if limit < 64:
            assert ref.ITERATION_LIMIT in got["status"] and got["iterations"].max() == limit
    assert want_status == {ref.CONVERGED, ref.ITERATION_LIMIT, ref.NO_CORRESPONDENCE, ref.NO_POINTS}
    # each pair alone: the same bits as in the batch (got: the last, max_iterations 64)
    for k in range(40):
        one = rx.run(g, clouds, [src[k]], [tgt[k]], init[k:k + 1], max_iterations=64, **opt)
        for f in rx.FIELDS:
            assert ref.same(one[f][0], got[f][k]), (k, f)
        assert np.array_equal(one["matches"][0][0], got["matches"][k][0]) and ref.same(one["matches"][0][1], got["matches"][k][1])
        assert ref.same(one["cov"][src[k]], got["cov"][src[k]]) and ref.same(one["cov"][tgt[k]], got["cov"][tgt[k]])


# ---- error handling ----
def _raw(h, pts, off, src, tgt, init=None, opt=None, stride=3, n_clouds=None, n_pairs=None, dev=0):
    return h._L.sgtd_register_clouds(h._h, None if opt is None else C.byref(opt), _ptr(pts), stride, _ptr(off),
                                     len(off) - 1 if n_clouds is None else n_clouds, _ptr(src), _ptr(tgt), _ptr(init),
                                     len(src) if n_pairs is None else n_pairs, dev)


def test_errors_keep_the_earlier_results(mods):
    manager, _, _lib = mods[:3]
    h = manager.STDescManager()
    L = h._L
    n64 = C.c_int64(0)
    buf = np.zeros(16)
    # the getters before a run
    assert L.sgtd_result_registered(h._h, _ptr(buf), None, None, None, None, None) == -7
    assert L.sgtd_result_register_covariances(h._h, 0, None, 0, C.byref(n64)) == -7
    assert L.sgtd_result_register_matches(h._h, 0, None, None, 0, C.byref(n64)) == -7
    assert L.sgtd_register_stage_ms(h._h, None, None, None, None) == -7
    s, t, _, _ = ref.planted_scene(150, 2)
    first = rx.run(h, [s, t], [0], [1], None, k_neighbors=8, max_corr_dist=2.0)
    pts, off = rx.pack([s, t])
    src, tgt = np.array([0], np.int32), np.array([1], np.int32)
    eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])[None].copy()
    assert L.sgtd_register_clouds(None, None, _ptr(pts), 3, _ptr(off), 2, _ptr(src), _ptr(tgt), None, 1, 0) == -1
    bad = [
        dict(n_clouds=-1), dict(n_pairs=-1), dict(stride=2), dict(stride=5),
        dict(pts=None), dict(off=None, n_clouds=2), dict(src=None, n_pairs=1), dict(tgt=None),
        dict(off=np.array([1, 150, 400], np.int64)), dict(off=np.array([0, 250, 150], np.int64)),
        dict(src=np.array([2], np.int32)), dict(src=np.array([-1], np.int32)), dict(tgt=np.array([2], np.int32)), dict(tgt=np.array([-1], np.int32)),
    ]
    for v in (np.nan, np.inf, -np.inf):
        p = eye.copy()
        p[0, 4] = v
        bad.append(dict(init=p))
    for field, values in (("k_neighbors", (2, 33, -1)), ("max_iterations", (0, -3)), ("lm_max_trials", (0,)), ("reserved", (1,)),
                          ("max_corr_dist", (0.0, -1.0, np.nan)), ("lm_init_lambda_factor", (0.0, np.inf, np.nan)),
                          ("rotation_eps", (0.0, -1.0, np.nan)), ("translation_eps", (0.0, np.inf)), ("plane_eps", (0.0, np.nan))):
        for v in values:
            o = _lib.RegisterOptions()
            L.sgtd_default_register_options(C.byref(o))
            setattr(o, field, v)
            bad.append(dict(opt=o))
    for kw in bad:
        a = dict(pts=pts, off=off, src=src, tgt=tgt)
        a.update(kw)
        assert _raw(h, **a) == -1, kw
    # more than a cap: SGTD_ERR_UNSUPPORTED, and the handle says which
    big = np.array([0, (1 << 17) + 1], np.int64)
    assert _raw(h, pts, big, src, np.array([0], np.int32)) == -6 and b"points a cloud" in L.sgtd_last_error(h._h)
    # +inf is a max_corr_dist; the earlier results are all still there
    again = {k: v for k, v in h.result_registered().items()}
    for f in rx.FIELDS:
        assert ref.same(again[f], first[f]), f
    assert ref.same(h.register_covariances(1), first["cov"][1]) and np.array_equal(h.register_matches(0)[0], first["matches"][0][0])
    # too small a capacity: the size needed, the first entries written
    cov = np.full((10, 3, 3), -7.0)
    assert L.sgtd_result_register_covariances(h._h, 0, _ptr(cov), 4, C.byref(n64)) == -4 and n64.value == 150
    assert ref.same(cov[:4], first["cov"][0][:4]) and (cov[4:] == -7.0).all()
    j, d2 = np.full(10, -9, np.int32), np.full(10, -9.0)
    assert L.sgtd_result_register_matches(h._h, 0, _ptr(j), _ptr(d2), 6, C.byref(n64)) == -4 and n64.value == 150
    assert np.array_equal(j[:6], first["matches"][0][0][:6]) and (j[6:] == -9).all() and ref.same(d2[:6], first["matches"][0][1][:6])
    assert L.sgtd_result_register_matches(h._h, 0, None, None, 0, C.byref(n64)) == 0 and n64.value == 150
    assert L.sgtd_result_register_covariances(h._h, 2, None, 0, C.byref(n64)) == -1
    assert L.sgtd_result_register_matches(h._h, 1, None, None, 0, C.byref(n64)) == -1
    assert L.sgtd_result_register_matches(h._h, 0, None, None, -1, C.byref(n64)) == -1
    # no pair at all is a run: nothing comes back, no cloud has covariances
    out = h.register_clouds(pts, off, [], [])
    assert out["pose"].shape == (0, 12) and h.register_covariances(0).shape == (0, 3, 3)
    h.close()


def test_views_shards_and_a_pending_batch(mods):
    """the call is independent of the table and the batch: a view whose owner holds a pending batch and a multi-device
    handle give the plain handle's bits, and the batch is still there afterwards"""
    manager, synth = mods[:2]
    s, t, Rm, tm = ref.planted_scene(200, 4)
    single, multi, view = manager.STDescManager(), manager.STDescManager(devices=[0, 0]), manager.STDescManager()
    m = synth.make_map(12, 80, stream=5)
    single.add_frames(m.xyz, m.label)
    view.attach_table(single)
    before = single.query_frames(m.xyz[:3], m.label[:3])
    want = rx.run(single, [s, t], [0], [1], ref.near_start(Rm, tm)[None], k_neighbors=10, max_corr_dist=2.0)
    for h in (view, multi):
        got = rx.run(h, [s, t], [0], [1], ref.near_start(Rm, tm)[None], k_neighbors=10, max_corr_dist=2.0)
        for f in rx.FIELDS:
            assert ref.same(got[f], want[f]), f
        assert ref.same(got["cov"][0], want["cov"][0]) and np.array_equal(got["matches"][0][0], want["matches"][0][0])
    after = single.results()
    assert np.array_equal(before.cand_frame, after.cand_frame) and np.array_equal(before.n_cand, after.n_cand)
    view.close()
    multi.close()
    single.close()


def test_stage_times(g):
    s, t, _, _ = ref.planted_scene(300, 7)
    plain = rx.run(g, [s, t], [0], [1], None, k_neighbors=10, max_corr_dist=2.0)
    assert g.register_stage_ms() == (0.0, 0.0, 0.0, 0.0)
    g.set_timing(True)
    try:
        timed = rx.run(g, [s, t], [0], [1], None, k_neighbors=10, max_corr_dist=2.0)
        ms = g.register_stage_ms()
    finally:
        g.set_timing(False)
    assert all(v > 0.0 for v in ms) and ms[3] >= max(ms[:3])
    for f in rx.FIELDS:
        assert ref.same(timed[f], plain[f]), f


# ---- register_loops ----
def test_register_loops(mods):
    manager, synth, _, evaluate, ingest = mods
    cfg = {"min_seg": [20] * 32}
    p, l, off, _ = synth.make_posed_scans(20, 6000, stream=33, spacing=2.0, n_blobs=60, sensor_range=40.0, sigma=(0.05, 0.12))
    h = manager.STDescManager()
    kp_off = h.add_scans(p, l, off, cfg)
    assert np.all(np.diff(kp_off) >= 20)
    rng = np.random.default_rng(6)
    picks = [3, 9, 15]
    qp = np.concatenate([p[off[f]:off[f + 1]] for f in picks]).copy()
    qp[:, :3] += rng.normal(0.0, 0.01, (len(qp), 3)).astype(np.float32)
    ql = np.concatenate([l[off[f]:off[f + 1]] for f in picks])
    qo = np.arange(4, dtype=np.int64) * 6000
    res = h.query_scans(qp, ql, qo, cfg)
    assert np.all(res.n_cand > 0)
    # the raw clouds, thinned; frames 4 and 10 have none
    map_clouds = {f: ingest.voxel_downsample(p[off[f]:off[f + 1], :3], 0.25) for f in range(20) if f not in (4, 10)}
    thin = [ingest.voxel_downsample(qp[qo[q]:qo[q + 1], :3], 0.25) for q in range(3)]
    assert all(50 < len(c) < 2000 for c in thin)
    tq = np.concatenate(thin)
    to = np.concatenate([[0], np.cumsum([len(c) for c in thin])]).astype(np.int64)
    with pytest.raises(manager.SgtdError):
        h.register_loops(tq, to, map_clouds)                   # before verify()
    h.verify()
    with pytest.raises(manager.SgtdError):
        h.register_loops(tq, to, map_clouds, start="refined")      # refine_poses has not run on this batch
    opt = dict(k_neighbors=10, max_iterations=5, max_corr_dist=3.0)
    for start in ("verify", "refined"):
        if start == "refined":
            h.refine_poses()
        out = h.register_loops(tq, to, map_clouds, max_per_query=4, start=start, **opt)
        # the pairs: per query the candidates with a result by descending score, ties in candidate order, the first four,
        # those whose frame has a cloud
        want = []
        for q in range(3):
            score, rot, t = h.result_verify(q)
            if start == "refined":
                r = h.result_refined(q)
                rot, t = r["rot"], r["t"]
            ok = sorted((c for c in range(int(res.n_cand[q])) if score[c] >= 0), key=lambda c: (-score[c], c))[:4]
            want += [(q, c, int(res.cand_frame[q, c]), np.concatenate([rot[c].reshape(9), t[c]])) for c in ok
                     if int(res.cand_frame[q, c]) in map_clouds]
        assert len(want) >= 3, "the batch has too few verified candidates to say anything"
        assert out["query"].tolist() == [w[0] for w in want] and out["cand"].tolist() == [w[1] for w in want]
        assert out["frame"].tolist() == [w[2] for w in want] and np.array_equal(out["init"], np.array([w[3] for w in want]))
        assert not set(out["frame"].tolist()) & {4, 10}
        # the results: a direct register_clouds call on those pairs
        frames = sorted(set(w[2] for w in want))
        clouds = thin + [map_clouds[f] for f in frames]
        direct = rx.run(h, clouds, [w[0] for w in want], [3 + frames.index(w[2]) for w in want], np.array([w[3] for w in want]), **opt)
        for f in rx.FIELDS:
            assert ref.same(out[f], direct[f]), (start, f)
        # the node's choice over one query's rows is a pure function of them
        rows = out["query"] == 0
        k, frame, fit = evaluate.choose_registered(out["frame"][rows], out["fitness"][rows], best_fitness=0.0)
        assert k == -1 or fit == np.nanmin(out["fitness"][rows])
    h.close()
