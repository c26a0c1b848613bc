"""sgtd_register_voxels on the device against the numpy restatement of the rule in include/sgtd_accel.h
(tests/_voxel_register_ref.py): every array of every getter is compared bit for bit: pose, fitness, costs, counts,
iterations, status, the voxel maps (coordinates, counts, means, covariances) and the matches (NaNs equal whatever their
payload).  The handles here need no table, except for register_loops_local."""
import ctypes as C

import numpy as np
import pytest

import _register_edges as rx
import _register_ref as ref
import _voxel_register_edges as vx
import _voxel_register_ref as vref

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
@pytest.mark.parametrize("mode", [1, 7, 27])
@pytest.mark.parametrize("n,k", [(300, 10), (600, 20)])
def test_planted_scene(g, n, k, mode):
    s, t, Rm, tm = ref.planted_scene(n, 7)
    near = ref.near_start(Rm, tm)
    got, want = vx.check(g, [s, t], [0, 1], [1], None, [0, 0], [0, 0], np.array([vx.EYE, near]), "planted %d mode %d" % (n, mode),
                         k_neighbors=k, neighbor_mode=mode)
    assert got["status"].tolist() == [vref.CONVERGED, vref.CONVERGED]
    assert (got["n_matched"] > n // 2).all() and (got["n_corr"] >= got["n_matched"]).all()
    e0 = ref.pose_error(near, Rm, tm)
    for row in got["pose"]:
        after = ref.pose_error(row, Rm, tm)
        assert after[0] < 0.5 * e0[0] and after[1] < 0.5 * e0[1]      # (the bounds proper: test_voxel_register_host.py)
    # init_pose NULL is the identity
    alone, _ = vx.check(g, [s, t], [0, 1], [1], None, [0], [0], None, "identity", k_neighbors=k, neighbor_mode=mode)
    for f in vx.FIELDS:
        assert ref.same(alone[f][0], got[f][0]), f


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
    # maps: 0 one scan; 1 two posed scans; 2 no member; 3 an empty member alone; 4 the far cloud; 5 four members, an empty
    # one and cloud 1 (a source as well) among them
    members = [[1], [1, 3], [], [6], [8], [5, 7, 1, 6]]
    map_off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    map_cloud = np.array([c for m in members for c in m], np.int32)
    map_pose = np.array([vx.EYE, vx.EYE, vx.pose_row([0.1, 1.0, 0.2], 0.004, [0.01, -0.02, 0.005]), vx.EYE, vx.EYE,
                         vx.pose_row([1.0, 0.0, 0.3], -0.003, [0.0, 0.015, -0.01]), vx.EYE, vx.pose_row([0.0, 0.0, 1.0], 0.002, [0.02, 0.0, 0.0]),
                         vx.EYE])
    near = ref.near_start(Rm, tm)
    src, tgt, init = [], [], []
    for k in range(40):
        if k % 10 == 6:
            a, b = (6, 0) if k < 20 else (0, 2 if k < 30 else 3)      # no points: the source, a map without a voxel
        elif k % 10 == 8:
            a, b = 0, 4                                               # a map 100 m from its source
        elif k % 10 == 3:
            a, b = 1, 0 if k < 20 else 5                              # cloud 1 against maps it is a member of
        else:
            a, b = [0, 2, 4][k % 3], [0, 1, 5, 1][k % 4]              # several pairs on one map
        src.append(a)
        tgt.append(b)
        init.append(near if k % 2 else vx.EYE)
    return clouds, map_off, map_cloud, map_pose, src, tgt, np.array(init)


def test_mixed_batch_and_each_pair_alone(g):
    clouds, map_off, map_cloud, map_pose, src, tgt, init = _mixed()
    seen = set()
    for mode, limit in ((1, 2), (27, 1), (7, 64)):
        got, want = vx.check(g, clouds, map_off, map_cloud, map_pose, src, tgt, init, "mixed, mode %d, max_iterations %d" % (mode, limit),
                             k_neighbors=8, neighbor_mode=mode, max_iterations=limit)
        seen |= set(got["status"].tolist())
        if limit < 64:
            assert vref.ITERATION_LIMIT in got["status"] and got["iterations"].max() == limit
    assert seen == {vref.CONVERGED, vref.ITERATION_LIMIT, vref.NO_CORRESPONDENCE, vref.NO_POINTS}
    assert [len(m["n_points"]) for m in got["maps"]][2:4] == [0, 0]
    # each pair alone, with its map alone: the same bits as in the batch (got: the last, mode 7)
    for k in range(40):
        m = tgt[k]
        lo, hi = int(map_off[m]), int(map_off[m + 1])
        one = vx.run(g, clouds, [0, hi - lo], map_cloud[lo:hi], map_pose[lo:hi], [src[k]], [0], init[k:k + 1], k_neighbors=8, neighbor_mode=7)
        for f in vx.FIELDS:
            assert ref.same(one[f][0], got[f][k]), (k, f)
        assert np.array_equal(one["matches"][0], got["matches"][k]) and vx.same_maps(one["maps"][0], got["maps"][m]), k


# ---- strides, host and device points ----
def test_strides_and_device_points(g):
    clouds, map_off, map_cloud, map_pose, src, tgt, init = _mixed()
    opt = dict(k_neighbors=8, neighbor_mode=7, max_iterations=3)
    base, _ = vx.check(g, clouds, map_off, map_cloud, map_pose, src[:12], tgt[:12], init[:12], "stride 3, host", **opt)
    for dev, stride in ((False, 4), (True, 3), (True, 4)):
        got = vx.run(g, clouds, map_off, map_cloud, map_pose, src[:12], tgt[:12], init[:12], dev=dev, stride=stride, **opt)
        vx.compare(got, base, "stride %d, device %s" % (stride, dev))


# ---- error handling ----
def _raw(h, pts, off, moff, mcl, src, tgt, mpose=None, init=None, opt=None, stride=3, n_clouds=None, n_maps=None, n_pairs=None, dev=0):
    return h._L.sgtd_register_voxels(h._h, None if opt is None else C.byref(opt), _ptr(pts), stride, _ptr(off),
                                     len(off) - 1 if n_clouds is None else n_clouds, _ptr(moff), _ptr(mcl), _ptr(mpose),
                                     len(moff) - 1 if n_maps is None else n_maps, _ptr(src), _ptr(tgt), _ptr(init),
                                     len(src) if n_pairs is None else n_pairs, dev)


def test_errors_keep_the_earlier_results(mods):
    manager, _, _lib = mods[:3]
    h = manager.STDescManager()
    L = h._L
    n64 = C.c_int64(0)
    buf = np.zeros(16)
    # the getters before a run
    assert L.sgtd_result_voxel_registered(h._h, _ptr(buf), None, None, None, None, None, None) == -7
    assert L.sgtd_result_voxel_map(h._h, 0, None, None, None, None, 0, C.byref(n64)) == -7
    assert L.sgtd_result_voxel_matches(h._h, 0, None, 0, C.byref(n64)) == -7
    assert L.sgtd_voxel_register_stage_ms(h._h, None, None, None, None, None) == -7
    s, t, _, _ = ref.planted_scene(150, 2)
    first = vx.run(h, [s, t], [0, 1], [1], None, [0], [0], None, k_neighbors=8, neighbor_mode=7)
    pts, off = rx.pack([s, t])
    moff, mcl = np.array([0, 1], np.int32), np.array([1], np.int32)
    src, tgt = np.array([0], np.int32), np.array([0], np.int32)
    eye = vx.EYE[None].copy()
    assert L.sgtd_register_voxels(None, None, _ptr(pts), 3, _ptr(off), 2, _ptr(moff), _ptr(mcl), None, 1, _ptr(src), _ptr(tgt), None, 1, 0) == -1
    bad = [
        dict(n_clouds=-1), dict(n_pairs=-1), dict(n_maps=-1), dict(stride=2), dict(stride=5),
        dict(pts=None), dict(off=None, n_clouds=2), dict(src=None, n_pairs=1), dict(tgt=None), dict(moff=None, n_maps=1), dict(mcl=None),
        dict(off=np.array([1, 150, 400], np.int64)), dict(off=np.array([0, 250, 150], np.int64)),
        dict(moff=np.array([1, 1], np.int32)), dict(moff=np.array([0, 1, 0], np.int32), tgt=np.array([0], np.int32)),
        dict(mcl=np.array([2], np.int32)), dict(mcl=np.array([-1], np.int32)),
        dict(src=np.array([2], np.int32)), dict(src=np.array([-1], np.int32)), dict(tgt=np.array([1], np.int32)), dict(tgt=np.array([-1], np.int32)),
    ]
    for v in (np.nan, np.inf, -np.inf):
        p = eye.copy()
        p[0, 4] = v
        bad.append(dict(init=p))
        bad.append(dict(mpose=p))
    for field, values in (("k_neighbors", (2, 33, -1)), ("max_iterations", (0, -3)), ("lm_max_trials", (0,)), ("reserved", (1,)),
                          ("voxel_resolution", (0.0, -1.0, np.nan, np.inf)), ("neighbor_mode", (0, 2, 6, 26, 28, -1)),
                          ("lm_init_lambda_factor", (0.0, np.inf, np.nan)), ("rotation_eps", (0.0, -1.0, np.nan)),
                          ("translation_eps", (0.0, np.inf)), ("plane_eps", (0.0, np.nan))):
        for v in values:
            o = _lib.VoxelRegisterOptions()
            L.sgtd_default_voxel_register_options(C.byref(o))
            setattr(o, field, v)
            bad.append(dict(opt=o))
    for kw in bad:
        a = dict(pts=pts, off=off, moff=moff, mcl=mcl, src=src, tgt=tgt)
        a.update(kw)
        assert _raw(h, **a) == -1, kw
    # more than a cap: SGTD_ERR_UNSUPPORTED, and the handle says which.  (Offsets alone name the sizes: nothing is read)
    big = np.array([0, (1 << 17) + 1], np.int64)
    assert _raw(h, pts, big, moff, np.array([0], np.int32), src, tgt) == -6 and b"points a cloud" in L.sgtd_last_error(h._h)
    many = np.zeros(65537, np.int32)
    assert _raw(h, pts, off, many, mcl, src, tgt) == -6 and b"SGTD_VREG_MAX_MAPS" in L.sgtd_last_error(h._h)
    full = np.array([0, 1 << 17], np.int64)
    assert _raw(h, None, full, np.array([0, 257], np.int32), np.zeros(257, np.int32), src, tgt, n_pairs=0) == -1      # (points NULL)
    fat = np.zeros((1, 3), np.float32)
    assert _raw(h, fat, full, np.array([0, 257], np.int32), np.zeros(257, np.int32), src, tgt, n_pairs=0) == -6
    assert b"SGTD_VREG_MAX_MEMBER_POINTS" in L.sgtd_last_error(h._h)
    o = _lib.VoxelRegisterOptions()
    L.sgtd_default_voxel_register_options(C.byref(o))
    o.neighbor_mode = 27
    nsrc = (1 << 26) // 27 // (1 << 17) + 1
    assert _raw(h, fat, full, np.array([0, 0], np.int32), np.zeros(0, np.int32), np.zeros(nsrc, np.int32), np.zeros(nsrc, np.int32), opt=o) == -6
    assert b"SGTD_VREG_MAX_CORR" in L.sgtd_last_error(h._h)
    # the earlier results are all still there
    again = h.result_voxel_registered()
    for f in vx.FIELDS:
        assert ref.same(again[f], first[f]), f
    assert vx.same_maps(h.voxel_map(0), first["maps"][0]) and np.array_equal(h.voxel_matches(0), first["matches"][0])
    # too small a capacity: the size needed, the first entries written
    nv = len(first["maps"][0]["n_points"])
    assert nv > 4
    coord, cnt, mean, cov = np.full((10, 3), -9, np.int32), np.full(10, -9, np.int32), np.full((10, 3), -7.0), np.full((10, 3, 3), -7.0)
    assert L.sgtd_result_voxel_map(h._h, 0, _ptr(coord), _ptr(cnt), _ptr(mean), _ptr(cov), 4, C.byref(n64)) == -4 and n64.value == nv
    assert np.array_equal(coord[:4], first["maps"][0]["coord"][:4]) and (coord[4:] == -9).all()
    assert np.array_equal(cnt[:4], first["maps"][0]["n_points"][:4]) and (cnt[4:] == -9).all()
    assert ref.same(mean[:4], first["maps"][0]["mean"][:4]) and (mean[4:] == -7.0).all()
    assert ref.same(cov[:4], first["maps"][0]["cov"][:4]) and (cov[4:] == -7.0).all()
    j = np.full(20, -9, np.int32)
    assert L.sgtd_result_voxel_matches(h._h, 0, _ptr(j), 6, C.byref(n64)) == -4 and n64.value == 150 * 7
    assert np.array_equal(j[:6], first["matches"][0][:6]) and (j[6:] == -9).all()
    assert L.sgtd_result_voxel_matches(h._h, 0, None, 0, C.byref(n64)) == 0 and n64.value == 150 * 7
    assert L.sgtd_result_voxel_map(h._h, 1, None, None, None, None, 0, C.byref(n64)) == -1
    assert L.sgtd_result_voxel_map(h._h, -1, None, None, None, None, 0, C.byref(n64)) == -1
    assert L.sgtd_result_voxel_matches(h._h, 1, None, 0, C.byref(n64)) == -1
    assert L.sgtd_result_voxel_matches(h._h, 0, None, -1, C.byref(n64)) == -1
    # no pair at all is a run: the maps are built, no pair comes back; no map at all is one too
    out = h.register_voxels(pts, off, moff, mcl, None, [], [], k_neighbors=8)
    assert out["pose"].shape == (0, 12) and vx.same_maps(h.voxel_map(0), first["maps"][0])
    out = h.register_voxels(pts, off, [0], [], None, [], [])
    assert out["pose"].shape == (0, 12)
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
    args = ([s, t], [0, 1], [1], None, [0], [0], ref.near_start(Rm, tm)[None])
    want = vx.run(single, *args, k_neighbors=10, neighbor_mode=7)
    for h in (view, multi):
        got = vx.run(h, *args, k_neighbors=10, neighbor_mode=7)
        vx.compare(got, want, "view or shards")
    after = single.results()
    assert np.array_equal(before.cand_frame, after.cand_frame) and np.array_equal(before.n_cand, after.n_cand)
    view.close()
    multi.close()
    single.close()


def test_register_clouds_and_register_voxels_keep_apart(g):
    """neither call disturbs the other's results"""
    s, t, Rm, tm = ref.planted_scene(200, 4)
    near = ref.near_start(Rm, tm)[None]
    dense = rx.run(g, [s, t], [0], [1], near, k_neighbors=10, max_corr_dist=2.0)
    vox = vx.run(g, [t, s], [0, 1], [0], None, [1], [0], near, k_neighbors=10, neighbor_mode=7)
    again = g.result_registered()
    for f in rx.FIELDS:
        assert ref.same(again[f], dense[f]), f
    assert ref.same(g.register_covariances(0), dense["cov"][0]) and ref.same(g.register_covariances(1), dense["cov"][1])
    assert np.array_equal(g.register_matches(0)[0], dense["matches"][0][0]) and ref.same(g.register_matches(0)[1], dense["matches"][0][1])
    rx.run(g, [s[:120], t[:90]], [0, 1], [1, 0], None, k_neighbors=6, max_corr_dist=1.0)
    again = g.result_voxel_registered()
    for f in vx.FIELDS:
        assert ref.same(again[f], vox[f]), f
    assert vx.same_maps(g.voxel_map(0), vox["maps"][0]) and np.array_equal(g.voxel_matches(0), vox["matches"][0])


def test_stage_times(g):
    s, t, _, _ = ref.planted_scene(300, 7)
    args = ([s, t], [0, 1], [1], None, [0], [0], None)
    plain = vx.run(g, *args, k_neighbors=10, neighbor_mode=7)
    assert g.voxel_register_stage_ms() == (0.0, 0.0, 0.0, 0.0, 0.0)
    g.set_timing(True)
    try:
        timed = vx.run(g, *args, k_neighbors=10, neighbor_mode=7)
        ms = g.voxel_register_stage_ms()
    finally:
        g.set_timing(False)
    assert all(v > 0.0 for v in ms) and ms[4] >= max(ms[:4])
    vx.compare(timed, plain, "timed")


# ---- register_loops_local ----
def test_register_loops_local(mods):
    manager, synth, _, evaluate, ingest = mods
    cfg = {"min_seg": [20] * 32}
    p, l, off, poses = synth.make_posed_scans(20, 6000, stream=33, spacing=2.0, n_blobs=60, sensor_range=40.0, sigma=(0.05, 0.12))
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
    # the frames' world poses as rows of (rot row-major, t); the raw clouds, thinned; frames 4 and 10 have none
    poses = np.asarray(poses, np.float64)
    T = poses.reshape(-1, 3, 4) if poses.ndim == 2 else poses[:, :3, :]
    frame_poses = [np.concatenate([T[f][:, :3].reshape(9), T[f][:, 3]]) for f in range(20)]
    map_clouds = {f: ingest.voxel_downsample(p[off[f]:off[f + 1], :3], 0.25) for f in range(20) if f not in (4, 10)}
    thin = [ingest.voxel_downsample(qp[qo[q]:qo[q + 1], :3], 0.25) for q in range(3)]
    tq = np.concatenate(thin)
    to = np.concatenate([[0], np.cumsum([len(c) for c in thin])]).astype(np.int64)
    with pytest.raises(manager.SgtdError):
        h.register_loops_local(tq, to, map_clouds, frame_poses)                   # before verify()
    h.verify()
    opt = dict(k_neighbors=10, max_iterations=5, neighbor_mode=7)
    out = h.register_loops_local(tq, to, map_clouds, frame_poses, radius=5.0, max_members=4, max_per_query=4, **opt)
    q, c, f, init = h.register_pairs(4, "verify")
    keep = np.array([int(x) in map_clouds for x in f], bool)
    assert keep.sum() >= 3, "the batch has too few verified candidates to say anything"
    assert out["query"].tolist() == q[keep].tolist() and out["cand"].tolist() == c[keep].tolist() and out["frame"].tolist() == f[keep].tolist()
    assert np.array_equal(out["init"], init[keep]) and not set(out["frame"].tolist()) & {4, 10}
    # the maps: one per distinct candidate frame, its members by the host rule
    assert out["map_frames"] == sorted(set(f[keep].tolist())) and len(out["members"]) == len(out["map_frames"])
    for x, mem in zip(out["map_frames"], out["members"]):
        near = [i for i in range(20) if i != x and i in map_clouds and np.linalg.norm(frame_poses[i][9:] - frame_poses[x][9:]) <= 5.0]
        assert mem.tolist() == ([x] + near)[:4] and not set(mem.tolist()) & {4, 10}
    assert any(len(m) > 1 for m in out["members"])
    # the results: a direct register_voxels call on those maps and pairs
    frames = sorted(set(int(i) for m in out["members"] for i in m))
    clouds = thin + [map_clouds[i] for i in frames]
    map_cloud = np.array([3 + frames.index(int(i)) for m in out["members"] for i in m], np.int32)
    assert np.array_equal(map_cloud, out["map_cloud"])
    tgt = [out["map_frames"].index(int(x)) for x in out["frame"]]
    direct = vx.run(h, clouds, out["map_off"], map_cloud, out["map_pose"], out["query"], tgt, out["init"], **opt)
    for fld in vx.FIELDS:
        assert ref.same(out[fld], direct[fld]), fld
    rows = out["query"] == 0
    k, frame, fit = evaluate.choose_registered(out["frame"][rows], out["fitness"][rows], best_fitness=0.0)
    assert k == -1 or fit == np.nanmin(out["fitness"][rows])
    h.close()
