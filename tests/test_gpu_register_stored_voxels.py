"""sgtd_register_stored_voxels on the device: the results are those of sgtd_register_voxels on [the call's clouds] + [the
member frames' stored clouds], bit for bit (pose, fitness, costs, counts, iterations, status, every voxel of every map, every
match): against the numpy restatement (tests/_voxel_register_ref.py) and against a direct sgtd_register_voxels call, through
every getter."""
import ctypes as C

import numpy as np
import pytest

import _register_edges as rx
import _register_ref as ref
import _stored_edges as sx
import _stored_voxel_edges as svx
import _voxel_register_edges as vx
import _voxel_register_ref as vref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, manager, synth
    return manager, synth, _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the planted scene ----
@pytest.mark.parametrize("mode", [1, 7, 27])
def test_planted_scene(mods, mode):
    h = mods[0].STDescManager()
    s, t, Rm, tm = ref.planted_scene(300, 7)
    near = ref.near_start(Rm, tm)
    h.set_frame_clouds([5], [t], k_neighbors=10)
    got, _ = svx.check(h, [s], {5: t}, [0, 1], [5], None, [0, 0], [0, 0], np.array([vx.EYE, near]), "planted, mode %d" % mode, k_neighbors=10,
                       neighbor_mode=mode)
    assert got["status"].tolist() == [vref.CONVERGED, vref.CONVERGED] and (got["n_matched"] > 150).all()
    e0 = ref.pose_error(near, Rm, tm)
    for row in got["pose"]:
        after = ref.pose_error(row, Rm, tm)
        assert after[0] < 0.5 * e0[0] and after[1] < 0.5 * e0[1]
    # init None is the identity
    alone = svx.run(h, [s], [0, 1], [5], None, [0], [0], None, k_neighbors=10, neighbor_mode=mode)
    for f in svx.FIELDS:
        assert ref.same(alone[f][0], got[f][0]), f
    h.close()


# ---- a mixed batch ----
def _mixed():
    """an empty source, a frame stored with zero points, a one-point cloud on either side, a NaN coordinate on either side,
    a map with no voxel, a frame that is a member of several maps and twice of one, an empty map, a map 100 m away"""
    rng = np.random.default_rng(31)
    s, t, Rm, tm = ref.planted_scene(400, 12)
    cut = lambda base, n: base[rng.permutation(len(base))[:n]].copy()      # noqa: E731
    calls = [cut(s, 260), cut(s, 90), cut(s, 0), cut(s, 1), cut(s, 129)]
    calls[4][17, 1] = np.nan
    stored = {2: cut(t, 300), 7: cut(t, 150), 11: cut(t, 0), 13: cut(t, 1), 19: cut(t, 75),
              17: (t[:200].astype(np.float64) + [100.0, 0.0, 0.0]).astype(np.float32)}
    stored[19][40, 2] = np.nan
    # maps: 0 one frame; 1 two posed frames; 2 no member; 3 the empty frame alone (no voxel); 4 the far frame; 5 four
    # members, the empty one among them; 6 frame 7 twice and the one-point frame
    members = [[2], [2, 7], [], [11], [17], [19, 7, 2, 11], [7, 7, 13]]
    map_off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    map_frame = np.array([f for m in members for f in m], np.uint32)
    pa, pb, pc = (vx.pose_row([0.1, 1.0, 0.2], 0.004, [0.01, -0.02, 0.005]), vx.pose_row([1.0, 0.0, 0.3], -0.003, [0.0, 0.015, -0.01]),
                  vx.pose_row([0.0, 0.0, 1.0], 0.002, [0.02, 0.0, 0.0]))
    map_pose = np.array([vx.EYE, vx.EYE, pa, vx.EYE, vx.EYE, pb, vx.EYE, pc, vx.EYE, vx.EYE, pa, vx.EYE])
    assert len(map_pose) == len(map_frame)
    near = ref.near_start(Rm, tm)
    src, tgt, init = [], [], []
    for a in range(len(calls)):
        for m in range(len(members)):
            src.append(a)
            tgt.append(m)
            init.append(near if (a + m) % 2 else vx.EYE)
    return calls, stored, map_off, map_frame, map_pose, src, tgt, np.array(init)


def test_mixed_batch_and_each_pair_alone(mods):
    h = mods[0].STDescManager()
    calls, stored, map_off, map_frame, map_pose, src, tgt, init = _mixed()
    sx.store(h, stored, k_neighbors=8)
    seen = set()
    for mode, limit in ((1, 2), (27, 1), (7, 64)):
        got, _ = svx.check(h, calls, stored, map_off, map_frame, map_pose, src, tgt, init, "mixed, mode %d, max_iterations %d" % (mode, limit),
                           k_neighbors=8, neighbor_mode=mode, max_iterations=limit)
        seen |= set(got["status"].tolist())
    assert seen == {vref.CONVERGED, vref.ITERATION_LIMIT, vref.NO_CORRESPONDENCE, vref.NO_POINTS}
    assert [len(m["n_points"]) for m in got["maps"]][2:4] == [0, 0] and len(got["maps"][5]["n_points"]) > 1
    status = dict(zip(zip(src, tgt), got["status"].tolist()))
    assert status[(2, 0)] == vref.NO_POINTS and status[(0, 2)] == vref.NO_POINTS and status[(0, 3)] == vref.NO_POINTS
    assert status[(0, 4)] == vref.NO_CORRESPONDENCE
    # each pair alone, with its map alone: the same bits as in the batch (got: the last, mode 7)
    for k in range(len(src)):
        m = tgt[k]
        lo, hi = int(map_off[m]), int(map_off[m + 1])
        one = svx.run(h, calls, [0, hi - lo], map_frame[lo:hi], map_pose[lo:hi], [src[k]], [0], init[k:k + 1], k_neighbors=8, neighbor_mode=7)
        for f in svx.FIELDS:
            assert ref.same(one[f][0], got[f][k]), (k, f)
        assert np.array_equal(one["matches"][0], got["matches"][k]) and vx.same_maps(one["maps"][0], got["maps"][m]), k
    h.close()


def test_null_map_pose_is_the_identity(mods):
    h = mods[0].STDescManager()
    s, t, Rm, tm = ref.planted_scene(200, 9)
    near = ref.near_start(Rm, tm)[None]
    stored = {3: t[:110], 8: t[90:], 9: np.zeros((0, 3), np.float32)}
    sx.store(h, stored, k_neighbors=8)
    opt = dict(k_neighbors=8, neighbor_mode=7)
    null, _ = svx.check(h, [s], stored, [0, 3], [3, 9, 8], None, [0], [0], near, "NULL map_pose", **opt)
    eye, _ = svx.check(h, [s], stored, [0, 3], [3, 9, 8], np.array([vx.EYE] * 3), [0], [0], near, "identity map_pose", **opt)
    vx.compare(eye, null, "identities against NULL")
    assert null["status"][0] == vref.CONVERGED
    h.close()


# ---- independence ----
def test_independence_views_and_shards(mods):
    """the stored voxel call's results and those of sgtd_register_clouds, sgtd_register_voxels and sgtd_register_stored do
    not touch each other; a pending batch is still there afterwards; a view with a store of its own and a multi-device
    handle give the plain handle's bits"""
    manager, synth = mods[:2]
    s, t, Rm, tm = ref.planted_scene(200, 4)
    s2, t2, _, _ = ref.planted_scene(150, 9)
    near = ref.near_start(Rm, tm)[None]
    dopt = dict(k_neighbors=10, max_corr_dist=2.0)
    vopt = dict(k_neighbors=10, neighbor_mode=7)
    single, multi, view = manager.STDescManager(), manager.STDescManager(devices=[0, 0]), manager.STDescManager()
    m = synth.make_map(12, 80, stream=5)
    single.add_frames(m.xyz, m.label)
    view.attach_table(single)
    before = single.query_frames(m.xyz[:3], m.label[:3])
    stored = {8: t[:120], 9: t[100:]}
    sx.store(single, stored, k_neighbors=10)
    dense = rx.run(single, [s2, t2], [0], [1], None, **dopt)
    voxel = vx.run(single, [s2, t2], [0, 1], [1], None, [0], [0], None, **vopt)
    kept = sx.run(single, [s2], [0], [8], None, **dopt)
    args = ([s], [0, 2], [8, 9], None, [0], [0], near)
    want = svx.run(single, *args, **vopt)
    assert want["status"][0] == vref.CONVERGED
    # the other calls' results are what they were
    again = single.result_registered()
    for f in rx.FIELDS:
        assert ref.same(again[f], dense[f]), f
    assert ref.same(single.register_covariances(1), dense["cov"][1]) and np.array_equal(single.register_matches(0)[0], dense["matches"][0][0])
    again = single.result_voxel_registered()
    assert all(ref.same(again[f], voxel[f]) for f in vx.FIELDS)
    assert vx.same_maps(single.voxel_map(0), voxel["maps"][0]) and np.array_equal(single.voxel_matches(0), voxel["matches"][0])
    sx.compare(sx.getters(single, single.result_stored_registered(), 1), kept, [0], "sgtd_register_stored's results")
    # and the other way round
    rx.run(single, [t2, s2], [1], [0], None, **dopt)
    vx.run(single, [t2, s2], [0, 1], [0], None, [1], [0], None, **vopt)
    sx.run(single, [t2], [0], [9], None, **dopt)
    vx.compare(svx.getters(single, single.result_stored_voxel_registered(), 1), want, "after the other calls")
    # later set calls do not change the results either
    single.set_frame_clouds([8], [s2], k_neighbors=10)
    vx.compare(svx.getters(single, single.result_stored_voxel_registered(), 1), want, "after a set call")
    # the batch is still there
    after = single.results()
    assert np.array_equal(before.cand_frame, after.cand_frame) and np.array_equal(before.n_cand, after.n_cand)
    # a view has a store of its own; a multi-device handle keeps it on its first device
    assert view.frame_clouds_info()["n_frames"] == 0
    for h in (view, multi):
        sx.store(h, stored, k_neighbors=10)
        vx.compare(svx.run(h, *args, **vopt), want, "view / shards")
    view.close()
    multi.close()
    single.close()


def test_stage_times(mods):
    h = mods[0].STDescManager()
    s, t, _, _ = ref.planted_scene(300, 7)
    h.set_frame_clouds([1], [t], k_neighbors=10)
    args = ([s], [0, 1], [1], None, [0], [0], None)
    plain = svx.run(h, *args, k_neighbors=10, neighbor_mode=7)
    assert h.stored_voxel_register_stage_ms() == (0.0, 0.0, 0.0, 0.0, 0.0)
    h.set_timing(True)
    try:
        timed = svx.run(h, *args, k_neighbors=10, neighbor_mode=7)
        ms = h.stored_voxel_register_stage_ms()
    finally:
        h.set_timing(False)
    assert all(v > 0.0 for v in ms) and ms[4] >= max(ms[:4])
    vx.compare(timed, plain, "timed")
    h.close()


# ---- error handling ----
def test_errors_keep_the_earlier_results(mods):
    manager, _, _lib = mods
    h = manager.STDescManager()
    L = h._L
    n64 = C.c_int64(0)
    buf = np.zeros(16)
    # the getters before a run
    assert L.sgtd_result_stored_voxel_registered(h._h, _ptr(buf), None, None, None, None, None, None) == -7
    assert L.sgtd_result_stored_voxel_map(h._h, 0, None, None, None, None, 0, C.byref(n64)) == -7
    assert L.sgtd_result_stored_voxel_matches(h._h, 0, None, 0, C.byref(n64)) == -7
    assert L.sgtd_stored_voxel_register_stage_ms(h._h, None, None, None, None, None) == -7
    s, t, _, _ = ref.planted_scene(150, 2)
    stored = {6: t, 3: t[:40]}
    sx.store(h, stored, k_neighbors=8)
    first = svx.run(h, [s], [0, 1], [6], None, [0], [0], None, k_neighbors=8, neighbor_mode=7)
    # a sgtd_register_voxels run on the same handle: the getters of the two calls must not be mixed up
    other = vx.run(h, [s[:50], t[:60]], [0, 1], [1], None, [0], [0], None, k_neighbors=8, neighbor_mode=1)
    pts, off = rx.pack([s])
    moff, mfr = np.array([0, 1], np.int32), np.array([6], np.uint32)
    src, tgt = np.array([0], np.int32), np.array([0], np.int32)
    eye = vx.EYE[None].copy()

    def raw(pts=pts, off=off, moff=moff, mfr=mfr, src=src, tgt=tgt, mpose=None, init=None, opt=None, stride=3, n_clouds=None, n_maps=None,
            n_pairs=None):
        return L.sgtd_register_stored_voxels(h._h, None if opt is None else C.byref(opt), _ptr(pts), stride, _ptr(off),
                                             len(off) - 1 if n_clouds is None else n_clouds, _ptr(moff), _ptr(mfr), _ptr(mpose),
                                             len(moff) - 1 if n_maps is None else n_maps, _ptr(src), _ptr(tgt), _ptr(init),
                                             len(src) if n_pairs is None else n_pairs, 0)

    def options(**kw):
        o = _lib.VoxelRegisterOptions()
        L.sgtd_default_voxel_register_options(C.byref(o))
        o.k_neighbors, o.neighbor_mode = 8, 7
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    bad = [
        dict(n_clouds=-1), dict(n_pairs=-1), dict(n_maps=-1), dict(stride=2), dict(stride=5),
        dict(pts=None), dict(off=None, n_clouds=1), dict(src=None, n_pairs=1), dict(tgt=None), dict(moff=None, n_maps=1), dict(mfr=None),
        dict(off=np.array([1, 150], np.int64)), dict(off=np.array([0, 150, 100], np.int64)),
        dict(moff=np.array([1, 1], np.int32)), dict(moff=np.array([0, 1, 0], np.int32), tgt=np.array([0], np.int32)),
        dict(src=np.array([1], np.int32)), dict(src=np.array([-1], np.int32)), dict(tgt=np.array([1], np.int32)), dict(tgt=np.array([-1], np.int32)),
    ]
    for v in (np.nan, np.inf, -np.inf):
        p = eye.copy()
        p[0, 4] = v
        bad.append(dict(init=p))
        bad.append(dict(mpose=p))
    for field, values in (("max_iterations", (0, -3)), ("lm_max_trials", (0,)), ("reserved", (1,)), ("k_neighbors", (2, 33)),
                          ("voxel_resolution", (0.0, -1.0, np.nan, np.inf)), ("neighbor_mode", (0, 2, 6, 26, 28, -1)),
                          ("lm_init_lambda_factor", (0.0, np.nan)), ("rotation_eps", (0.0, np.nan)), ("translation_eps", (0.0, np.inf)),
                          ("plane_eps", (0.0, np.nan))):
        bad += [dict(opt=options(**{field: v})) for v in values]
    assert raw(opt=options()) == 0
    first = svx.getters(h, h.result_stored_voxel_registered(), 1)
    for kw in bad:
        assert raw(**kw) == -1, kw
    # a member without a cloud: SGTD_ERR_INVALID, and the handle says which (the last id of the table, and one beyond it)
    for missing in (4, 7, 1 << 20):
        assert raw(mfr=np.array([missing], np.uint32), opt=options()) == -1
        assert ("frame %d has no stored cloud" % missing).encode() in L.sgtd_last_error(h._h)
    # the store's settings: SGTD_ERR_STATE
    assert raw(opt=options(k_neighbors=9)) == -7 and b"cloud store's" in L.sgtd_last_error(h._h)
    assert raw(opt=options(plane_eps=2e-3)) == -7
    assert raw() == -7      # (the defaults: k_neighbors 20)
    # the caps, from the offsets alone (the checks come before every read)
    o8 = options()
    big = np.array([0, (1 << 17) + 1], np.int64)
    assert raw(off=big, opt=o8) == -6 and b"points a cloud" in L.sgtd_last_error(h._h)
    assert raw(moff=np.zeros(65537, np.int32), opt=o8) == -6 and b"SGTD_VREG_MAX_MAPS" in L.sgtd_last_error(h._h)
    n_mem = (1 << 25) // 150 + 1
    assert raw(moff=np.array([0, n_mem], np.int32), mfr=np.full(n_mem, 6, np.uint32), opt=o8) == -6
    assert b"SGTD_VREG_MAX_MEMBER_POINTS" in L.sgtd_last_error(h._h)
    full = np.array([0, 1 << 17], np.int64)
    nsrc = (1 << 26) // 27 // (1 << 17) + 1
    assert raw(off=full, src=np.zeros(nsrc, np.int32), tgt=np.zeros(nsrc, np.int32), opt=options(neighbor_mode=27)) == -6
    assert b"SGTD_VREG_MAX_CORR" in L.sgtd_last_error(h._h)
    # the earlier results are all still there, and so are sgtd_register_voxels'
    vx.compare(svx.getters(h, h.result_stored_voxel_registered(), 1), first, "after the failed calls")
    again = h.result_voxel_registered()
    assert all(ref.same(again[f], other[f]) for f in vx.FIELDS) and vx.same_maps(h.voxel_map(0), other["maps"][0])
    assert np.array_equal(h.voxel_matches(0), other["matches"][0])
    # too small a capacity: the size needed, the first entries written
    nv = len(first["maps"][0]["n_points"])
    assert nv > 4
    coord, cnt, mean, cov = np.full((10, 3), -9, np.int32), np.full(10, -9, np.int32), np.full((10, 3), -7.0), np.full((10, 3, 3), -7.0)
    assert L.sgtd_result_stored_voxel_map(h._h, 0, _ptr(coord), _ptr(cnt), _ptr(mean), _ptr(cov), 4, C.byref(n64)) == -4 and n64.value == nv
    assert np.array_equal(coord[:4], first["maps"][0]["coord"][:4]) and (coord[4:] == -9).all()
    assert np.array_equal(cnt[:4], first["maps"][0]["n_points"][:4]) and (cnt[4:] == -9).all()
    assert ref.same(mean[:4], first["maps"][0]["mean"][:4]) and (mean[4:] == -7.0).all()
    assert ref.same(cov[:4], first["maps"][0]["cov"][:4]) and (cov[4:] == -7.0).all()
    j = np.full(20, -9, np.int32)
    assert L.sgtd_result_stored_voxel_matches(h._h, 0, _ptr(j), 6, C.byref(n64)) == -4 and n64.value == 150 * 7
    assert np.array_equal(j[:6], first["matches"][0][:6]) and (j[6:] == -9).all()
    assert L.sgtd_result_stored_voxel_map(h._h, 1, None, None, None, None, 0, C.byref(n64)) == -1
    assert L.sgtd_result_stored_voxel_map(h._h, -1, None, None, None, None, 0, C.byref(n64)) == -1
    assert L.sgtd_result_stored_voxel_matches(h._h, 1, None, 0, C.byref(n64)) == -1
    assert L.sgtd_result_stored_voxel_matches(h._h, 0, None, -1, C.byref(n64)) == -1
    # no pair at all is a run: the maps are built, no pair comes back; no map at all is one too
    out = h.register_stored_voxels(pts, off, moff, mfr, None, [], [], k_neighbors=8)
    assert out["pose"].shape == (0, 12) and vx.same_maps(h.stored_voxel_map(0), first["maps"][0])
    out = h.register_stored_voxels(pts, off, [0], [], None, [], [], k_neighbors=8)
    assert out["pose"].shape == (0, 12)
    h.close()
