"""sgtd_register_stored_local_loops on a small verified batch: the rows, maps, members and member poses formed on the device
against the numpy restatement of the header's rule (tests/_stored_voxel_ref.py), and the results against
sgtd_register_stored_voxels on those maps and rows, bit for bit, through every getter.  Frames with a cloud but no pose, a pose
but no cloud or a pose that is not finite; a frame exactly at d2 == rr and the next representable distance beyond; equal d2 at
the max_members cut; more eligible frames than a workgroup has threads among a few thousand ids; every max_per_query, start and
state error."""
import ctypes as C

import numpy as np
import pytest

import _register_ref as ref
import _stored_voxel_edges as svx
import _stored_voxel_ref as sv
import _voxel_register_edges as vx
import _voxel_register_ref as vref

pytestmark = pytest.mark.gpu

OPT = dict(k_neighbors=10, max_iterations=30, neighbor_mode=7)
NO_CLOUD, NO_POSE, BAD_POSE = (4, 10), (12,), (6,)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def batch():
    """test_register_loops_stored's map and batch, verified; every frame's thinned cloud but NO_CLOUD's is stored, every frame's
    pose but NO_POSE's, and BAD_POSE's has a float that is not finite"""
    from sgtd_amd import ingest, manager, synth
    cfg = {"min_seg": [20] * 32}
    p, l, off, poses = synth.make_posed_scans(20, 6000, stream=33, spacing=2.0, n_blobs=60, sensor_range=40.0, sigma=(0.05, 0.12))
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
    clouds = {f: ingest.voxel_downsample(p[off[f]:off[f + 1], :3], 0.25) for f in range(20) if f not in NO_CLOUD}
    clouds[20] = clouds[3].copy()
    h.set_frame_clouds(list(clouds), [clouds[f] for f in clouds], k_neighbors=10)
    stored = {f: np.asarray(poses[min(f, 19) if f != 20 else 3], np.float32).reshape(12).copy() for f in range(21) if f not in NO_POSE}
    stored[BAD_POSE[0]][5] = np.inf
    thin = [ingest.voxel_downsample(qp[qo[q]:qo[q + 1], :3], 0.25) for q in range(3)]
    tq = np.concatenate(thin)
    to = np.concatenate([[0], np.cumsum([len(c) for c in thin])]).astype(np.int64)
    h.verify()
    b = dict(h=h, manager=manager, cn=cn, res=res, clouds=clouds, poses=stored, true_poses=dict(stored), thin=thin, tq=tq, to=to)
    yield b
    h.close()


def _set_poses(b, poses):
    h = b["h"]
    h.set_frame_poses(None, None)
    ids = sorted(poses)
    h.set_frame_poses(np.array(ids, np.int64), np.array([poses[i] for i in ids], np.float32))
    b["poses"] = poses


def _stage(b, start):
    """score, n_cand, cand_frame and the named stage's relative poses, per query"""
    h, res = b["h"], b["res"]
    score, rel = [], []
    for q in range(3):
        s, rot, t = h.result_verify(q)
        if start != "verify":
            r = h.result_refined(q) if start == "refined" else h.result_aligned(q)
            rot, t = r["rot"], r["t"]
        score.append(s)
        rel.append([np.concatenate([rot[c].reshape(9), t[c]]) for c in range(len(s))])
    return score, res.n_cand, res.cand_frame, rel


def _check(b, start="verify", max_per_query=5, radius=5.0, max_members=0, what="", dev=False):
    """one call against the restatement (rows, maps, members, poses) and against register_stored_voxels on those maps and rows"""
    h = b["h"]
    tq = b["tq"]
    if dev:
        import torch
        tq = torch.from_numpy(tq).cuda()
    out = h.register_loops_local_stored(tq, b["to"], radius=radius, max_members=max_members, max_per_query=max_per_query, start=start, **OPT)
    svx.getters(h, out, len(out["map_frames"]))
    score, n_cand, cand_frame, rel = _stage(b, start)
    want = sv.form(score, n_cand, cand_frame, rel, max_per_query, b["cn"], set(b["clouds"]), b["poses"], radius, max_members)
    for f in ("query", "cand", "frame", "tgt_map"):
        assert out[f].tolist() == want[f].tolist(), (what, f, out[f], want[f])
    assert ref.same(out["init"], want["init"]), what
    assert out["map_frames"] == want["map_frames"], what
    assert [m.tolist() for m in out["members"]] == want["members"], (what, out["members"], want["members"])
    assert np.array_equal(out["map_off"], want["map_off"]) and np.array_equal(out["map_frame"], want["map_frame"]), what
    assert ref.same(out["map_pose"], want["map_pose"]), what
    if len(want["query"]):
        direct = svx.run(h, b["thin"], want["map_off"], want["map_frame"], want["map_pose"], want["query"], want["tgt_map"], want["init"], **OPT)
        vx.compare(out, direct, what + " (register_stored_voxels)")
    else:
        assert out["pose"].shape == (0, 12) and out["map_frames"] == []
    return out, want


def test_state_errors_come_first():
    """on a handle of its own: the order of the tests and the module's batch do not matter"""
    from sgtd_amd import manager, synth
    h = manager.STDescManager()
    m = synth.make_map(12, 80, stream=5)
    h.add_frames(m.xyz, m.label)
    s, t, _, _ = ref.planted_scene(150, 2)
    h.set_frame_clouds([3], [t], k_neighbors=10)
    tq = np.concatenate([s, s[:100], s[:50]])
    to = np.array([0, 150, 250, 300], np.int64)
    L = h._L
    n = C.c_int64(0)
    assert L.sgtd_register_stored_local_loops(h._h, None, _ptr(tq), 3, _ptr(to), 4, 0, 5.0, 0, 0) == -7      # no batch at all
    h.query_frames(m.xyz[:3], m.label[:3])
    with pytest.raises(manager.SgtdError) as err:
        h.register_loops_local_stored(tq, to, **OPT)                         # before verify()
    assert err.value.status == -7 and "sgtd_verify" in str(err.value)
    h.verify()
    for start in ("refined", "aligned"):
        with pytest.raises(manager.SgtdError) as err:
            h.register_loops_local_stored(tq, to, start=start, **OPT)      # the stage has not run on this batch
        assert err.value.status == -7
    with pytest.raises(manager.SgtdError) as err:
        h.register_loops_local_stored(tq, to, **dict(OPT, k_neighbors=11))  # not the store's settings
    assert err.value.status == -7
    assert L.sgtd_result_stored_local_pairs(h._h, None, None, None, None, None, 0, C.byref(n)) == -7
    # the raw call's own argument errors
    for args in ((-1, 0, 5.0, 0), (4, 3, 5.0, 0), (4, -1, 5.0, 0), (4, 0, -1.0, 0), (4, 0, np.nan, 0), (4, 0, np.inf, 0), (4, 0, 5.0, -1)):
        assert L.sgtd_register_stored_local_loops(h._h, None, _ptr(tq), 3, _ptr(to), args[0], args[1], args[2], args[3], 0) == -1, args
    # no frame has a pose: the call runs and forms no row
    out = h.register_loops_local_stored(tq, to, **OPT)
    assert out["pose"].shape == (0, 12) and out["map_frames"] == [] and len(out["query"]) == 0
    # after the explicit form the rows and maps are not there
    out = svx.run(h, [s], [0, 1], [3], None, [0], [0], None, **OPT)
    assert len(out["status"]) == 1
    assert L.sgtd_result_stored_local_pairs(h._h, None, None, None, None, None, 0, C.byref(n)) == -7
    assert L.sgtd_result_stored_local_maps(h._h, None, None, None, None, 0, 0, C.byref(n), C.byref(n)) == -7
    h.close()


def test_rows_maps_members_and_results(batch):
    h, cn = batch["h"], batch["cn"]
    _set_poses(batch, batch["true_poses"])
    before = h.results()
    # what the cases rely on: taken candidates whose frame is not eligible, of every kind, and such frames in reach of a map
    score, n_cand, cand_frame, rel = _stage(batch, "verify")
    every = sv.rows(score, n_cand, cand_frame, rel, cn, cn, set(range(21)))
    taken = set(r[2] for r in every)
    print("frames of the verified candidates:", sorted(taken))
    assert taken & set(NO_CLOUD) and len(every) > 6, "no verified candidate's frame is without a cloud"
    for start in ("verify", "refined", "aligned"):
        if start == "refined":
            h.refine_poses()
        if start == "aligned":
            h.align_keypoints(1.0)
        for mpq in (0, 1, 4, cn + 1):
            out, want = _check(batch, start, mpq, 5.0, 0, "%s, max_per_query %d" % (start, mpq), dev=mpq == 1)
            assert not set(out["frame"].tolist()) & set(NO_CLOUD + NO_POSE + BAD_POSE)
            for m in out["members"]:
                assert not set(m.tolist()) & set(NO_CLOUD + NO_POSE + BAD_POSE)
    assert len(out["query"]) >= 3 and any(len(m) > 1 for m in out["members"]), "the batch says too little"
    print("status of the rows, no cap:", out["status"].tolist(), "iterations:", out["iterations"].tolist())
    assert (out["status"] == vref.CONVERGED).any(), "no pair converges"
    # the frames that are not eligible lie within reach of some map's frame: they were left out, not merely far
    t = {f: np.asarray(batch["true_poses"].get(f, np.zeros(12)), np.float64)[[3, 7, 11]] for f in range(21)}
    near = [f for f in NO_CLOUD + BAD_POSE for j in out["map_frames"] if np.linalg.norm(t[f] - t[j]) <= 5.0]
    assert near, "no ineligible frame is within reach of a map"
    # the cut: max_members 1, 2 and 3 against no cap
    for m in (1, 2, 3):
        cut, _ = _check(batch, "verify", 4, 5.0, m, "max_members %d" % m)
        assert max(len(x) for x in cut["members"]) == m
    print("status of the rows, max_members 3:", cut["status"].tolist(), "iterations:", cut["iterations"].tolist())
    assert (cut["status"] == vref.CONVERGED).any(), "no pair converges"
    # the getters' capacities (_check's register_stored_voxels call has replaced the results: the loops form runs again)
    again = h.register_loops_local_stored(batch["tq"], batch["to"], radius=5.0, max_members=3, max_per_query=4, **OPT)
    assert all(ref.same(again[f], cut[f]) for f in vx.FIELDS)
    L = h._L
    n, k = C.c_int64(0), C.c_int64(0)
    q = np.full(2, -9, np.int32)
    assert L.sgtd_result_stored_local_pairs(h._h, _ptr(q), None, None, None, None, 1, C.byref(n)) == -4 and n.value == len(cut["query"])
    assert q.tolist() == [int(cut["query"][0]), -9]
    mf, mem = np.full(2, 77, np.uint32), np.full(2, 77, np.uint32)
    assert L.sgtd_result_stored_local_maps(h._h, _ptr(mf), None, _ptr(mem), None, 1, 1, C.byref(n), C.byref(k)) == -4
    assert (n.value, k.value) == (len(cut["map_frames"]), len(cut["map_frame"])) and mf.tolist() == [cut["map_frames"][0], 77]
    assert mem.tolist() == [int(cut["map_frame"][0]), 77]
    # the batch is untouched
    after = h.results()
    assert np.array_equal(before.cand_frame, after.cand_frame) and np.array_equal(before.n_cand, after.n_cand)


def _edges_of_the_rule(batch, added):
    h = batch["h"]
    _set_poses(batch, batch["true_poses"])
    first, _ = _check(batch, "verify", 2, 5.0, 0, "the rows")
    j0 = int(first["frame"][0])
    f32 = np.float32
    # every map frame far from every other; the helpers around j0 at (1000 * j0, 0, 0)
    poses = {}
    for f in range(21):
        if f in NO_POSE:
            continue
        p = batch["true_poses"][f].copy()
        p[[3, 7, 11]] = [1000.0 * f, 0.0, 0.0]
        poses[f] = p
    base = poses[j0].copy()

    def at(dx, dy, dz):
        p = base.copy()
        p[[3, 7, 11]] = [f32(1000.0 * j0) + f32(dx), f32(dy), f32(dz)]
        return p

    helpers = {30: at(3, 4, 0),                                       # d2 == rr: in
               31: at(3, np.nextafter(f32(4), f32(9)), 0),           # the next float beyond: out
               32: at(0, 1, 0), 33: at(1, 0, 0), 34: at(0, 0, -1),   # equal d2 = 1: the smaller ids win the cut
               35: at(0, 0.5, 0),                                     # the nearest
               36: at(0, 0, 6), 37: at(np.nan, 0, 0)}                 # out of reach; not finite
    poses.update(helpers)
    tiny = batch["clouds"][j0][:40]
    added += list(helpers)
    h.set_frame_clouds(list(helpers), [tiny[k::8] for k in range(len(helpers))], k_neighbors=10)
    clouds = dict(batch["clouds"])
    clouds.update({f: None for f in helpers})
    batch["clouds"] = clouds
    _set_poses(batch, poses)
    out, want = _check(batch, "verify", 2, 5.0, 0, "by hand, no cap")
    mem = out["members"][out["map_frames"].index(j0)].tolist()
    assert mem == [j0, 30, 32, 33, 34, 35], mem
    print("status of the rows, by hand:", out["status"].tolist(), "iterations:", out["iterations"].tolist())
    assert (out["status"] == vref.CONVERGED).any(), "no pair converges"
    for m, kept in ((2, [35]), (3, [32, 35]), (4, [32, 33, 35]), (5, [32, 33, 34, 35]), (6, [30, 32, 33, 34, 35]), (7, [30, 32, 33, 34, 35])):
        out, _ = _check(batch, "verify", 2, 5.0, m, "by hand, max_members %d" % m)
        assert out["members"][out["map_frames"].index(j0)].tolist() == [j0] + kept, (m, out["members"])
    # radius 0 keeps a frame at the very same position, and nothing else
    poses[38] = at(0, 0, 0)
    added.append(38)
    h.set_frame_clouds([38], [tiny[:3]], k_neighbors=10)
    batch["clouds"][38] = None
    _set_poses(batch, poses)
    out, _ = _check(batch, "verify", 2, 0.0, 0, "radius 0")
    assert out["members"][out["map_frames"].index(j0)].tolist() == [j0, 38]
    # 400 frames of empty clouds within reach, ids 1000 .. 1399, their distances drawn from 50 values (ties everywhere);
    # poses without clouds up to id 5000 and a cloud without a pose at 6000 stretch the tables
    rng = np.random.default_rng(5)
    many = {1000 + k: at(0, 0, 0.05 * (1 + rng.integers(0, 50))) for k in range(400)}
    poses.update(many)
    poses.update({f: at(0.1, 0.1, 0.1) for f in range(2000, 5001, 7)})
    empty = np.zeros((0, 3), np.float32)
    added += list(many) + [6000]
    h.set_frame_clouds(list(many) + [6000], [empty] * 401, k_neighbors=10)
    batch["clouds"].update({f: None for f in list(many) + [6000]})
    _set_poses(batch, poses)
    out, _ = _check(batch, "verify", 2, 5.0, 0, "400 in reach")
    assert len(out["members"][out["map_frames"].index(j0)]) == 1 + 6 + 400
    for m in (2, 257, 300, 406):
        out, _ = _check(batch, "verify", 2, 5.0, m, "400 in reach, max_members %d" % m)
        assert len(out["members"][out["map_frames"].index(j0)]) == m
    print("status of the rows, 400 in reach:", out["status"].tolist(), "iterations:", out["iterations"].tolist())
    assert (out["status"] == vref.CONVERGED).any(), "no pair converges"


def test_members_at_the_edges_of_the_rule(batch):
    """poses placed by hand around the first row's frame j0: a frame at d2 == rr and one a float beyond, equal d2 at the cut,
    and 400 frames of empty clouds within reach among ids up to 6000 (more than a workgroup's threads; the select's digits)"""
    clouds, added = batch["clouds"], []
    try:
        _edges_of_the_rule(batch, added)
    finally:      # the module's batch as it was: the helpers' clouds forgotten, the true poses back
        if added:
            batch["h"].set_frame_clouds(added, None)
        batch["clouds"] = clouds
        _set_poses(batch, batch["true_poses"])
