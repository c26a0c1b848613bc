#!/usr/bin/env python3
"""sgtd_register_stored_voxels beside sgtd_register_voxels, on tools/voxel_register_bench.py's local-map legs: one query
cloud (tests/_register_ref.planted_scene) registered from a start 0.13 m / 0.9 degrees off against `maps` local maps of
`scans` posed scans each, every scan a cloud of its own, posed a few centimetres and a fraction of a degree off one another.

sgtd_register_voxels gets the query and every member cloud in one device array and computes all their covariances in the
call; for sgtd_register_stored_voxels the member clouds are stored once (sgtd_set_frame_clouds, timed apart) and the call
gets the query cloud alone.  The two calls alternate in one run on the same inputs, and every result is asserted to agree bit
for bit: the result rows, every voxel of every map, every match.  For every configuration: the wall time of the whole call
with the points on the device (host waits included), the device time by stage under sgtd_set_timing (the events serialise the
call), and the one-off time of storing the members.  Prints one JSON line per configuration; warm-up first, then --reps timed
calls.  The lines replace what --out held.

usage: tools/stored_voxel_register_bench.py [--sizes 2048,8192,32768] [--scans 10,30] [--maps 1,8] [--modes 1,7] [--reps 3]
                                             [--out profiles/stored_voxel_register_bench_mi355x.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MAX_TOTAL_POINTS = 1 << 25
FIELDS = ("pose", "fitness", "cost", "n_matched", "n_corr", "iterations", "status")
MAP_FIELDS = ("coord", "n_points", "mean", "cov")
STAGES = ("covariances", "map_build", "correspondences", "sums_control", "total")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,8192,32768")
    ap.add_argument("--scans", default="10,30", help="posed scans per local map")
    ap.add_argument("--maps", default="1,8", help="local maps per call")
    ap.add_argument("--modes", default="1,7")
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loops", type=int, default=1, help="1: also the loops form on a small verified batch beside register_loops_local")
    ap.add_argument("--distinct", type=int, default=4, help="distinct draws of the map cloud (repeated to as many clouds as needed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stored_voxel_register_bench_mi355x.jsonl"),
                    help="the file the lines are written to, replacing what it held ('' = none)")
    a = ap.parse_args()
    import torch
    import _register_ref as ref
    from sgtd_amd import manager

    g = manager.STDescManager()
    stat = lambda v: {"min": round(min(v), 3), "median": round(float(np.median(v)), 3), "n": len(v)}      # noqa: E731
    ints = lambda s: [int(x) for x in s.split(",") if x]                                                 # noqa: E731

    if a.out:
        open(a.out, "w").close()      # (a run's lines replace the file's: a second run does not double them)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def timed(call, stage_ms):
        g.set_timing(True)
        call()
        ms = stage_ms()
        g.set_timing(False)
        return {k: round(v, 3) for k, v in zip(STAGES, ms)}

    for size in ints(a.sizes):
        draws = []
        for d in range(a.distinct):
            s, t, Rm, tm = ref.planted_scene(size, 100 + d)
            draws.append((s, t[:size]))
        near = ref.near_start(Rm, tm)
        query = torch.from_numpy(draws[0][0]).cuda()
        qoff = np.array([0, size], np.int64)
        rng = np.random.default_rng(size)
        for scans in ints(a.scans):
            for maps in ints(a.maps):
                members = maps * scans
                rec = {"run": "stored_voxel_register", "target": "local", "pairs": maps, "maps": maps, "scans_per_map": scans,
                       "points_per_cloud": size, "stored_frames": members}
                if (members + 1) * size > MAX_TOTAL_POINTS:
                    rec["error"] = "beyond sgtd_register_voxels' caps: %d points in all" % ((members + 1) * size)
                    emit(rec)
                    continue
                clouds = [draws[k % a.distinct][1] for k in range(members)]
                off = np.arange(members + 2, dtype=np.int64) * size
                map_off = np.arange(maps + 1, dtype=np.int32) * scans
                map_cloud = 1 + np.arange(members, dtype=np.int32)
                map_frame = np.arange(members, dtype=np.uint32)
                pose = np.zeros((members, 12))
                for k in range(members):
                    pose[k, :9] = ref.rot_axis(rng.normal(0, 1, 3), np.deg2rad(0.2) * rng.uniform(-1, 1)).reshape(9)
                    pose[k, 9:] = rng.normal(0, 0.03, 3)
                src, tgt_map = np.zeros(maps, np.int32), np.arange(maps, dtype=np.int32)
                init = np.repeat(near[None], maps, 0)
                pts = torch.from_numpy(np.concatenate([draws[0][0]] + clouds)).cuda()
                # the members are stored once: the store is emptied first, so the time is that of a map that arrives
                g.set_frame_clouds(None, None)
                t0 = time.perf_counter()
                g.set_frame_clouds(map_frame, (pts[size:], off[1:] - size), k_neighbors=20)
                rec["ms_wall_set_frame_clouds"] = round((time.perf_counter() - t0) * 1e3, 3)
                for mode in ints(a.modes):
                    vopt = dict(k_neighbors=20, neighbor_mode=mode, voxel_resolution=a.resolution)
                    r = dict(rec, options=vopt)
                    calls = {"voxels": lambda: g.register_voxels(pts, off, map_off, map_cloud, pose, src, tgt_map, init, **vopt),
                             "stored": lambda: g.register_stored_voxels(query, qoff, map_off, map_frame, pose, src, tgt_map, init, **vopt)}
                    wall, res = {"voxels": [], "stored": []}, {}
                    for i in range(1 + a.reps):                     # warm-up first; the two calls alternate
                        for name, call in calls.items():
                            t0 = time.perf_counter()
                            res[name] = call()
                            if i:
                                wall[name].append((time.perf_counter() - t0) * 1e3)
                    # bit for bit: the rows, every voxel of every map, every match
                    for f in FIELDS:
                        assert ref.same(res["stored"][f], res["voxels"][f]), "%s differs: %r" % (f, r)
                    voxels = 0
                    for m in range(maps):
                        va, vb = g.stored_voxel_map(m), g.voxel_map(m)
                        voxels += len(va["n_points"])
                        for f in MAP_FIELDS:
                            assert ref.same(va[f], vb[f]), "%s of map %d differs: %r" % (f, m, r)
                    for k in range(maps):
                        assert np.array_equal(g.stored_voxel_matches(k), g.voxel_matches(k)), "matches of pair %d differ: %r" % (k, r)
                    r["bit_for_bit"] = True
                    it = res["stored"]["iterations"]
                    r.update(voxels=voxels, iterations={"min": int(it.min()), "max": int(it.max()), "sum": int(it.sum())},
                             status_counts=np.bincount(res["stored"]["status"], minlength=5).tolist(),
                             ms_wall={k: stat(v) for k, v in wall.items()},
                             ms_timed={"voxels": timed(calls["voxels"], g.voxel_register_stage_ms),
                                       "stored": timed(calls["stored"], g.stored_voxel_register_stage_ms)})
                    r["wall_stored_over_voxels"] = round(r["ms_wall"]["stored"]["median"] / r["ms_wall"]["voxels"]["median"], 4)
                    emit(r)
                del pts
    g.close()
    if a.loops:
        loops_leg(a, emit, stat)


def loops_leg(a, emit, stat):
    """the loops form on a small verified batch (20 posed scans of 6000 points, 3 queries) beside register_loops_local, which
    gathers clouds and poses on the host and sends them with every call; both calls get the query points from the host, so
    the difference is the map side's.  No cap on the members, where the two rules agree
    on membership; the member poses differ in their last bits (f64 poses composed on the host there, the stored f32 poses
    composed on the device here), so rows and members are asserted equal and the results are not compared"""
    from sgtd_amd import ingest, manager, synth
    cfg = {"min_seg": [20] * 32}
    p, l, off, poses = synth.make_posed_scans(20, 6000, stream=33, spacing=2.0, n_blobs=60, sensor_range=40.0, sigma=(0.05, 0.12))
    h = manager.STDescManager()
    h.add_scans(p, l, off, cfg)
    rng = np.random.default_rng(6)
    picks = [3, 9, 15]
    qp = np.concatenate([p[off[f]:off[f + 1]] for f in picks]).copy()
    qp[:, :3] += rng.normal(0.0, 0.01, (len(qp), 3)).astype(np.float32)
    ql = np.concatenate([l[off[f]:off[f + 1]] for f in picks])
    qo = np.arange(4, dtype=np.int64) * 6000
    h.query_scans(qp, ql, qo, cfg)
    h.verify()
    poses = np.asarray(poses, np.float32).reshape(20, 12)
    T = poses.astype(np.float64).reshape(20, 3, 4)
    frame_poses = [np.concatenate([T[f][:, :3].reshape(9), T[f][:, 3]]) for f in range(20)]
    map_clouds = {f: ingest.voxel_downsample(p[off[f]:off[f + 1], :3], 0.25) for f in range(20)}
    thin = [ingest.voxel_downsample(qp[qo[q]:qo[q + 1], :3], 0.25) for q in range(3)]
    tq = np.concatenate(thin)
    to = np.concatenate([[0], np.cumsum([len(c) for c in thin])]).astype(np.int64)
    t0 = time.perf_counter()
    h.set_frame_poses(np.arange(20, dtype=np.int64), poses)
    h.set_frame_clouds(list(map_clouds), [map_clouds[f] for f in map_clouds], k_neighbors=10)
    set_ms = (time.perf_counter() - t0) * 1e3
    opt = dict(k_neighbors=10, max_iterations=5, neighbor_mode=7)
    calls = {"register_loops_local": lambda: h.register_loops_local(tq, to, map_clouds, frame_poses, radius=5.0, max_members=0, max_per_query=4, **opt),
             "register_loops_local_stored": lambda: h.register_loops_local_stored(tq, to, radius=5.0, max_members=0, max_per_query=4, **opt)}
    wall, res = {k: [] for k in calls}, {}
    for i in range(1 + a.reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            res[name] = call()
            if i:
                wall[name].append((time.perf_counter() - t0) * 1e3)
    x, y = res["register_loops_local"], res["register_loops_local_stored"]
    for f in ("query", "cand", "frame", "tgt_map"):
        assert np.array_equal(x[f], y[f]), f
    assert x["map_frames"] == y["map_frames"] and [m.tolist() for m in x["members"]] == [m.tolist() for m in y["members"]]
    emit({"run": "stored_voxel_register", "target": "loops", "queries": 3, "map_frames": 20, "rows": int(len(y["query"])), "maps": len(y["map_frames"]),
          "members": int(len(y["map_frame"])), "query_points": int(len(tq)), "query_points_from": "host, both calls", "map_points": int(sum(len(c) for c in map_clouds.values())), "options": opt,
          "rows_and_members_agree": True, "ms_wall_set_poses_and_clouds": round(set_ms, 3), "ms_wall": {k: stat(v) for k, v in wall.items()},
          "status_counts": np.bincount(y["status"], minlength=5).tolist()})
    h.close()


if __name__ == "__main__":
    main()
