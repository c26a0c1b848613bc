#!/usr/bin/env python3
"""sgtd_register_voxels on synthetic surfaces, by tools/register_bench.py's scenes and method: one query cloud
(tests/_register_ref.planted_scene) registered from a start 0.13 m / 0.9 degrees off against

  single  `pairs` voxel maps of one scan each, every scan a cloud of its own (so every one gets its covariances; where
          that passes the caps on all points, the maps share --distinct clouds and the line says so), and, in the same run
          with the two calls alternating, sgtd_register_clouds on the same (query, scan) pairs;
  local   `maps` local maps of `scans` posed scans each, every scan a cloud of its own, posed a few centimetres and a
          fraction of a degree off one another.

For every configuration: the wall time of the whole call with the points on the device (host waits included), the device
time by stage under sgtd_set_timing (the events serialise the call), iteration counts, and the time of a device-to-device
copy of the inputs as the floor.  corr_over_search is the voxel call's correspondence stage over sgtd_register_clouds'
search stage, as timed.  A configuration beyond a call's caps is recorded as such.  Prints one JSON line per
configuration; warm-up first, then --reps timed calls.  It measures and does not check.

usage: tools/voxel_register_bench.py [--pairs 1,64,1024] [--sizes 2048,8192,32768] [--scans 10,30] [--maps 1,8] [--modes 1,7]
                                      [--reps 3] [--out profiles/voxel_register_bench_mi355x.jsonl]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,64,1024")
    ap.add_argument("--sizes", default="2048,8192,32768")
    ap.add_argument("--scans", default="10,30", help="posed scans per local map")
    ap.add_argument("--maps", default="1,8", help="local maps per call")
    ap.add_argument("--modes", default="1,7")
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=4, help="distinct draws of the map cloud (repeated to as many clouds as needed)")
    ap.add_argument("--max-corr-dist", type=float, default=2.0, help="of the sgtd_register_clouds calls")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_register_bench_mi355x.jsonl"), help="the file the lines are appended to ('' = none)")
    a = ap.parse_args()
    import torch
    import _register_ref as ref
    from sgtd_amd import manager
    from sgtd_amd._lib import SgtdError

    g = manager.STDescManager()
    stat = lambda v: {"min": round(min(v), 3), "median": round(float(np.median(v)), 3), "n": len(v)}      # noqa: E731
    ints = lambda s: [int(x) for x in s.split(",") if x]                                                 # noqa: E731

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    def copy_ms(pts):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        out = []
        for i in range(1 + a.reps):
            ev[0].record()
            dup = pts.clone()
            ev[1].record()
            torch.cuda.synchronize()
            if i:
                out.append(ev[0].elapsed_time(ev[1]))
            del dup
        return stat(out)

    def summary(res):
        it = res["iterations"]
        return dict(iterations={"min": int(it.min()), "max": int(it.max()), "sum": int(it.sum())},
                    status_counts=np.bincount(res["status"], minlength=5).tolist(), n_matched_mean=round(float(res["n_matched"].mean()), 1),
                    fitness_mean=float(np.nanmean(res["fitness"])))

    def timed_voxels(call):
        g.set_timing(True)
        call()
        ms = g.voxel_register_stage_ms()
        g.set_timing(False)
        return {"covariances": round(ms[0], 3), "map_build": round(ms[1], 3), "correspondences": round(ms[2], 3), "sums_control": round(ms[3], 3),
                "total": round(ms[4], 3)}

    for size in ints(a.sizes):
        draws = []
        for d in range(a.distinct):
            s, t, Rm, tm = ref.planted_scene(size, 100 + d)
            draws.append((s, t[:size]))
        near = ref.near_start(Rm, tm)
        # ---- single-scan maps, beside sgtd_register_clouds on the same pairs
        for pairs in ints(a.pairs):
            shared = (pairs + 1) * size > MAX_TOTAL_POINTS
            n_map_clouds = a.distinct if shared else pairs
            clouds = [draws[0][0]] + [draws[k % a.distinct][1] for k in range(n_map_clouds)]
            off = np.arange(n_map_clouds + 2, dtype=np.int64) * size
            src = np.zeros(pairs, np.int32)
            tgt_cloud = 1 + np.arange(pairs, dtype=np.int32) % n_map_clouds
            map_off, tgt_map = np.arange(pairs + 1, dtype=np.int32), np.arange(pairs, dtype=np.int32)
            init = np.repeat(near[None], pairs, 0)
            pts = torch.from_numpy(np.concatenate(clouds)).cuda()
            floor = copy_ms(pts)
            dense_opt = dict(k_neighbors=20, max_corr_dist=a.max_corr_dist)
            for mode in ints(a.modes):
                vopt = dict(k_neighbors=20, neighbor_mode=mode, voxel_resolution=a.resolution)
                rec = {"run": "voxel_register", "target": "single", "pairs": pairs, "points_per_cloud": size, "clouds": n_map_clouds + 1,
                       "map_clouds_shared": shared, "options": vopt, "ms_device_copy_of_inputs": floor}
                vox = lambda: g.register_voxels(pts, off, map_off, tgt_cloud, None, src, tgt_map, init, **vopt)      # noqa: E731
                dense = lambda: g.register_clouds(pts, off, src, tgt_cloud, init, **dense_opt)                      # noqa: E731
                wall, res = {"voxels": [], "clouds": []}, {}
                for name, call in (("voxels", vox), ("clouds", dense)):
                    try:
                        call()                                      # warm-up, and whether the call takes the configuration
                    except SgtdError as err:
                        rec[name + "_error"] = str(err)
                for i in range(a.reps):                             # the two calls alternate
                    for name, call in (("voxels", vox), ("clouds", dense)):
                        if name + "_error" in rec:
                            continue
                        t0 = time.perf_counter()
                        res[name] = call()
                        wall[name].append((time.perf_counter() - t0) * 1e3)
                if "voxels" in res:
                    rec.update(ms_wall=stat(wall["voxels"]), ms_timed=timed_voxels(vox), **summary(res["voxels"]))
                    rec["n_corr_mean"] = round(float(res["voxels"]["n_corr"].mean()), 1)
                if "clouds" in res:
                    g.set_timing(True)
                    dense()
                    ms = g.register_stage_ms()
                    g.set_timing(False)
                    rec["register_clouds"] = dict(ms_wall=stat(wall["clouds"]), options=dense_opt,
                                                  ms_timed={"covariances": round(ms[0], 3), "searches": round(ms[1], 3),
                                                            "matches_sums_control": round(ms[2], 3), "total": round(ms[3], 3)}, **summary(res["clouds"]))
                    if "voxels" in res:
                        rec["corr_over_search"] = round(rec["ms_timed"]["correspondences"] / ms[1], 4)
                        rec["wall_over_register_clouds"] = round(rec["ms_wall"]["median"] / rec["register_clouds"]["ms_wall"]["median"], 4)
                emit(rec)
            del pts
        # ---- local maps of posed scans
        rng = np.random.default_rng(size)
        for scans in ints(a.scans):
            for maps in ints(a.maps):
                members = maps * scans
                rec = {"run": "voxel_register", "target": "local", "pairs": maps, "maps": maps, "scans_per_map": scans, "points_per_cloud": size,
                       "clouds": members + 1}
                if (members + 1) * size > MAX_TOTAL_POINTS:
                    rec["voxels_error"] = "beyond the caps: %d points in all" % ((members + 1) * size)
                    emit(rec)
                    continue
                clouds = [draws[0][0]] + [draws[k % a.distinct][1] for k in range(members)]
                off = np.arange(members + 2, dtype=np.int64) * size
                map_off = np.arange(maps + 1, dtype=np.int32) * scans
                map_cloud = 1 + np.arange(members, dtype=np.int32)
                pose = np.zeros((members, 12))
                for k in range(members):
                    pose[k, :9] = ref.rot_axis(rng.normal(0, 1, 3), np.deg2rad(0.2) * rng.uniform(-1, 1)).reshape(9)
                    pose[k, 9:] = rng.normal(0, 0.03, 3)
                src, tgt_map = np.zeros(maps, np.int32), np.arange(maps, dtype=np.int32)
                init = np.repeat(near[None], maps, 0)
                pts = torch.from_numpy(np.concatenate(clouds)).cuda()
                rec["ms_device_copy_of_inputs"] = copy_ms(pts)
                for mode in ints(a.modes):
                    vopt = dict(k_neighbors=20, neighbor_mode=mode, voxel_resolution=a.resolution)
                    r = dict(rec, options=vopt)
                    vox = lambda: g.register_voxels(pts, off, map_off, map_cloud, pose, src, tgt_map, init, **vopt)      # noqa: E731
                    try:
                        wall, res = [], None
                        for i in range(1 + a.reps):
                            t0 = time.perf_counter()
                            res = vox()
                            if i:
                                wall.append((time.perf_counter() - t0) * 1e3)
                        r.update(ms_wall=stat(wall), ms_timed=timed_voxels(vox), voxels_per_map=int(len(g.voxel_map(0)["n_points"])), **summary(res))
                        r["n_corr_mean"] = round(float(res["n_corr"].mean()), 1)
                    except SgtdError as err:
                        r["voxels_error"] = str(err)
                    emit(r)
                del pts
    g.close()


if __name__ == "__main__":
    main()
