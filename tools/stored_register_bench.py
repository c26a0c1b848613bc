#!/usr/bin/env python3
"""sgtd_register_stored beside sgtd_register_clouds, on tools/register_bench.py's protocol and scene: one query cloud
registered against `pairs` map clouds of the same size (synthetic surfaces, tests/_register_ref.planted_scene), from a start
0.13 m / 0.9 degrees off, k 20, points on the device.  For every (pairs, size): the time of sgtd_set_frame_clouds for the
map, once (the points packed and every map cloud's covariances); then, after a warm-up of each, --reps repetitions that
alternate the two calls in the same run: the wall time of the whole call (host waits included) and, in one further call each
under sgtd_set_timing, the device time by stage (covariances, searches, the rest).  The stored call gets the query cloud alone;
sgtd_register_clouds gets the query and every map cloud, as it must.  The two calls' results are compared bit for bit (every
field of every pair, the matches of the first and the last pair, the query's covariances) and the line says whether they
agree.  A configuration beyond a call's caps is recorded as such, for that call.  Prints one JSON line per configuration.

usage: tools/stored_register_bench.py [--pairs 1,64,1024] [--sizes 2048,8192,32768] [--reps 3] [--out profiles/stored_register_bench_mi355x.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELDS = ("pose", "fitness", "cost", "n_matched", "iterations", "status")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,64,1024")
    ap.add_argument("--sizes", default="2048,8192,32768")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=4, help="distinct draws of the map cloud (repeated to `pairs` clouds)")
    ap.add_argument("--max-corr-dist", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stored_register_bench_mi355x.jsonl"), help="the file the lines are appended to ('' = none)")
    a = ap.parse_args()
    import torch
    import _register_ref as ref
    from sgtd_amd import manager
    from sgtd_amd._lib import SgtdError

    g = manager.STDescManager()
    opt = dict(k_neighbors=20, max_corr_dist=a.max_corr_dist)
    stat = lambda v: {"min": round(min(v), 3), "median": round(float(np.median(v)), 3), "n": len(v)}      # noqa: E731
    stages = lambda ms: {"covariances": round(ms[0], 3), "searches": round(ms[1], 3), "matches_sums_control": round(ms[2], 3),      # noqa: E731
                         "total": round(ms[3], 3)}
    for size in (int(x) for x in a.sizes.split(",")):
        draws = []
        for d in range(a.distinct):
            s, t, Rm, tm = ref.planted_scene(size, 100 + d)
            draws.append((s, t[:size]))
        near = ref.near_start(Rm, tm)
        for pairs in (int(x) for x in a.pairs.split(",")):
            maps = [draws[k % a.distinct][1] for k in range(pairs)]
            frames = np.arange(pairs, dtype=np.uint32)
            init = np.repeat(near[None], pairs, 0)
            rec = {"run": "stored_register", "pairs": pairs, "points_per_cloud": size, "options": opt}
            query = torch.from_numpy(draws[0][0]).cuda()
            qoff = np.array([0, size], np.int64)
            map_pts = torch.from_numpy(np.concatenate(maps)).cuda()
            # the map, once
            g.set_frame_clouds(None, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.set_frame_clouds(frames, (map_pts, np.arange(pairs + 1, dtype=np.int64) * size), k_neighbors=20)
            rec["ms_set_frame_clouds"] = round((time.perf_counter() - t0) * 1e3, 3)
            rec["store"] = g.frame_clouds_info()
            src = np.zeros(pairs, np.int32)
            all_pts = torch.cat([query, map_pts])
            off = np.arange(pairs + 2, dtype=np.int64) * size
            tgt = np.arange(1, pairs + 1, dtype=np.int32)
            calls = {
                "stored": (lambda: g.register_stored(query, qoff, src, frames, init, **opt), g.stored_register_stage_ms),
                "clouds": (lambda: g.register_clouds(all_pts, off, src, tgt, init, **opt), g.register_stage_ms),
            }
            wall, res, failed = {k: [] for k in calls}, {}, {}
            for i in range(1 + a.reps):      # (the first: warm-up; then alternating)
                for k, (call, _) in calls.items():
                    if k in failed:
                        continue
                    try:
                        t0 = time.perf_counter()
                        res[k] = call()
                        if i:
                            wall[k].append((time.perf_counter() - t0) * 1e3)
                    except SgtdError as err:
                        failed[k] = str(err)
            g.set_timing(True)
            for k, (call, ms) in calls.items():
                if k in failed:
                    rec[k] = {"error": failed[k]}
                    continue
                call()
                it = res[k]["iterations"]
                rec[k] = {"ms_wall": stat(wall[k]), "ms_timed": stages(ms()),
                          "iterations": {"min": int(it.min()), "max": int(it.max()), "sum": int(it.sum())},
                          "status_counts": np.bincount(res[k]["status"], minlength=5).tolist()}
            g.set_timing(False)
            if not failed:
                same = all(ref.same(res["stored"][f], res["clouds"][f]) for f in FIELDS)
                g.register_stored(query, qoff, src, frames, init, **opt)
                g.register_clouds(all_pts, off, src, tgt, init, **opt)
                for k in sorted({0, pairs - 1}):
                    (j, d2), (rj, rd2) = g.stored_matches(k), g.register_matches(k)
                    same = same and bool(np.array_equal(j, rj)) and ref.same(d2, rd2)
                same = same and ref.same(g.stored_covariances(0), g.register_covariances(0))
                rec["bit_for_bit"] = bool(same)
                rec["stored_over_clouds_wall_median"] = round(rec["stored"]["ms_wall"]["median"] / rec["clouds"]["ms_wall"]["median"], 3)
            del query, map_pts, all_pts
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    g.set_frame_clouds(None, None)
    g.close()


if __name__ == "__main__":
    main()
