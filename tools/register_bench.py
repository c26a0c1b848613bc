#!/usr/bin/env python3
"""sgtd_register_clouds on synthetic surfaces (tests/_register_ref.planted_scene): one query cloud registered against
`pairs` map clouds of the same size, every map cloud a cloud of its own (so every one gets its covariances), from a start
0.13 m / 0.9 degrees off.  For every (pairs, size): the wall time of the whole call with the points on the device, the
device time by stage under sgtd_set_timing (covariances, searches, the rest: matches, sums and control; the events
serialise the call, so their total is above the untimed wall time's device share), the iteration counts, the time of a
device-to-device copy of the inputs as the floor, and, up to --ref-max points, the restatement's time for one pair on the
host.  A configuration beyond the call's caps is recorded as such.  Prints one JSON line per configuration; warm-up first,
then --reps timed calls.  It measures and does not check.

usage: tools/register_bench.py [--pairs 1,64,1024] [--sizes 2048,8192,32768] [--reps 3] [--out profiles/register_bench_mi355x.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,64,1024")
    ap.add_argument("--sizes", default="2048,8192,32768")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=4, help="distinct draws of the map cloud (repeated to `pairs` clouds)")
    ap.add_argument("--ref-max", type=int, default=2048, help="largest size the restatement is timed at")
    ap.add_argument("--max-corr-dist", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_bench_mi355x.jsonl"), help="the file the lines are appended to ('' = none)")
    a = ap.parse_args()
    import torch
    import _register_ref as ref
    from sgtd_amd import manager
    from sgtd_amd._lib import SgtdError

    g = manager.STDescManager()
    opt = dict(k_neighbors=20, max_corr_dist=a.max_corr_dist)
    stat = lambda v: {"min": round(min(v), 3), "median": round(float(np.median(v)), 3), "n": len(v)}      # noqa: E731
    for size in (int(x) for x in a.sizes.split(",")):
        draws = []
        for d in range(a.distinct):
            s, t, Rm, tm = ref.planted_scene(size, 100 + d)
            draws.append((s, t[:size]))
        near = ref.near_start(Rm, tm)
        ref_s = None
        if size <= a.ref_max:
            t0 = time.perf_counter()
            ref.register([draws[0][0], draws[0][1]], [0], [1], near[None], **opt)
            ref_s = round(time.perf_counter() - t0, 2)
        for pairs in (int(x) for x in a.pairs.split(",")):
            clouds = [draws[0][0]] + [draws[k % a.distinct][1] for k in range(pairs)]
            off = np.arange(pairs + 2, dtype=np.int64) * size
            src, tgt = np.zeros(pairs, np.int32), np.arange(1, pairs + 1, dtype=np.int32)
            init = np.repeat(near[None], pairs, 0)
            rec = {"run": "register", "pairs": pairs, "points_per_cloud": size, "clouds": pairs + 1, "options": opt,
                   "restatement_one_pair_s": ref_s}
            try:
                pts = torch.from_numpy(np.concatenate(clouds)).cuda()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                copy_ms = []
                for i in range(1 + a.reps):
                    ev[0].record()
                    dup = pts.clone()
                    ev[1].record()
                    torch.cuda.synchronize()
                    if i:
                        copy_ms.append(ev[0].elapsed_time(ev[1]))
                    del dup
                wall, res = [], None
                for i in range(1 + a.reps):
                    t0 = time.perf_counter()
                    res = g.register_clouds(pts, off, src, tgt, init, **opt)
                    if i:
                        wall.append((time.perf_counter() - t0) * 1e3)
                g.set_timing(True)
                g.register_clouds(pts, off, src, tgt, init, **opt)
                ms = g.register_stage_ms()
                g.set_timing(False)
                it = res["iterations"]
                rec.update(ms_wall=stat(wall), ms_device_copy_of_inputs=stat(copy_ms),
                           ms_timed={"covariances": round(ms[0], 3), "searches": round(ms[1], 3), "matches_sums_control": round(ms[2], 3),
                                     "total": round(ms[3], 3)},
                           iterations={"min": int(it.min()), "max": int(it.max()), "sum": int(it.sum())},
                           status_counts=np.bincount(res["status"], minlength=5).tolist(),
                           n_matched_mean=round(float(res["n_matched"].mean()), 1), fitness_mean=float(np.nanmean(res["fitness"])))
                del pts
            except SgtdError as err:
                rec["error"] = str(err)
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    g.close()


if __name__ == "__main__":
    main()
