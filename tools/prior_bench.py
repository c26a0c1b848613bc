#!/usr/bin/env python3
"""Position priors by two routes on synth.make_map maps (bench.py's north-star map, 10 000 frames x 200 keypoints, and a
100 000-frame map), 2048-query batches, one prior of R m around each query's true (x, y).  Prints one JSON line per run:

  host      evaluate.frames_near (chunked over the queries, so the [queries, frames, 2] temporaries stay bounded) +
            manager.pack_frame_rows + sgtd_set_frame_filter: the host preparation (ms_prep), then the select step
            (sgtd_query_frames + sgtd_sync, wall) of the first batch under the new rows (prepare_filter re-bases and
            uploads them) and of a repeated batch, with sgtd_stats ms_probe (the sweep, the undecided records and the
            filter pass)
  device    sgtd_set_frame_poses once (ms_poses), then sgtd_set_position_prior (ms_prep): the same select-step figures;
            the first batch builds the rows on the device (prior_kernels.hip.h), a repeated one reuses them
            same_candidates: the candidate tables (n_cand, frames, votes, list offsets) of the two routes are identical
            for every query

The row kernel's own device time comes from a rocprofv3 --kernel-trace --stats run of this tool (prior_rows_kernel).

usage: tools/prior_bench.py [--maps 10000:200,100000:200] [--queries 2048] [--reps 3] [--radius 50] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FIELDS = ("n_cand", "cand_frame", "cand_votes", "pair_off")


def frames_near_chunked(evaluate, map_xy, prior_xy, radius, chunk=64):
    out = np.zeros((len(prior_xy), len(map_xy)), bool)
    for q0 in range(0, len(prior_xy), chunk):
        out[q0:q0 + chunk] = evaluate.frames_near(map_xy, prior_xy[q0:q0 + chunk], radius)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", default="10000:200,100000:200", help="frames:keypoints of each map, comma separated")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--radius", type=float, default=50.0)
    ap.add_argument("--stream", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sgtd_amd import evaluate, manager, synth

    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def select(g, qs):
        t = time.perf_counter()
        g.query_frames(qs.xyz, qs.label, fetch=False)
        g.sync()
        wall = (time.perf_counter() - t) * 1e3
        return wall, g.stats(), g.results()

    for spec in a.maps.split(","):
        frames, kp = (int(x) for x in spec.split(":"))
        t0 = time.time()
        m = synth.make_map(frames, kp, stream=a.stream)
        qs = synth.make_queries(m, a.queries, stream=a.stream + 1)
        rows = np.stack([evaluate.pose_row(*p) for p in m.pose])
        map_xy = rows[:, [3, 7]]
        g = manager.STDescManager(max_frame_n=max(20000, frames + 1))
        g.add_frames(m.xyz, m.label)
        g.finalize()
        g.set_timing(True)
        _, st, _ = select(g, qs)                 # warm-up: buffers sized, kernels loaded
        emit({"run": "input", "frames": frames, "kp": kp, "queries": a.queries, "radius_m": a.radius,
              "entries": st["n_entries"], "setup_s": round(time.time() - t0, 2), "device": torch.cuda.get_device_name(0)})
        t = time.perf_counter()
        g.set_frame_poses(np.arange(frames), rows)
        ms_poses = (time.perf_counter() - t) * 1e3
        for rep in range(a.reps):
            # a fresh set of priors every rep (the queries' positions, moved a little), so the first batch makes its rows
            prior_xy = qs.pose[:, :2] + np.random.default_rng(rep).normal(0.0, 1.0, (a.queries, 2))
            recs = {}
            for route in ("host", "device"):
                t = time.perf_counter()
                if route == "host":
                    allowed = frames_near_chunked(evaluate, map_xy, prior_xy, a.radius)
                    g.set_frame_filter(allowed)
                else:
                    g.set_position_prior(prior_xy, a.radius)
                ms_prep = (time.perf_counter() - t) * 1e3
                w1, st1, res = select(g, qs)
                cand = [getattr(res, k).copy() for k in FIELDS]
                w2, st2, res2 = select(g, qs)
                rec = {"run": route, "frames": frames, "rep": rep, "ms_prep": round(ms_prep, 3),
                       "ms_wall_first": round(w1, 3), "ms_probe_first": round(st1["ms_probe"], 3),
                       "ms_wall_repeat": round(w2, 3), "ms_probe_repeat": round(st2["ms_probe"], 3),
                       "ms_total_repeat": round(st2["ms_total"], 3), "last_M": st2["last_M"],
                       "repeat_same_candidates": all(np.array_equal(x, getattr(res2, k)) for x, k in zip(cand, FIELDS))}
                if route == "host":
                    rec["allowed_frames_mean"] = round(float(allowed.sum(axis=1).mean()), 1)
                    g.set_frame_filter(None)
                else:
                    rec["ms_poses"] = round(ms_poses, 3)
                    g.set_position_prior(None)
                recs[route] = (rec, cand)
            same = all(np.array_equal(x, y) for x, y in zip(recs["host"][1], recs["device"][1]))
            for route in ("host", "device"):
                recs[route][0]["same_candidates"] = same
                emit(recs[route][0])
        g.close()


if __name__ == "__main__":
    main()
