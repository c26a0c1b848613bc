#!/usr/bin/env python3
"""Cost of per-query frame filters (sgtd_set_frame_filter) on bench.py's north-star map: synth.make_map, 10 000 frames x
200 keypoints, 2048-query batches.  Prints one JSON line per run:

  select     the select step (sgtd_query_frames + sgtd_sync, wall) and its device split (sgtd_stats ms_probe — the sweep,
             the undecided records and the filter pass — ms_votes, ms_total) in three cases: no filter; every frame allowed
             (the difference is the pass's own cost); per-query priors of R m around each query's true position
             (evaluate.frames_near), with the frames they allow
  verify     sgtd_verify + sgtd_search_loop (wall) behind the unfiltered and the prior batch
  frame      sgtd_search_frame per frame (wall), one query frame at a time, without and with its prior

usage: tools/filter_bench.py [--frames 10000] [--kp 200] [--queries 2048] [--reps 5] [--radius 50] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--kp", type=int, default=200)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--radius", type=float, default=50.0)
    ap.add_argument("--frame_queries", type=int, default=64)
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

    t0 = time.time()
    m = synth.make_map(a.frames, a.kp, stream=a.stream)
    qs = synth.make_queries(m, a.queries, stream=a.stream + 1)
    prior = evaluate.frames_near(m.pose[:, :2], qs.pose[:, :2], a.radius)
    n_allowed = prior.sum(axis=1)
    emit({"run": "input", "frames": a.frames, "kp": a.kp, "queries": a.queries, "radius_m": a.radius,
          "allowed_frames_mean": round(float(n_allowed.mean()), 1), "allowed_frames_median": float(np.median(n_allowed)),
          "make_map_s": round(time.time() - t0, 2), "device": torch.cuda.get_device_name(0)})
    g = manager.STDescManager()
    g.add_frames(m.xyz, m.label)
    g.finalize()
    g.set_timing(True)
    cases = {"none": None, "all_allowed": np.ones((1, a.frames), bool), "prior": prior}
    g.query_frames(qs.xyz, qs.label)          # warm-up: buffers sized, kernels loaded
    for rep in range(a.reps):
        for name, allowed in cases.items():
            g.set_frame_filter(allowed)
            g.query_frames(qs.xyz, qs.label, fetch=False)
            g.sync()                      # (a warm batch of this filter: its rows are uploaded once)
            t = time.perf_counter()
            g.query_frames(qs.xyz, qs.label, fetch=False)
            g.sync()
            wall = (time.perf_counter() - t) * 1e3
            st = g.stats()
            res = g.results()
            rec = {"run": "select", "case": name, "rep": rep, "ms_wall": round(wall, 3),
                   "ms_probe": round(st["ms_probe"], 3), "ms_votes": round(st["ms_votes"], 3), "ms_total": round(st["ms_total"], 3),
                   "last_M": st["last_M"], "queries_with_candidates": int(np.sum(res.n_cand > 0)),
                   "candidates_mean": round(float(res.n_cand.mean()), 2)}
            if name != "all_allowed":
                t = time.perf_counter()
                g.verify()
                g.search_loop()
                rec["ms_verify_search_loop_wall"] = round((time.perf_counter() - t) * 1e3, 3)
            emit(rec)
    g.set_frame_filter(None)
    # one frame per call
    nf = min(a.frame_queries, a.queries)
    descs = [g.BuildSingleScanSTD(qs.xyz[q], qs.label[q]) for q in range(nf)]
    for d in descs[:4]:
        g.search_frame(d)
    for rep in range(2):
        for name in ("none", "prior"):
            ts = []
            for q in range(nf):
                allowed = prior[q:q + 1] if name == "prior" else None
                if allowed is not None:
                    g.set_frame_filter(allowed)
                t = time.perf_counter()
                g.search_frame(descs[q])
                ts.append((time.perf_counter() - t) * 1e3)
                if allowed is not None:
                    g.set_frame_filter(None)
            emit({"run": "frame", "case": name, "rep": rep, "frames": nf, "ms_per_frame_mean": round(float(np.mean(ts)), 3),
                  "ms_per_frame_median": round(float(np.median(ts)), 3)})
    g.close()


if __name__ == "__main__":
    main()
