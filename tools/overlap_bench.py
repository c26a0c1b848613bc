#!/usr/bin/env python3
"""sgtd_overlap on bench.py's north-star workload (synth.make_map, 10 000 frames x 200 keypoints, one 2048-query batch).
Prints one JSON line per run:

  timing        device time (events on the handle's stream around the call; warm-up first, then --reps timed regions, min
                and median) of sgtd_verify and of sgtd_overlap (radius 1.0, sgtd_verify's pose, the batch's own
                keypoints) on the same batch in the same run, with the counts of the model:
                  tests   n_query_kp * n_frame_kp per verified candidate whose frame has keypoints (label compare, then
                          for equal labels the f64 distance) and how many of them had equal labels;
                  bytes   per such candidate its query keypoints (16 B each: 12 B of xyz, 4 B of label), its frame's
                          (16 B each), the pose (96 B) and the results (32 B), each byte once.
                overlap_below_verify tells whether the pass is cheaper than the verification it follows.
  distribution  synth.make_queries at its default noise on a map 12 m apart: n_hit_query of the verified candidates by
                the distance of their frame from the query's true position (median, 5th and 95th percentile), and the
                overlap of the gt_frame candidate.

usage: tools/overlap_bench.py [--map 10000:200] [--queries 2048] [--reps 7] [--distribution 300:96] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", default="10000:200", help="frames:keypoints of the timing map")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--radius", type=float, default=1.0)
    ap.add_argument("--distribution", default="300:96", help="frames:queries of the distribution run ('' = skip)")
    ap.add_argument("--stream", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sgtd_amd import manager, synth

    out = open(a.out, "a") if a.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def device_ms(call, reps, warm=2):
        ms = []
        for i in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if i >= warm:
                ms.append(e0.elapsed_time(e1))
        return {"min": round(min(ms), 4), "median": round(float(np.median(ms)), 4), "n": len(ms)}

    frames, kp = (int(x) for x in a.map.split(":"))
    t0 = time.time()
    m = synth.make_map(frames, kp, stream=a.stream)
    qs = synth.make_queries(m, a.queries, stream=a.stream + 1)
    g = manager.STDescManager(max_frame_n=max(20000, frames + 1))
    g.add_frames(m.xyz, m.label, keep_keypoints=True)
    g.finalize()
    res = g.query_frames(qs.xyz, qs.label)
    g.sync()
    cn = g.config_setting_["candidate_num"]
    t_verify = device_ms(g.verify, a.reps)
    g.overlap(a.radius)                      # (the first call also builds the store's device copy)
    t_overlap = device_ms(lambda: g.overlap(a.radius), a.reps)
    g.refine_poses(1)
    t_overlap_ref = device_ms(lambda: g.overlap(a.radius, refined=True), a.reps)
    g.overlap(a.radius)
    verified = tests = same = n_bytes = 0
    labels_f = [np.bincount(m.label[f].astype(np.int64)) for f in range(frames)]
    for q in range(a.queries):
        r = g.result_overlap(q)
        lq = np.bincount(qs.label[q].astype(np.int64))
        for k in np.nonzero(r["n_frame_kp"] >= 0)[0]:
            nqk, nfk = int(r["n_query_kp"][k]), int(r["n_frame_kp"][k])
            lf = labels_f[int(res.cand_frame[q, k])]
            n = min(len(lq), len(lf))
            verified += 1
            tests += nqk * nfk
            same += int((lq[:n] * lf[:n]).sum())
            n_bytes += 16 * (nqk + nfk) + 96 + 32
    emit({"run": "timing", "frames": frames, "kp": kp, "queries": a.queries, "candidate_num": cn, "radius": a.radius,
          "verified_candidates": verified, "label_tests": tests, "distance_tests": same, "model_bytes": n_bytes,
          "ms_verify": t_verify, "ms_overlap": t_overlap, "ms_overlap_refined_pose": t_overlap_ref,
          "label_tests_per_ns": round(tests / (t_overlap["median"] * 1e6), 3),
          "overlap_below_verify": bool(t_overlap["median"] < t_verify["median"] and t_overlap["min"] < t_verify["min"]),
          "setup_s": round(time.time() - t0, 1), "device": torch.cuda.get_device_name(0)})
    g.close()

    if a.distribution:
        frames, nq = (int(x) for x in a.distribution.split(":"))
        m = synth.make_map(frames, 200, stream=411, spacing=12.0)
        qs = synth.make_queries(m, nq, stream=412)
        g = manager.STDescManager()
        g.add_frames(m.xyz, m.label, keep_keypoints=True)
        g.finalize()
        res = g.query_frames(qs.xyz, qs.label)
        g.verify()
        g.refine_poses(1)
        rec = {"run": "distribution", "frames": frames, "spacing_m": 12.0, "queries": nq, "radius": a.radius}
        for tag, refined in (("verify_pose", False), ("refined_pose", True)):
            g.overlap(a.radius, refined=refined)
            bins = {"within_12m": [], "12_to_40m": [], "beyond_40m": []}
            gt = []
            for q in range(nq):
                r = g.result_overlap(q)
                for k in np.nonzero(r["n_frame_kp"] >= 0)[0]:
                    f = int(res.cand_frame[q, k])
                    d = float(np.hypot(m.pose[f][0] - qs.pose[q][0], m.pose[f][1] - qs.pose[q][1]))
                    bins["within_12m" if d <= 12 else ("12_to_40m" if d <= 40 else "beyond_40m")].append(int(r["n_hit_query"][k]))
                    if f == int(qs.gt_frame[q]):
                        gt.append(float(r["overlap"][k]))
            rec[tag] = {name: {"n": len(v), "median": float(np.median(v)), "p5": float(np.percentile(v, 5)), "p95": float(np.percentile(v, 95))}
                        for name, v in bins.items() if v}
            rec[tag]["gt_frame_overlap"] = {"n": len(gt), "min": round(min(gt), 4), "median": round(float(np.median(gt)), 4),
                                            "below_0.4": int(sum(o < 0.4 for o in gt))}
        emit(rec)
        g.close()


if __name__ == "__main__":
    main()
