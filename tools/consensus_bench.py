#!/usr/bin/env python3
"""sgtd_pose_consensus on bench.py's north-star workload (synth.make_map, 10 000 frames x 200 keypoints with poses, one
2048-query batch).  Prints one JSON line per run:

  timing        device time (events on the handle's stream around the call; warm-up first, then --reps timed regions, min
                and median) of sgtd_verify and of sgtd_pose_consensus on the same batch in the same run, and their ratio.
                The ratio is measured, not asserted.  Also how the batch looks to the pass: valid candidates and set sizes.
  localisation  synth.make_queries at its default noise on a smaller map, through evaluate.evaluate_consensus: the
                translation / rotation error (evaluate.compute_adj_rpe against the ground truth) of SearchLoop's choice
                with its own pose and of the fused pose, and accepted / wrong counts (wrong: beyond 5 m or 10 degrees) at
                a few min_support values; with --refine N both sides use sgtd_refine_poses' poses.

usage: tools/consensus_bench.py [--map 10000:200] [--queries 2048] [--reps 7] [--localise 400:256] [--max-trans 2.0]
                                [--max-rot-deg 10] [--refine 0] [--out profiles/consensus_bench_mi355x.jsonl]"""
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
    ap.add_argument("--localise", default="400:256", help="frames:queries of the localisation run ('' = skip)")
    ap.add_argument("--max-trans", type=float, default=2.0)
    ap.add_argument("--max-rot-deg", type=float, default=10.0)
    ap.add_argument("--min-support", default="1,2,3,5")
    ap.add_argument("--refine", type=int, default=0)
    ap.add_argument("--stream", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "consensus_bench_mi355x.jsonl"),
                    help="the file the lines are appended to ('' = none)")
    a = ap.parse_args()
    import torch
    from sgtd_amd import evaluate as ev, manager, synth

    out = open(a.out, "a") if a.out else None
    max_rot = np.deg2rad(a.max_rot_deg)

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
    g.add_frames(m.xyz, m.label)
    g.finalize()
    g.set_frame_poses(np.arange(frames), np.stack([ev.pose_row(*p) for p in m.pose]))
    g.query_frames(qs.xyz, qs.label)
    g.sync()
    t_verify = device_ms(g.verify, a.reps)
    g.pose_consensus(a.max_trans, max_rot)          # (the pose store's upload happens once, here)
    t_cons = device_ms(lambda: g.pose_consensus(a.max_trans, max_rot, fetch=False), a.reps)
    r = g.result_consensus()
    emit({"run": "timing", "frames": frames, "kp": kp, "queries": a.queries, "candidate_num": g.config_setting_["candidate_num"],
          "max_trans": a.max_trans, "max_rot_deg": a.max_rot_deg,
          "valid_candidates": int(r["n_valid"].sum()), "queries_with_a_set": int((r["n_set"] > 0).sum()),
          "mean_set_size": round(float(r["n_set"][r["n_set"] > 0].mean()) if (r["n_set"] > 0).any() else 0.0, 3),
          "max_set_size": int(r["n_set"].max()) if r["n_set"].size else 0,
          "ms_verify": t_verify, "ms_consensus": t_cons,
          "consensus_over_verify": round(t_cons["median"] / t_verify["median"], 5),
          "setup_s": round(time.time() - t0, 1), "device": torch.cuda.get_device_name(0)})
    g.close()

    if a.localise:
        frames, nq = (int(x) for x in a.localise.split(":"))
        m = synth.make_map(frames, 200, stream=421)
        qs = synth.make_queries(m, nq, stream=422)
        g = manager.STDescManager()
        g.add_frames(m.xyz, m.label)
        g.finalize()
        g.set_frame_poses(np.arange(frames), np.stack([ev.pose_row(*p) for p in m.pose]))
        map4 = np.stack([ev.pose_matrix(*p) for p in m.pose])
        gt4 = np.stack([ev.pose_matrix(*p) for p in qs.pose])

        def figures(side):
            t, r_ = side["t_errors"], side["r_errors"]
            return {"accepted": side["accepted"], "wrong": int(side["wrong"]),
                    "median_t_error_m": round(float(np.median(t)), 6) if t else None,
                    "mean_t_error_m": round(float(np.mean(t)), 6) if t else None,
                    "median_r_error_deg": round(float(np.median(r_)), 6) if r_ else None,
                    "mean_r_error_deg": round(float(np.mean(r_)), 6) if r_ else None}

        rec = {"run": "localisation", "frames": frames, "queries": nq, "max_trans": a.max_trans, "max_rot_deg": a.max_rot_deg,
               "refine": a.refine, "consensus": {}}
        for ms in (int(x) for x in a.min_support.split(",")):
            res = ev.evaluate_consensus(g, map4, qs.xyz, qs.label, gt4, a.max_trans, max_rot, min_support=ms, refine=a.refine)
            rec["search_loop"] = figures(res["search_loop"])
            rec["consensus"]["min_support_%d" % ms] = figures(res["consensus"])
            rec["mean_support"] = round(float(np.mean(res["consensus"]["support"])), 3)
        emit(rec)
        g.close()


if __name__ == "__main__":
    main()
