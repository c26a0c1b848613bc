#!/usr/bin/env python3
"""sgtd_align_keypoints on bench.py's north-star workload (synth.make_map, 10 000 frames x 200 keypoints, one 2048-query
batch).  Prints one JSON line:

  timing   device time (events on the handle's stream around the call; warm-up first, then --reps timed regions, min and
           median) of sgtd_verify, of sgtd_overlap and of sgtd_align_keypoints (radius 1.0, 10 iterations, from
           sgtd_verify's pose and from the refined pose, the batch's own keypoints) on the same batch in the same run,
           with the walks made (one per fit and one more), the fits, the stop reasons and the keypoint rms before and
           after over the verified candidates.

usage: tools/align_bench.py [--map 10000:200] [--queries 2048] [--reps 7] [--radius 1.0] [--iterations 10] [--out FILE.jsonl]"""
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
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--stream", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sgtd_amd import manager, synth

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
    g.query_frames(qs.xyz, qs.label)
    g.sync()
    t_verify = device_ms(g.verify, a.reps)
    g.overlap(a.radius)                      # (the first call also builds the store's device copy)
    t_overlap = device_ms(lambda: g.overlap(a.radius), a.reps)
    g.refine_poses(1)
    t_align_ref = device_ms(lambda: g.align_keypoints(a.radius, iterations=a.iterations, refined=True), a.reps)
    t_align = device_ms(lambda: g.align_keypoints(a.radius, iterations=a.iterations), a.reps)
    fits, stops, rb, ra = [], np.zeros(3, np.int64), [], []
    for q in range(a.queries):
        r = g.result_aligned(q)
        ok = r["stop"] >= 0
        fits += r["n_fits"][ok].tolist()
        stops += np.bincount(r["stop"][ok], minlength=3)
        both = ok & ~np.isnan(r["rms_before"]) & ~np.isnan(r["rms_after"])
        rb += r["rms_before"][both].tolist()
        ra += r["rms_after"][both].tolist()
    fits = np.asarray(fits)
    rec = {"run": "timing", "frames": frames, "kp": kp, "queries": a.queries, "candidate_num": g.config_setting_["candidate_num"],
           "radius": a.radius, "iterations": a.iterations, "verified_candidates": int(fits.size), "fits": int(fits.sum()),
           "walks": int(fits.sum() + fits.size), "fits_max": int(fits.max()) if fits.size else 0,
           "stop_iterations_few_converged": stops.tolist(),
           "rms_before_median": round(float(np.median(rb)), 4) if rb else None, "rms_after_median": round(float(np.median(ra)), 4) if ra else None,
           "ms_verify": t_verify, "ms_overlap": t_overlap, "ms_align": t_align, "ms_align_refined_pose": t_align_ref,
           "align_over_overlap": round(t_align["median"] / t_overlap["median"], 3),
           "align_over_verify": round(t_align["median"] / t_verify["median"], 3),
           "setup_s": round(time.time() - t0, 1), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    g.close()


if __name__ == "__main__":
    main()
