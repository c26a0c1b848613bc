#!/usr/bin/env python3
"""sgtd_refine_poses on bench.py's north-star workload (synth.make_map, 10 000 frames x 200 keypoints, one 2048-query
batch).  Prints one JSON line per run:

  timing    device time (events on the handle's stream around the call; warm-up first, then --reps timed regions, min and
            median) of sgtd_verify and of sgtd_refine_poses with 1 and 3 iterations on the same batch in the same run, the
            byte model of the refit and the fraction of the HBM peak it reaches:
              1 B flag + 8 B pair word per listed pair, 72 B of vertices per inlier pair,
              and per further iteration the vertices of every listed pair once more (72 B) plus a flag read and written
            (the model counts each byte once; the kernel reads the vertices of sets beyond its LDS capacity three times,
            mostly from cache — DESIGN.md).  refine_1_below_verify is the one condition on the kernel.
  accuracy  synth.make_queries at its default noise on a smaller map: the median translation / rotation error
            (evaluate.compute_adj_rpe against the ground truth) of SearchLoop's choice with sgtd_verify's world pose and
            with the refined one, and the mean inlier rmse under both.

usage: tools/refine_bench.py [--map 10000:200] [--queries 2048] [--reps 7] [--accuracy 400:256] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBS = 8000.0      # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", default="10000:200", help="frames:keypoints of the timing map")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--accuracy", default="400:256", help="frames:queries of the accuracy run ('' = skip)")
    ap.add_argument("--stream", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sgtd_amd import evaluate as ev, manager, synth

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
    g.add_frames(m.xyz, m.label)
    g.finalize()
    res = g.query_frames(qs.xyz, qs.label)
    g.sync()
    cn = g.config_setting_["candidate_num"]
    t_verify = device_ms(g.verify, a.reps)
    t_r1 = device_ms(lambda: g.refine_poses(1), a.reps)
    listed = inliers = verified = 0
    for q in range(a.queries):
        n = g.result_refined(q)["n_pairs"]
        has = n > 0
        listed += int((res.pair_off[q, 1:cn + 1] - res.pair_off[q, :cn])[has].sum())
        inliers += int(n.sum())
        verified += int(has.sum())
    t_r3 = device_ms(lambda: g.refine_poses(3), a.reps)
    inliers3 = sum(int(g.result_refined(q)["n_pairs"].sum()) for q in range(a.queries))
    bytes_1 = 9 * listed + 72 * inliers
    bytes_3 = bytes_1 + 2 * (74 * listed) + 72 * 2 * inliers3       # (two further re-selections, two further gathers at most)
    emit({"run": "timing", "frames": frames, "kp": kp, "queries": a.queries, "candidate_num": cn, "verified_candidates": verified,
          "listed_pairs": listed, "inlier_pairs": inliers, "inlier_pairs_after_3": inliers3,
          "ms_verify": t_verify, "ms_refine_1": t_r1, "ms_refine_3": t_r3,
          "model_bytes_refine_1": bytes_1, "model_bytes_refine_3_upper": bytes_3,
          "hbm_fraction_refine_1": round(bytes_1 / (t_r1["median"] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
          "hbm_fraction_refine_3": round(bytes_3 / (t_r3["median"] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4),
          "refine_1_below_verify": bool(t_r1["median"] < t_verify["median"] and t_r1["min"] < t_verify["min"]),
          "setup_s": round(time.time() - t0, 1), "device": torch.cuda.get_device_name(0)})
    g.close()

    if a.accuracy:
        frames, nq = (int(x) for x in a.accuracy.split(":"))
        m = synth.make_map(frames, 200, stream=421)
        qs = synth.make_queries(m, nq, stream=422)
        rows = np.stack([ev.pose_row(*p) for p in m.pose])
        g = manager.STDescManager()
        g.add_frames(m.xyz, m.label)
        g.finalize()
        g.set_frame_poses(np.arange(frames), rows)
        g.query_frames(qs.xyz, qs.label)
        g.verify()
        bc, bf, _ = g.search_loop()
        rec = {"run": "accuracy", "frames": frames, "queries": nq, "loops": int((bf >= 0).sum())}
        for it in (1, 3):
            g.refine_poses(it)
            err = {"verify": [], "refined": []}
            rm = {"verify": [], "refined": []}
            for q in range(nq):
                if bf[q] < 0:
                    continue
                gt, k = ev.pose_matrix(*qs.pose[q]), int(bc[q])
                r = g.result_refined(q)
                rm["verify"].append(r["rmse_verify"][k])
                rm["refined"].append(r["rmse"][k])
                for name, w in (("verify", g.result_world_poses(q)), ("refined", g.result_refined_world_poses(q))):
                    err[name].append(ev.compute_adj_rpe(gt, ev.matrix_from_row(w[k])))
            for name in ("verify", "refined"):
                tag = name if name == "verify" else "refined_%d" % it
                rec["median_t_error_m_" + tag] = round(float(np.median([e[0] for e in err[name]])), 6)
                rec["median_r_error_deg_" + tag] = round(float(np.median([e[1] for e in err[name]])), 6)
                rec["mean_inlier_rmse_m_" + ("verify_on_set_%d" % it if name == "verify" else tag)] = round(float(np.mean(rm[name])), 6)
        emit(rec)
        g.close()


if __name__ == "__main__":
    main()
