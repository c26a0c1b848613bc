#!/usr/bin/env python3
"""sgtd_scan_keypoints on a synthetic batch of labelled scans (synth.make_scans: 64 scans of about 120 000 points in
Gaussian blobs, points and labels already on the device).  Prints one JSON line:

  ms_scan_batch / ms_per_scan   time of the call between two events on the device's default stream (warm-up first, then
                                --reps timed calls, min and median).  The call waits for its own kernels — for the
                                component rounds' flags and once for the offsets — so this is the call as a caller sees
                                it, host gaps included, not a sum of kernel times.
  ms_build_batch                the same for sgtd_add_frames (descriptor build + append) on the keypoints the call left
                                on the device: the stage it feeds, for scale.
  s_numpy_one_scan              wall time of the numpy restatement of the rule (tests/_scan_ref.py) on the batch's first
                                scan, whose keypoints are also checked against the device's.

Nothing is promised or asserted about the times.

usage: tools/scan_bench.py [--scans 64] [--points 120000] [--blobs 120] [--reps 5] [--out profiles/scan_bench_mi355x.jsonl]"""
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
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--blobs", type=int, default=120)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stream", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_bench_mi355x.jsonl"), help="the file the line is appended to ('' = none)")
    a = ap.parse_args()
    import torch
    import _scan_ref as ref
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

    t0 = time.time()
    pts, lab, off = synth.make_scans(a.scans, a.points, stream=a.stream, n_blobs=a.blobs, sigma=(0.1, 0.4))
    d_pts, d_lab = torch.from_numpy(pts).cuda(), torch.from_numpy(lab.view(np.int32)).cuda()
    setup_s = time.time() - t0
    g = manager.STDescManager(max_frame_n=a.scans * (a.reps + 4) + 1)
    t_scan = device_ms(lambda: g.scan_keypoints(d_pts, d_lab, off, fetch=False), a.reps)
    xyz, label, kp_off, n_points = g.scan_results()

    def build():
        x, l, o, dev = g._scan_view()
        g._check(g._L.sgtd_add_frames(g._h, x, l, o.ctypes.data_as(manager.C.c_void_p), o.size - 1, dev))

    t_build = device_ms(build, a.reps)
    t1 = time.time()
    first = ref.scan_rule(pts[:off[1]], lab[:off[1]])
    s_numpy = time.time() - t1
    k0 = int(kp_off[1])
    same = bool(np.array_equal(first["xyz"].view(np.uint32), xyz[:k0].view(np.uint32)) and np.array_equal(first["n_points"], n_points[:k0]))
    rec = {"run": "scan_keypoints", "scans": a.scans, "points_per_scan": a.points, "blobs_per_scan": a.blobs,
           "keypoints": int(kp_off[-1]), "keypoints_per_scan": round(float(kp_off[-1]) / max(a.scans, 1), 2),
           "points_in_keypoints": int(n_points.sum()), "ms_scan_batch": t_scan,
           "ms_per_scan": round(t_scan["median"] / max(a.scans, 1), 4), "ms_build_batch": t_build,
           "s_numpy_one_scan": round(s_numpy, 3), "first_scan_equals_numpy": same, "setup_s": round(setup_s, 1),
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    g.close()


if __name__ == "__main__":
    main()
