#!/usr/bin/env python3
"""sgtd_thin_clouds on a synthetic batch of raw scans (synth.make_scans: 64 scans of 120 000 points, four floats a point,
already on the device) at several leaves.  Prints one JSON line:

  ms_thin_batch[leaf]     time of the call between two events on the device's default stream (warm-up first, then --reps
                          timed calls, min and median).  The call waits for its own kernels — once for the output size,
                          once at its end — so this is the call as a caller sees it, host gaps included.
  ms_copy_batch           the same for a device-to-device copy of the batch's bytes: the floor of anything that reads them.
  s_host_one_scan[leaf]   wall time of ingest.voxel_downsample on the batch's first scan (the best of three).
  store                   at --store-leaf, for the first --store-frames scans: wall time of set_frame_scans (thin on the
                          device, store from the view) against ingest.voxel_downsample per scan + set_frame_clouds from
                          host arrays, each followed by a wait for the device.

Every timed result is compared bit for bit with ingest.voxel_downsample (every scan of every leaf; the stored clouds'
points and covariances of the two store paths) before anything is reported; a difference ends the run without a line.
Nothing is promised or asserted about the times.

usage: tools/thin_bench.py [--scans 64] [--points 120000] [--leaves 0.1,0.25,0.5] [--reps 5] [--out profiles/thin_bench_mi355x.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--blobs", type=int, default=120)
    ap.add_argument("--leaves", default="0.1,0.25,0.5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stream", type=int, default=1)
    ap.add_argument("--store-leaf", type=float, default=0.5)
    ap.add_argument("--store-frames", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thin_bench_mi355x.jsonl"), help="the file the line is appended to ('' = none)")
    a = ap.parse_args()
    import torch
    from sgtd_amd import ingest, manager, synth

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

    def bits(x):
        return np.ascontiguousarray(x, np.float32).view(np.uint32)

    t0 = time.time()
    pts, _, off = synth.make_scans(a.scans, a.points, stream=a.stream, n_blobs=a.blobs, sigma=(0.1, 0.4))
    d_pts = torch.from_numpy(pts).cuda()
    setup_s = time.time() - t0
    g = manager.STDescManager()
    leaves = [float(v) for v in a.leaves.split(",") if v]
    t_thin, s_host, kept, stages = {}, {}, {}, {}
    for leaf in leaves:
        key = "%g" % leaf
        t_thin[key] = device_ms(lambda: g.thin_clouds(d_pts, off, leaf, fetch=False), a.reps)
        g.set_timing(True)
        g.thin_clouds(d_pts, off, leaf, fetch=False)
        stages[key] = [round(v, 4) for v in g.thin_stage_ms()]
        g.set_timing(False)
        out = g.thin_results()
        best = None
        for s in range(a.scans):
            t1 = time.perf_counter()
            want = ingest.voxel_downsample(pts[off[s]:off[s + 1]], leaf)
            if s == 0:
                best = time.perf_counter() - t1
                for _ in range(2):
                    t1 = time.perf_counter()
                    ingest.voxel_downsample(pts[off[0]:off[1]], leaf)
                    best = min(best, time.perf_counter() - t1)
            got = out["points"][out["pt_off"][s]:out["pt_off"][s + 1]]
            if got.shape != want.shape or not np.array_equal(bits(got), bits(want)):
                sys.exit("leaf %g, scan %d: the device's thinned cloud is not ingest.voxel_downsample's" % (leaf, s))
        if out["n_dropped"].any():
            sys.exit("leaf %g: points were dropped" % leaf)
        s_host[key] = round(best, 4)
        kept[key] = int(out["pt_off"][-1])
    copy = torch.empty_like(d_pts)
    t_copy = device_ms(lambda: (copy.copy_(d_pts), torch.cuda.synchronize()), a.reps)

    # the store: thin on the device and store from the view, against thin on the host and store from host arrays
    nf = min(a.store_frames, a.scans)
    frames = list(range(nf))
    sub_off = off[:nf + 1].copy()
    d_sub = d_pts[:int(sub_off[-1])]
    h_dev, h_host = manager.STDescManager(), manager.STDescManager()

    def store_device():
        h_dev.set_frame_clouds(None, None)
        t1 = time.perf_counter()
        h_dev.set_frame_scans(frames, (d_sub, sub_off), a.store_leaf)
        h_dev.sync()
        torch.cuda.synchronize()
        return time.perf_counter() - t1

    def store_host():
        h_host.set_frame_clouds(None, None)
        t1 = time.perf_counter()
        thin = [ingest.voxel_downsample(pts[sub_off[f]:sub_off[f + 1]], a.store_leaf) for f in frames]
        t2 = time.perf_counter()
        h_host.set_frame_clouds(frames, thin)
        h_host.sync()
        torch.cuda.synchronize()
        return time.perf_counter() - t1, t2 - t1

    store_device(), store_host()      # warm-up: allocations
    s_dev = min(store_device() for _ in range(3))
    both = [store_host() for _ in range(3)]
    s_hst, s_hst_thin = min(b[0] for b in both), min(b[1] for b in both)
    stored_points = 0
    for f in frames:
        (xa, ca), (xb, cb) = h_dev.frame_cloud(f), h_host.frame_cloud(f)
        if xa.shape != xb.shape or not np.array_equal(bits(xa), bits(xb)) or ca.tobytes() != cb.tobytes():
            sys.exit("frame %d: the cloud stored from the device view is not the one stored from the host-thinned cloud" % f)
        stored_points += len(xa)
    rec = {"run": "thin_clouds", "scans": a.scans, "points_per_scan": a.points, "blobs_per_scan": a.blobs, "stride_floats": int(pts.shape[1]),
           "batch_bytes": int(pts.nbytes), "kept_points": kept, "ms_thin_batch": t_thin,
           "ms_thin_per_scan": {k: round(v["median"] / max(a.scans, 1), 4) for k, v in t_thin.items()},
           "ms_stage_sort_rest_total": stages, "ms_copy_batch": t_copy, "s_host_one_scan": s_host,
           "store": {"leaf": a.store_leaf, "frames": nf, "stored_points": stored_points, "s_set_frame_scans": round(s_dev, 4),
                     "s_host_thin_plus_set_frame_clouds": round(s_hst, 4), "s_host_thin_alone": round(s_hst_thin, 4)},
           "all_results_equal_host": True, "setup_s": round(setup_s, 1), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    for h in (g, h_dev, h_host):
        h.close()


if __name__ == "__main__":
    main()
