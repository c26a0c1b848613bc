#!/usr/bin/env python3
"""Sequence loop detection (sgtd_loop_frames) on one synthetic session: a closed Lissajous trajectory of synth.make_map
(it revisits places), 10 000 frames x 200 keypoints, skip_near 0 and 100.  Prints one JSON line per run:

  loop        loop_frames over the whole session in chunks of sgtd_max_batch frames: device events around every chunk,
              one synchronise at the end; frames/s over the wall time
  plain       the same frames as plain query_frames batches (same chunks) against the finished table — every query
              sweeps the whole table (its own frame excluded) instead of the frames below its bound
  sequential  the one-frame path on the first SEQ frames: BuildSingleScanSTD + search_frame + AddSTDescs per frame
              (skip_near > 0: the frame skip_near back is added instead), and whether its candidates, votes and list
              offsets equal the loop batch's for those frames

usage: tools/loop_bench.py [--frames 10000] [--kp 200] [--seq 1000] [--skips 0,100]"""
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
    ap.add_argument("--seq", type=int, default=1000)
    ap.add_argument("--skips", default="0,100")
    ap.add_argument("--stream", type=int, default=41)
    a = ap.parse_args()
    import torch
    from sgtd_amd import manager, synth

    t0 = time.time()
    m = synth.make_map(a.frames, a.kp, stream=a.stream)
    xyz, label = m.xyz, m.label
    print(json.dumps({"run": "input", "frames": a.frames, "kp": a.kp, "make_map_s": round(time.time() - t0, 2)}), flush=True)
    cn = manager.DEFAULTS["candidate_num"]
    for skip in [int(s) for s in a.skips.split(",")]:
        # ---- loop: the whole session, chunked at max_batch
        g = manager.STDescManager()
        chunks, evs = [], []
        torch.cuda.synchronize()
        t = time.perf_counter()
        f0 = 0
        while f0 < a.frames:
            b = int(min(a.frames - f0, max(1, g.max_batch(a.kp))))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.loop_frames(xyz[f0:f0 + b], label[f0:f0 + b], skip_near=skip, batch=b, fetch=False)
            e1.record()
            evs.append((e0, e1))
            chunks.append((f0, b))
            f0 += b
        g.sync()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        dev_ms = sum(e0.elapsed_time(e1) for e0, e1 in evs)
        st = g.stats()
        print(json.dumps({"run": "loop", "skip_near": skip, "frames": a.frames, "chunks": len(chunks),
                          "chunk_frames": [c[1] for c in chunks][:4], "wall_s": round(wall, 4),
                          "frames_per_s": round(a.frames / wall, 1), "device_ms_chunks": round(dev_ms, 3),
                          "entries": st["n_entries"]}), flush=True)
        # ---- plain: the same frames as query_frames batches against the finished table
        torch.cuda.synchronize()
        evs = []
        t = time.perf_counter()
        for f0, b in chunks:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.query_frames(xyz[f0:f0 + b], label[f0:f0 + b], fetch=False)
            e1.record()
            evs.append((e0, e1))
        g.sync()
        torch.cuda.synchronize()
        wall_p = time.perf_counter() - t
        dev_p = sum(e0.elapsed_time(e1) for e0, e1 in evs)
        print(json.dumps({"run": "plain", "skip_near": skip, "frames": a.frames, "wall_s": round(wall_p, 4),
                          "frames_per_s": round(a.frames / wall_p, 1), "device_ms_chunks": round(dev_p, 3),
                          "us_per_query_loop": round(1e3 * dev_ms / a.frames, 3), "us_per_query_plain": round(1e3 * dev_p / a.frames, 3),
                          "note": "plain sweeps the whole table (its own frame excluded); loop also adds its frames"}), flush=True)
        g.close()
        # ---- sequential: the one-frame path, and parity with the loop batch's first frames
        n = min(a.seq, a.frames)
        if n == 0:
            continue
        s = manager.STDescManager()
        built, added = [], 0
        seq = []
        torch.cuda.synchronize()
        t = time.perf_counter()
        for i in range(n):
            d = s.BuildSingleScanSTD(xyz[i], label[i])
            d.frame[:] = i                                     # frame id i (with skip_near > 0 the adds lag behind)
            built.append(d)
            if skip > 0:                                       # the table holds the frames j < i - skip
                while added < i - skip:
                    s.AddSTDescs(built[added])
                    added += 1
            fs = s.search_frame(d, capacity=4096) if d.n > 0 else None   # (candidates are valid on SGTD_ERR_CAPACITY too)
            seq.append(fs)
            if skip == 0:
                s.AddSTDescs(d)
                added += 1
        torch.cuda.synchronize()
        wall_s = time.perf_counter() - t
        # the loop batch's results for those frames: frames 0..n-1 on a handle of their own (chunking composes exactly, so
        # they are what the session's first chunk computed for them)
        p = manager.STDescManager()
        r = p.loop_frames(xyz[:n], label[:n], skip_near=skip)
        p.close()
        equal = True
        for q, fs in enumerate(seq):
            nc = int(r.n_cand[q])
            if fs is None:
                equal &= nc == 0
                continue
            equal &= (fs["n_cand"] == nc and np.array_equal(fs["cand_frame"][:nc], r.cand_frame[q, :nc])
                      and np.array_equal(fs["cand_votes"][:nc], r.cand_votes[q, :nc])
                      and np.array_equal(fs["pair_off"][:nc + 1], r.pair_off[q, :nc + 1]))
        print(json.dumps({"run": "sequential", "skip_near": skip, "frames": n, "wall_s": round(wall_s, 4),
                          "ms_per_frame": round(1e3 * wall_s / n, 4), "frames_per_s": round(n / wall_s, 1),
                          "results_equal_loop": bool(equal), "candidate_num": cn}), flush=True)
        s.close()


if __name__ == "__main__":
    main()
