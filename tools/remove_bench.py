#!/usr/bin/env python3
"""Cost of taking sessions out of a built table (sgtd_remove_frames) on one synthetic map of synth.make_map, 10 000
frames x 200 keypoints.  10 % of the frames go, two ways: one contiguous session, and scattered 64-frame blocks.
Prints one JSON line per run:

  remove       device events around sgtd_remove_frames on the handle's stream (the call is synchronous: wall time too), per
               repetition on a freshly built table; the next query batch's ms_finalize (the probe layout rebuilt over
               the survivors); the extra device memory the call allocates per entry (keep masks, tile counts, bitmaps and
               the one-field scratch) and what the device's free memory says afterwards
  rebuild      the alternative without the call: fetch the survivors' entries frame by frame (sgtd_fetch_entries), add
               them to a new handle one sgtd_add per frame, finalize; whether its candidate tables for a query batch
               equal the compacted handle's

usage: tools/remove_bench.py [--frames 10000] [--kp 200] [--reps 3] [--out FILE.jsonl]"""
import argparse
import ctypes
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--stream", type=int, default=41)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from sgtd_amd import _lib, manager, synth

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
    emit({"run": "input", "frames": a.frames, "kp": a.kp, "queries": a.queries, "make_map_s": round(time.time() - t0, 2),
          "device": torch.cuda.get_device_name(0)})
    F = a.frames
    n_rm = F // 10
    rng = np.random.default_rng(7)
    n_blocks = max(1, round(n_rm / 64))
    blocks = np.sort(rng.choice(F // 64, n_blocks, replace=False))
    ways = {
        "session": np.arange(F // 2, F // 2 + n_rm),
        "blocks64": np.concatenate([np.arange(b * 64, b * 64 + 64) for b in blocks]),
    }
    stream = torch.cuda.current_stream()

    def built():
        g = manager.STDescManager()
        g.set_stream(stream.cuda_stream)
        g.add_frames(m.xyz, m.label)
        g.query_frames(qs.xyz[:8], qs.label[:8])      # finalized, one batch behind it
        g.sync()
        return g

    for way, removed in ways.items():
        times, finals = [], []
        for rep in range(a.reps):
            g = built()
            E = g.stats()["n_entries"]
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w0 = time.perf_counter()
            e0.record(stream)
            n = g.remove_frames(removed)
            e1.record(stream)
            e1.synchronize()
            wall = (time.perf_counter() - w0) * 1e3
            free1 = torch.cuda.mem_get_info()[0]
            times.append(e0.elapsed_time(e1))
            res = g.query_frames(qs.xyz, qs.label)
            finals.append(g.stats()["ms_finalize"])
            kept = E - n
            # what the call allocates beyond the table: the scratch of the widest field (36 B per survivor), a keep mask
            # bit and a tile count per entry, two bitmaps over the frame span
            extra = 36 * kept + E // 8 + 4 * (E // 1024 + 1) + 2 * 4 * (F // 32 + 1)
            emit({"run": "remove", "way": way, "rep": rep, "frames_removed": int(len(removed)), "entries": E,
                  "entries_removed": n, "ms_remove_device": round(times[-1], 3), "ms_remove_wall": round(wall, 3),
                  "ms_finalize_next_query": round(finals[-1], 3), "extra_bytes_per_entry": round(extra / E, 2),
                  "free_mem_change_mb": round((free1 - free0) / 2 ** 20, 1)})
            if rep < a.reps - 1:
                g.close()
        # the alternative: the survivors' entries to the host frame by frame and into a new handle, one sgtd_add per frame
        h = built()
        E = h.stats()["n_entries"]
        fr = np.zeros(E, np.uint32)
        soa = _lib.DescSoa()
        soa.frame = fr.ctypes.data
        idx = np.arange(E, dtype=np.int64)
        t1 = time.perf_counter()
        assert h._L.sgtd_fetch_entries(h._h, idx.ctypes.data, E, ctypes.byref(soa)) == 0
        cut = np.flatnonzero(np.diff(fr.astype(np.int64))) + 1
        starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [E]])
        keep = ~np.isin(fr[starts], removed)
        fresh = manager.STDescManager(first_frame_id=F - int(keep.sum()))
        fresh.set_stream(stream.cuda_stream)
        t_fetch = t_add = 0.0
        for s0, s1 in zip(starts[keep], ends[keep]):
            ta = time.perf_counter()
            d = h.fetch_entries(np.arange(s0, s1))
            tb = time.perf_counter()
            fresh.AddSTDescs(d)
            t_fetch += tb - ta
            t_add += time.perf_counter() - tb
        tc = time.perf_counter()
        fresh.finalize()
        fresh.sync()
        t_fin = time.perf_counter() - tc
        total = time.perf_counter() - t1
        rb = fresh.query_frames(qs.xyz, qs.label)
        same = all(np.array_equal(getattr(res, k), getattr(rb, k)) for k in ("n_cand", "cand_frame", "cand_votes", "pair_off"))
        emit({"run": "rebuild", "way": way, "frames_kept": int(keep.sum()), "s_total": round(total, 2),
              "s_fetch": round(t_fetch, 2), "s_add": round(t_add, 2), "ms_finalize": round(t_fin * 1e3, 1),
              "candidates_equal_removed_handle": bool(same),
              "median_ms_remove_device": round(float(np.median(times)), 3),
              "median_ms_finalize_next_query": round(float(np.median(finals)), 3)})
        for x in (g, h, fresh):
            x.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
