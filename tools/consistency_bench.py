#!/usr/bin/env python3
"""sgtd_consistent_loops on synthetic loop closures: a random-walk trajectory, true loops with noise (2 cm, 0.2 deg) and
a share of wrong ones, a fifth of them aliases of one wrong place (tests/_consistency_ref.planted_world).  For every n
prints one JSON line: the call's wall time (sgtd_consistent_loops alone: upload, prepare, pair pass, greedy rounds, one
wait per group of rounds), the device time of the pair pass and of the greedy passes (sgtd_set_timing: events on the
handle's stream), the greedy rounds and |C|; warm-up first, then --reps timed calls, min and median.

usage: tools/consistency_bench.py [--n 1024,8192,32768] [--reps 5] [--outliers 0.2] [--max-trans 1.0] [--max-rot-deg 5] [--out FILE.jsonl]"""
import argparse
import ctypes as C
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
    ap.add_argument("--n", default="1024,8192,32768")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--outliers", type=float, default=0.2)
    ap.add_argument("--max-trans", type=float, default=1.0)
    ap.add_argument("--max-rot-deg", type=float, default=5.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import _consistency_ref as cr
    from sgtd_amd import manager

    for n in (int(x) for x in a.n.split(",")):
        t0 = time.time()
        n_out = int(n * a.outliers)
        w = cr.planted_world(n - n_out, n_out, n_out // 5, seed=a.seed, n_frames=2 * n)
        g = manager.STDescManager(max_frame_n=max(20000, 2 * n + 1))
        g.set_frame_poses(w["ids"], w["poses"])
        g.set_timing(True)
        fa = np.ascontiguousarray(w["frame_a"], np.uint32)
        fb = np.ascontiguousarray(w["frame_b"], np.uint32)
        rel = np.ascontiguousarray(w["rel_pose"], np.float64)
        n_set = C.c_int32(0)
        P = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
        wall, pairs, greedy = [], [], []
        for i in range(1 + a.reps):
            t = time.perf_counter()
            st = g._L.sgtd_consistent_loops(g._h, n, P(fa), P(fb), P(rel), None, a.max_trans, np.deg2rad(a.max_rot_deg), C.byref(n_set))
            dt = (time.perf_counter() - t) * 1e3
            g._check(st)
            s = g.stats()
            if i:
                wall.append(dt)
                pairs.append(s["ms_consistency_pairs"])
                greedy.append(s["ms_consistency_greedy"])
        got = g.consistent_loops(fa, fb, rel, a.max_trans, np.deg2rad(a.max_rot_deg))
        stat = lambda v: {"min": round(min(v), 4), "median": round(float(np.median(v)), 4), "n": len(v)}      # noqa: E731
        in_set = got["in_set"].astype(bool)
        rec = {"run": "consistency", "n": n, "true": int(w["is_true"].sum()), "aliases": int(w["is_alias"].sum()),
               "max_trans": a.max_trans, "max_rot_deg": a.max_rot_deg, "n_set": int(got["n_set"]),
               "true_in_set": int((in_set & w["is_true"]).sum()), "wrong_in_set": int((in_set & ~w["is_true"]).sum()),
               "rounds": int(g.stats()["consistency_rounds"]), "pairs": n * (n - 1) // 2,
               "ms_wall": stat(wall), "ms_pair_pass": stat(pairs), "ms_greedy": stat(greedy),
               "matrix_bytes": 8 * n * ((n + 63) // 64), "setup_s": round(time.time() - t0, 1), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        g.close()


if __name__ == "__main__":
    main()
