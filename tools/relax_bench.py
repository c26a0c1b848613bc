#!/usr/bin/env python3
"""sgtd_relax_poses on synthetic sessions: a random walk with dead-reckoned odometry and planted loops
(tests/_relax_ref.planted_world).  For every size two timed configurations with max_outer fixed and the tolerances so
tight that every outer iteration runs and every CG solve takes all of its max_inner iterations: from the two wall times
t = a * outer + b * cg the time per CG iteration (b) and the rest of an outer iteration (a) follow.  A third run with
the default options reports what a caller sees.  Prints one JSON line per size; warm-up first, then --reps timed calls.
It measures and does not check.

usage: tools/relax_bench.py [--sizes 1024:1024,5000:5000,20000:32768] [--reps 3] [--outer 6] [--out FILE.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GROUP = 4      # SGTD_RELAX_GROUP


def launches(outer_done, max_outer, max_inner):
    """kernel launches the host sent, DERIVED from its enqueue pattern (not counted): 3 to start, then 6 + 5 * max_inner
    per outer iteration, in groups of SGTD_RELAX_GROUP"""
    sent, need = 0, max(outer_done, 1)
    while sent < need:
        sent += min(GROUP, max_outer - sent)
    return 3 + sent * (6 + 5 * max_inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024:1024,5000:5000,20000:32768", help="nodes:loops, ...")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--outer", type=int, default=6)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import _relax_ref as rr
    from sgtd_amd import manager

    g = manager.STDescManager()
    for size in a.sizes.split(","):
        n, loops = (int(x) for x in size.split(":"))
        t0 = time.time()
        w = rr.planted_world(n, loops, a.seed)
        setup = time.time() - t0

        def timed(**opt):
            wall, res = [], None
            for i in range(1 + a.reps):
                t = time.perf_counter()
                res = g.relax_poses(w["odom"], w["node_i"], w["node_j"], w["meas"], **opt)
                if i:
                    wall.append((time.perf_counter() - t) * 1e3)
            return wall, res

        stat = lambda v: {"min": round(min(v), 3), "median": round(float(np.median(v)), 3), "n": len(v)}      # noqa: E731
        runs = {}
        for inner in (16, 64):
            opt = dict(max_outer=a.outer, max_inner=inner, cg_tol=1e-30, step_tol=1e-30, lambda_max=1e300)
            wall, res = timed(**opt)
            runs[inner] = dict(ms=min(wall), outer=res["outer_iterations"], cg=res["cg_iterations"], wall=stat(wall),
                               accepted=res["steps_accepted"], launches=launches(res["outer_iterations"], a.outer, inner))
        r1, r2 = runs[16], runs[64]
        det = r1["outer"] * r2["cg"] - r2["outer"] * r1["cg"]
        per_cg = (r1["outer"] * r2["ms"] - r2["outer"] * r1["ms"]) / det if det else float("nan")
        per_outer = (r1["ms"] - per_cg * r1["cg"]) / r1["outer"] if r1["outer"] else float("nan")
        wall, res = timed()
        rec = {"run": "relax", "nodes": n, "odometry_edges": n - 1, "loops": loops, "edges": n - 1 + loops,
               "fixed_16": r1, "fixed_64": r2, "us_per_cg_iteration": round(per_cg * 1e3, 2),
               "us_per_outer_iteration_without_cg": round(per_outer * 1e3, 2),
               "default": {"ms_wall": stat(wall), "outer": res["outer_iterations"], "accepted": res["steps_accepted"],
                           "cg": res["cg_iterations"], "status": res["status"], "cost_before": res["cost_before"],
                           "cost_after": res["cost_after"], "launches": launches(res["outer_iterations"], 50, 64),
                           "mean_trans_error_before": round(rr.mean_trans_error(w["odom"], w["truth"]), 4),
                           "mean_trans_error_after": round(rr.mean_trans_error(res["pose"], w["truth"]), 4)},
               "setup_s": round(setup, 1), "launches_are": "derived from the enqueue pattern"}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    g.close()


if __name__ == "__main__":
    main()
