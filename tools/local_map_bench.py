#!/usr/bin/env python3
"""sgtd_local_map_keypoints on synthetic posed scans (synth.make_posed_scans: one world of Gaussian blobs seen from
poses `spacing` metres apart along a path; points and labels already on the device).  Prints one JSON line per spacing:

  ms_call           the whole call between two events on the device's default stream, host waits included (warm-up
                    first, then --reps timed calls, min and median)
  ms_members / ms_gather / ms_scan_passes
                    the call's stages between events on its stream (sgtd_set_timing on: sgtd_local_map_stage_ms), of the
                    median call: both member-selection launches; per pass the segment table and the gather; per pass the
                    scan pipeline with its host waits
  ms_premerged_scan (a) sgtd_scan_keypoints on the same merged clouds, pre-merged on the host by the restatement
                    (tests/_local_map_ref.py) and handed over as device arrays, one call per pass of the same plan: the
                    floor for the clustering.  Its keypoints are compared bit for bit with the call's.
  ms_copy           (b) a plain device-to-device copy that moves as many bytes as the gather reads and writes (a copy of
                    n bytes reads n and writes n, so n = merged points * (4 * stride + 4 + 16) / 2): the floor for
                    the gather
  within_a_plus_3b / gather_within_2b
                    the two expectations of the feature's issue, as booleans: ms_call <= (a) + 3 (b), ms_gather <= 2 (b)
  s_numpy_one_anchor  wall time of the numpy restatement of the first anchor's local map

Nothing is asserted about the times.

usage: tools/local_map_bench.py [--scans 64] [--points 120000] [--spacing 3.0 1.0] [--reps 3] [--out profiles/local_map_bench_mi355x.jsonl]"""
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
    ap.add_argument("--spacing", type=float, nargs="+", default=[3.0, 1.0], help="metres between poses: 3.0 gives about 10 members at radius 15, 1.0 about 30")
    ap.add_argument("--radius", type=float, default=15.0)
    ap.add_argument("--blobs_per_100m", type=int, default=300, help="blobs per 100 m of path (about 120 within sensor range of a pose)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stream", type=int, default=1)
    ap.add_argument("--max_pass_points", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_map_bench_mi355x.jsonl"), help="the file the lines are appended to ('' = none)")
    a = ap.parse_args()
    import torch
    import _local_map_ref as ref
    from sgtd_amd import manager, synth

    def device_ms(call, reps, warm=1, after=None):
        ms, extra = [], []
        for i in range(warm + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if i >= warm:
                ms.append(e0.elapsed_time(e1))
                extra.append(after() if after else None)
        return ms, extra

    def summary(ms):
        return {"min": round(min(ms), 4), "median": round(float(np.median(ms)), 4), "n": len(ms)}

    for spacing in a.spacing:
        t0 = time.time()
        length = spacing * a.scans
        blobs = max(60, int(a.blobs_per_100m * (length + 80.0) / 100.0))
        pts, lab, off, poses = synth.make_posed_scans(a.scans, a.points, stream=a.stream, spacing=spacing, n_blobs=blobs, sensor_range=40.0,
                                                      sigma=(0.1, 0.4))
        d_pts, d_lab = torch.from_numpy(pts).cuda(), torch.from_numpy(lab.view(np.int32)).cuda()
        g = manager.STDescManager()
        g.set_timing(True)
        kw = dict(radius=a.radius, max_pass_points=a.max_pass_points)
        ms_call, stages = device_ms(lambda: g.local_map_keypoints(d_pts, d_lab, off, poses, fetch=False, **kw), a.reps, after=g.local_map_stage_ms)
        mid = int(np.argsort(ms_call)[len(ms_call) // 2])
        xyz, label, kp_off, n_points = g.local_map_results()
        mem_off, member, merged, n_passes = g.local_map_members()

        # (a) the same merged clouds, pre-merged on the host, through sgtd_scan_keypoints pass by pass
        cap = a.max_pass_points or 1 << 26
        passes, a0 = [], 0
        while a0 < a.scans:
            a1, room = a0, cap
            while a1 < a.scans and merged[a1] <= room:
                room -= merged[a1]
                a1 += 1
            passes.append((a0, a1))
            a0 = a1
        assert len(passes) == n_passes
        ms_pre, same = np.zeros(a.reps), True
        for a0, a1 in passes:
            clouds = [ref.merged_cloud(pts, lab, off, poses, member[mem_off[j]:mem_off[j + 1]].tolist()) for j in range(a0, a1)]
            m_off = np.concatenate([[0], np.cumsum([len(c[1]) for c in clouds])]).astype(np.int64)
            m_pts = torch.from_numpy(np.concatenate([c[0] for c in clouds])).cuda()
            m_lab = torch.from_numpy(np.concatenate([c[1] for c in clouds]).view(np.int32)).cuda()
            del clouds
            ms, _ = device_ms(lambda: g.scan_keypoints(m_pts, m_lab, m_off, fetch=False), a.reps)
            ms_pre += np.array(ms)
            sx, sl, so, sn = g.scan_results()
            k0, k1 = int(kp_off[a0]), int(kp_off[a1])
            same = same and bool(np.array_equal(sx.view(np.uint32), xyz[k0:k1].view(np.uint32)) and np.array_equal(sn, n_points[k0:k1]) and
                                 np.array_equal(so, kp_off[a0:a1 + 1] - k0))
            del m_pts, m_lab

        # (b) a copy that moves the gather's bytes
        total = int(merged.sum())
        n_copy = total * (4 * pts.shape[1] + 4 + 16) // 2
        chunk = min(n_copy, 1 << 30)
        src, dst = torch.empty(chunk, dtype=torch.uint8, device="cuda"), torch.empty(chunk, dtype=torch.uint8, device="cuda")

        def copy():
            left = n_copy
            while left > 0:
                n = min(left, chunk)
                dst[:n].copy_(src[:n])
                left -= n

        ms_copy, _ = device_ms(copy, a.reps)
        del src, dst

        t1 = time.time()
        first = ref.local_map_rule(pts, lab, off, poses, anchors=[0], radius=a.radius)
        s_numpy = time.time() - t1
        k0 = int(kp_off[1])
        first_same = bool(np.array_equal(first["xyz"].view(np.uint32), xyz[:k0].view(np.uint32)) and np.array_equal(first["n_points"], n_points[:k0]))
        call, pre, cp = float(np.median(ms_call)), float(np.median(ms_pre)), float(np.median(ms_copy))
        st = stages[mid]
        rec = {"run": "local_map_keypoints", "scans": a.scans, "points_per_scan": a.points, "spacing_m": spacing, "radius_m": a.radius,
               "blobs_in_world": blobs, "members_per_anchor": round(float(len(member)) / a.scans, 2), "merged_points": total,
               "n_passes": n_passes, "keypoints": int(kp_off[-1]), "keypoints_per_anchor": round(float(kp_off[-1]) / a.scans, 2),
               "ms_call": summary(ms_call), "ms_members": round(st[0], 4), "ms_gather": round(st[1], 4), "ms_scan_passes": round(st[2], 4),
               "ms_premerged_scan": summary(ms_pre.tolist()), "ms_copy": summary(ms_copy), "copy_bytes": n_copy,
               "copy_gb_per_s": round(2.0 * n_copy / cp / 1e6, 1), "gather_gb_per_s": round(2.0 * n_copy / max(st[1], 1e-9) / 1e6, 1),
               "within_a_plus_3b": bool(call <= pre + 3.0 * cp), "gather_within_2b": bool(st[1] <= 2.0 * cp),
               "equals_premerged_scan": same, "s_numpy_one_anchor": round(s_numpy, 3), "first_anchor_equals_numpy": first_same,
               "setup_s": round(time.time() - t0, 1), "device": torch.cuda.get_device_name(0)}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        g.close()
        del d_pts, d_lab
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
