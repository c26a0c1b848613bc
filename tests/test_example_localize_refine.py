"""examples/localize.cpp with --refine N: sgtd_refine_poses after the verification and a second set of error lines for
the refined poses.  Without the option the output is what it was; with it the default lines are unchanged, the extra
lines are there and equal the Python harness (evaluate_batch(..., refine=N)) on the same files."""
import re
import subprocess

import numpy as np
import pytest

import test_example_localize as tel

pytestmark = pytest.mark.gpu


def test_localize_with_refine(tmp_path):
    from sgtd_amd import evaluate as ev, ingest, synth
    from sgtd_amd.manager import STDescManager
    tel._build()
    smap = synth.make_map(60, 150, stream=19)
    q = synth.make_queries(smap, 14, stream=19)
    (tmp_path / "map").mkdir()
    (tmp_path / "query").mkdir()
    for f in range(60):
        ingest.write_graph_json(tmp_path / "map" / ("%06d.json" % f), smap.xyz[f], smap.label[f], ev.pose_row(*smap.pose[f]))
    for i in range(14):
        ingest.write_graph_json(tmp_path / "query" / ("%06d.json" % i), q.xyz[i], q.label[i], ev.pose_row(*q.pose[i]))
    args = [tel.EXE, str(tmp_path / "map"), str(tmp_path / "query"), "5"]
    base = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert base.returncode == 0, base.stdout + base.stderr
    lines = base.stdout.splitlines()
    assert len(lines) == 3 and lines[1].startswith("mean errors of the successes:") and lines[2].startswith("time:")
    assert "refined" not in base.stdout
    for extra in (["--refine", "1"], ["--refine", "3"]):
        out = subprocess.run(args + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        rl = out.stdout.splitlines()
        assert len(rl) == 6 and rl[:2] == lines[:2] and rl[5].startswith("time:")
        m1 = re.match(r"refined poses \((\d) iterations?\): success\(5m,10deg\) (\d+) \(([\d.]+)\)$", rl[2])
        m2 = re.match(r"mean errors of the successes, refined: ([\d.]+) m, ([\d.]+) deg$", rl[3])
        m3 = re.match(r"mean inlier rmse of the chosen candidates: ([\d.]+) m refined, ([\d.]+) m under the verification's pose$", rl[4])
        assert m1 and m2 and m3, out.stdout
        assert int(m1.group(1)) == int(extra[1])
        assert float(m3.group(1)) <= float(m3.group(2))
        mgr = STDescManager()
        mgr.add_frames(smap.xyz, smap.label)
        map_pose = np.stack([ev.matrix_from_row(ev.pose_row(*p)) for p in smap.pose])
        q_pose = np.stack([ev.matrix_from_row(ev.pose_row(*p)) for p in q.pose])
        met = ev.evaluate_batch(mgr, map_pose, q.xyz, q.label, q_pose, refine=int(extra[1]))
        mgr.close()
        assert int(m1.group(2)) == met.score_num
        assert abs(float(m2.group(1)) - np.mean(met.t_errors)) <= 1e-3
        # compute_adj_rpe takes the angle from the trace of an f32 matrix: next to the identity one ulp of the trace
        # (2.4e-7) moves acos((trace - 1) / 2) by sqrt(2.4e-7) rad = 0.028 deg, and the example's and numpy's f32
        # products round differently — the two means agree to that step, not better
        assert abs(float(m2.group(2)) - np.mean(met.r_errors)) <= 0.03
    # the option may stand anywhere on the line; a bad count is a usage error
    out = subprocess.run([tel.EXE, "--refine", "1"] + args[1:], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and len(out.stdout.splitlines()) == 6
    assert subprocess.run(args + ["--refine", "0"], capture_output=True, text=True, timeout=60).returncode == 2
