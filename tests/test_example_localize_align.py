"""examples/localize.cpp with --align RADIUS[,ITER]: the map's keypoints stored on the handle, sgtd_align_keypoints after
the verification and sgtd_search_loop_aligned's choice accounted with its aligned world pose.  Without the option the
output is what it was; with it two more lines follow, and their counts equal the Python harness
(evaluate_batch(..., align=RADIUS, align_iterations=ITER, min_overlap=0.4)) on the same files."""
import re
import subprocess

import numpy as np
import pytest

import test_example_localize as tel

pytestmark = pytest.mark.gpu

LINE = (r"keypoint alignment \(radius ([\d.]+) m, (\d+) iterations?, overlap >= 0.40\): chosen (\d+), another candidate than "
        r"SearchLoop's (\d+), success\(5m,10deg\) (\d+) \(([\d.]+)\)$")
LINE2 = r"mean errors of the successes, aligned: ([\d.]+) m, ([\d.]+) deg; mean keypoint rms of the chosen ([\d.]+) m before, ([\d.]+) m after$"


def test_localize_with_align(tmp_path):
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
    assert len(lines) == 3 and "alignment" not in base.stdout      # (the plain output: the lines of test_example_localize)
    map_pose = np.stack([ev.matrix_from_row(ev.pose_row(*p)) for p in smap.pose])
    q_pose = np.stack([ev.matrix_from_row(ev.pose_row(*p)) for p in q.pose])
    for opt, radius, it in (("1.0", 1.0, 10), ("0.5,3", 0.5, 3), ("1,1", 1.0, 1)):
        out = subprocess.run(args + ["--align", opt], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        ol = out.stdout.splitlines()
        assert len(ol) == 5 and ol[:2] == lines[:2] and ol[4].startswith("time:")      # the plain lines are byte-identical
        m, m2 = re.match(LINE, ol[2]), re.match(LINE2, ol[3])
        assert m and m2, out.stdout
        assert float(m.group(1)) == radius and int(m.group(2)) == it
        chosen, success = int(m.group(3)), int(m.group(5))
        assert 0 <= int(m.group(4)) <= chosen and success <= chosen
        mgr = STDescManager()
        mgr.add_frames(smap.xyz, smap.label, keep_keypoints=True)
        met = ev.evaluate_batch(mgr, map_pose, q.xyz, q.label, q_pose, align=radius, align_iterations=it, min_overlap=0.4)
        mgr.close()
        assert met.detected == chosen and met.score_num == success
        if success:
            assert abs(float(m2.group(1)) - np.mean(met.t_errors)) <= 1e-4
        if chosen and it > 1:
            assert float(m2.group(4)) <= float(m2.group(3)) + 1e-4
    # the option may stand anywhere on the line and beside --refine; bad values are usage errors
    a = subprocess.run([tel.EXE, "--align", "1.0"] + args[1:], capture_output=True, text=True, timeout=300)
    b = subprocess.run(args + ["--align", "1.0,10"], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0 and a.stdout.splitlines()[:4] == b.stdout.splitlines()[:4]
    r = subprocess.run(args + ["--refine", "1", "--align", "0.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and re.match(LINE, r.stdout.splitlines()[5]), r.stdout
    for bad in (["--align", "-1"], ["--align"], ["--align", "1.0,0"], ["--align", "1.0,x"], ["--align", "abc"]):
        assert subprocess.run(args + bad, capture_output=True, text=True, timeout=60).returncode == 2, bad
