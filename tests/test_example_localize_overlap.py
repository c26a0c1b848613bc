"""examples/localize.cpp with --overlap RADIUS --min-overlap X: the map's keypoints stored on the handle, sgtd_overlap after
the verification and sgtd_search_loop_overlap's gated choice.  Without the option the output is what it was; with it
one more line counts what the gate accepted and rejected, and the accounting equals the Python harness
(evaluate_batch(..., min_overlap=X, overlap_radius=RADIUS)) on the same files."""
import re
import subprocess

import numpy as np
import pytest

import test_example_localize as tel

pytestmark = pytest.mark.gpu

LINE = (r"keypoint overlap \(radius ([\d.]+) m, min ([\d.]+)\): accepted (\d+), rejected (\d+), moved to another candidate (\d+), "
        r"mean overlap of the accepted ([\d.]+)$")


def test_localize_with_overlap(tmp_path):
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
    assert len(lines) == 3 and "overlap" not in base.stdout
    loops = int(re.search(r"loops (\d+),", lines[0]).group(1))
    map_pose = np.stack([ev.matrix_from_row(ev.pose_row(*p)) for p in smap.pose])
    q_pose = np.stack([ev.matrix_from_row(ev.pose_row(*p)) for p in q.pose])
    for gate in ("0.4", "0.99", "0"):
        out = subprocess.run(args + ["--overlap", "1.0", "--min-overlap", gate], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        ol = out.stdout.splitlines()
        assert len(ol) == 4 and ol[1].startswith("mean errors of the successes:") and ol[3].startswith("time:")
        m = re.match(LINE, ol[2])
        assert m, out.stdout
        accepted, rejected = int(m.group(3)), int(m.group(4))
        assert float(m.group(1)) == 1.0 and float(m.group(2)) == float(gate)
        assert accepted + rejected == loops                   # every loop of the plain choice is accepted (maybe moved) or rejected
        assert int(re.search(r"loops (\d+),", ol[0]).group(1)) == accepted
        if float(gate) == 0:
            assert ol[:2] == lines[:2] and rejected == 0 and int(m.group(5)) == 0
        mgr = STDescManager()
        mgr.add_frames(smap.xyz, smap.label, keep_keypoints=True)
        met = ev.evaluate_batch(mgr, map_pose, q.xyz, q.label, q_pose, min_overlap=float(gate), overlap_radius=1.0)
        mgr.close()
        assert met.detected == accepted
        assert int(re.search(r"success\(5m,10deg\) (\d+)", ol[0]).group(1)) == met.score_num
        if accepted:
            assert float(gate) <= float(m.group(6)) + 5e-5 <= 1.0 + 1e-4
    # the option may stand anywhere on the line; the default gate is 0.4; bad values are usage errors
    a = subprocess.run([tel.EXE, "--overlap", "1.0"] + args[1:], capture_output=True, text=True, timeout=300)
    b = subprocess.run(args + ["--min-overlap", "0.4", "--overlap", "1.0"], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0 and a.stdout.splitlines()[:3] == b.stdout.splitlines()[:3]
    assert subprocess.run(args + ["--overlap", "-1"], capture_output=True, text=True, timeout=60).returncode == 2
    assert subprocess.run(args + ["--overlap"], capture_output=True, text=True, timeout=60).returncode == 2
    assert subprocess.run(args + ["--min-overlap", "0.4"], capture_output=True, text=True, timeout=60).returncode == 2
