"""examples/localize.cpp with its optional prior_radius argument: every query restricted to the map frames near its
ground-truth position (sgtd_set_frame_poses + sgtd_set_position_prior).  The run completes, succeeds at least as often
as the unrestricted one, and without the argument prints exactly what it printed before."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_example_localize as tel

pytestmark = pytest.mark.gpu

METRICS = r"map frames (\d+), queries (\d+): loops (\d+), success\(5m,10deg\) (\d+) .*candidate<10m (\d+), top-1 hit (\d+)"


def test_localize_with_a_prior_radius(tmp_path):
    from sgtd_amd import evaluate as ev, ingest, synth
    tel._build()
    smap = synth.make_map(300, 150, stream=23)
    q = synth.make_queries(smap, 24, stream=24)
    (tmp_path / "map").mkdir()
    (tmp_path / "query").mkdir()
    for f in range(300):
        ingest.write_graph_json(tmp_path / "map" / ("%06d.json" % f), smap.xyz[f], smap.label[f], ev.pose_row(*smap.pose[f]))
    for i in range(24):
        ingest.write_graph_json(tmp_path / "query" / ("%06d.json" % i), q.xyz[i], q.label[i], ev.pose_row(*q.pose[i]))
    args = [tel.EXE, str(tmp_path / "map"), str(tmp_path / "query"), "7", "0.4"]
    base = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert base.returncode == 0, base.stdout + base.stderr
    lines = base.stdout.splitlines()
    # without the argument: the metric lines, the error line and the time line, as before
    assert len(lines) == 3 and re.match(METRICS, lines[0]) and lines[1].startswith("mean errors") and lines[2].startswith("time:")
    assert "prior" not in base.stdout
    pri = subprocess.run(args + ["50"], capture_output=True, text=True, timeout=300)
    assert pri.returncode == 0, pri.stdout + pri.stderr
    plines = pri.stdout.splitlines()
    mb, mp = re.match(METRICS, lines[0]), re.match(METRICS, plines[0])
    assert mp, pri.stdout
    gb, gp = [int(x) for x in mb.groups()], [int(x) for x in mp.groups()]
    assert gp[:2] == gb[:2] == [300, 24]
    assert gp[3] >= gb[3] > 12
    m = re.match(r"position prior 50\.00 m: ([\d.]+) map frames allowed per query \((\d+) in all\)", plines[1])
    assert m, pri.stdout
    rows = np.stack([ev.pose_row(*p) for p in smap.pose])
    qrows = np.stack([ev.pose_row(*p) for p in q.pose])
    want = ev.frames_near(rows[:, [3, 7]], qrows[:, [3, 7]].astype(np.float64), 50.0).sum()
    assert int(m.group(2)) == want and 0 < want < 300 * 24
    assert plines[2].startswith("mean errors") and plines[3].startswith("time:") and len(plines) == 4
