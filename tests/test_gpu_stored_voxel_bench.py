"""tools/stored_voxel_register_bench.py at its smallest sizes: it runs, its bit-for-bit assertion between
sgtd_register_voxels and sgtd_register_stored_voxels holds, and its lines carry the keys the README's figures are read from."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = {"covariances", "map_build", "correspondences", "sums_control", "total"}


def test_the_benchmark_runs_and_agrees_bit_for_bit(tmp_path):
    out = str(tmp_path / "bench.jsonl")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stored_voxel_register_bench.py"), "--sizes", "256", "--scans", "2,3", "--maps", "1,2",
                          "--modes", "1,7", "--reps", "1", "--out", out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = [json.loads(line) for line in open(out)]
    assert [json.loads(line) for line in run.stdout.splitlines() if line.startswith("{")] == lines
    # the last line: the loops form beside register_loops_local on a small verified batch
    loops = lines.pop()
    assert loops["target"] == "loops" and loops["rows_and_members_agree"] is True and loops["rows"] >= 3 and loops["members"] > loops["maps"] >= 1
    assert set(loops["ms_wall"]) == {"register_loops_local", "register_loops_local_stored"} and all(v["min"] > 0 for v in loops["ms_wall"].values())
    assert [(r["scans_per_map"], r["maps"], r["options"]["neighbor_mode"]) for r in lines] == [(s, m, o) for s in (2, 3) for m in (1, 2) for o in (1, 7)]
    for r in lines:
        assert r["run"] == "stored_voxel_register" and r["bit_for_bit"] is True and r["points_per_cloud"] == 256
        assert r["stored_frames"] == r["maps"] * r["scans_per_map"] and r["pairs"] == r["maps"] and r["voxels"] > 0
        assert set(r["ms_wall"]) == set(r["ms_timed"]) == {"voxels", "stored"} and r["ms_wall_set_frame_clouds"] > 0
        for call in ("voxels", "stored"):
            assert set(r["ms_wall"][call]) == {"min", "median", "n"} and r["ms_wall"][call]["n"] == 1 and r["ms_wall"][call]["min"] > 0
            assert set(r["ms_timed"][call]) == STAGES and all(v > 0 for v in r["ms_timed"][call].values())
        assert r["wall_stored_over_voxels"] > 0 and sum(r["status_counts"]) == r["pairs"] and r["iterations"]["max"] >= 1
