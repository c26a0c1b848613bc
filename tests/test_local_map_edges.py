"""The worlds of tests/_local_map_edges.py reach their edges, and every mutant of the restatement changes the world named
for it: shown on the CPU with tests/_local_map_ref.py alone.  The GPU side is tests/test_gpu_local_map_edges.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _local_map_edges as le  # noqa: E402
import _local_map_ref as ref  # noqa: E402
import _scan_ref as sref  # noqa: E402


def lists(want):
    o = want["mem_off"]
    return [want["member"][o[a]:o[a + 1]].tolist() for a in range(len(o) - 1)]


def owned(mem, n_scans):
    """the members other than the anchor as flags, one row per thread of lm_members_kernel (16 consecutive scans)"""
    flags = np.zeros((n_scans + le.PER - 1) // le.PER * le.PER, bool)
    flags[mem[1:]] = True
    return flags.reshape(-1, le.PER)


def test_every_point_is_in_instance_mode():
    for name in ("lattice-600", "full-lds", "anchors-4097"):
        w = le.world(name)
        assert np.all((w["l"] & 0xFFFF) == 10) and np.all((w["l"] >> 16) >= 1) and w["cfg"]["min_instance_points"] == 0
        assert sref.clear_of_boundaries(w["p"], w["l"], w["cfg"])


def test_lattice_600():
    w, want = le.world("lattice-600"), le.expected("lattice-600")
    t = w["poses"][:, [3, 7, 11]]
    assert len(t) == 600 and np.array_equal(np.diff(w["off"]), 1 + np.arange(600) % 3)
    assert sorted(map(tuple, t.tolist())) == [(float(x), float(y), 0.0) for x in range(25) for y in range(24)]
    assert w["poses"][:, [0, 5, 10]].min() == 1.0 and np.abs(w["poses"][:, [1, 2, 4, 6, 8, 9]]).max() == 0.0
    assert w["kw"]["anchors"] == [0, 15, 16, 17, 255, 256, 257, 599] and w["kw"]["radius"] == 12.0
    mems = lists(want)
    counts = [len(m) for m in mems]
    assert all(200 <= c <= 400 for c in counts) and len(set(counts)) == len(counts), counts
    for j, m in zip(w["kw"]["anchors"], mems):
        assert m[0] == j and m[1:] == sorted(m[1:]) and m == ref.members(w["poses"], j, 12.0)
        rows = owned(m, 600)
        assert (~rows[:37].any(axis=1)).any(), "no thread without a member"
        assert (rows[:, 0] & rows[:, le.PER - 1]).any(), "no thread with members at both ends of its range"
        assert max(m) >= 512 and sum(i >= 256 for i in m) > 50      # (the strided loops take a second and a third step)
    sizes = np.diff(w["off"])
    assert want["merged_points"].tolist() == [int(sizes[m].sum()) for m in mems]
    assert all(len(r["label"]) == 7 for r in want["res"])      # seven instance groups, each of many members' points


@pytest.mark.parametrize("cut", le.CUTS)
def test_lattice_600_cut(cut):
    w, want = le.world("lattice-600-cut-%d" % cut), le.expected("lattice-600-cut-%d" % cut)
    poses, anchors = w["poses"], w["kw"]["anchors"]
    mems = lists(want)
    uncut = [len(m) for m in lists(le.expected("lattice-600"))]
    assert [len(m) for m in mems] == [min(cut, n) for n in uncut] and all(m[0] == j and m[1:] == sorted(m[1:]) for j, m in zip(anchors, mems))
    assert sum(n > cut for n in uncut) >= 4      # (at 257 and 258 some anchors have fewer candidates: their lists are not cut)
    assert all(m == le.members(poses, j, 12.0, cut) for j, m in zip(anchors, mems))
    if cut in (17, 257):
        # ties at the cut: equal d2 on both sides of it, the smaller index kept
        tied = [c for c in (le.cut(poses, j, 12.0, cut) for j in anchors) if c is not None and c[0][0] == c[1][0]]
        assert tied and all(c[0][1] < c[1][1] for c in tied)
        assert any(le.members(poses, j, 12.0, cut, "tie_high") != m for j, m in zip(anchors, mems))
    if cut > 2:
        assert any(le.members(poses, j, 12.0, cut, "rank_order") != m for j, m in zip(anchors, mems))
    assert [len(le.members(poses, j, 12.0, cut, "cut_without_anchor")) for j in anchors] == [min(cut + 1, n) for n in uncut]
    assert any(le.members(poses, j, 12.0, cut, "cut_without_anchor") != m for j, m in zip(anchors, mems))
    if cut == 257:
        assert any(sum(i >= 256 for i in m) > 0 and len(m) > 256 for m in mems)      # more kept members than threads


def test_ties_of_anchor_zero():
    poses = le.world("lattice-600")["poses"]
    (a, _), (b, _) = le.cut(poses, 0, 12.0, 17)
    (c, _), (d, _) = le.cut(poses, 0, 12.0, 257)
    print("anchor 0: d2 at the cut of 17: %g and %g; of 257: %g and %g" % (a, b, c, d))
    assert a == b and c == d


def test_full_lds():
    w, want = le.world("full-lds"), le.expected("full-lds")
    n = np.diff(w["off"])
    assert len(n) == le.MAX_SCANS == 4096 and sorted(np.nonzero(n)[0].tolist()) == sorted(le.FULL_LIVE) and all(50 <= c <= 200 for c in n[n > 0])
    assert {0, 4080, 4095} <= set(le.FULL_LIVE) and w["kw"]["anchors"] == [0, 4080, 4095]
    mems = lists(want)
    for m in mems:
        assert {0, 4080, 4095} <= set(m)
    assert len(mems[0]) > 20 and any(n[i] == 0 for i in mems[0])      # empty scans are members too
    assert want["merged_points"].tolist() == [int(n[m].sum()) for m in mems] and all(x > 0 for x in want["merged_points"])
    assert all(len(r["label"]) > 0 for r in want["res"])


def test_too_many_scans():
    p, l, off, poses = le.too_many_scans()
    assert len(off) - 1 == le.MAX_SCANS + 1 == len(poses) and off[-1] == len(l)


def test_rotated_600():
    w, want = le.world("rotated-600"), le.expected("rotated-600")
    assert np.array_equal(w["poses"][:, [3, 7, 11]], le.world("lattice-600")["poses"][:, [3, 7, 11]]) and np.array_equal(w["p"], le.world("lattice-600")["p"])
    r = w["poses"][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].astype(np.float64).reshape(600, 3, 3)
    assert not np.array_equal(r @ r.transpose(0, 2, 1), np.tile(np.eye(3), (600, 1, 1)))
    mems = lists(want)
    assert len(mems) == 12 and all(20 <= len(m) <= 60 for m in mems), [len(m) for m in mems]
    assert np.all(np.diff(want["kp_off"]) > 0)
    differs = 0
    for m, (xyz, lab), res in zip(mems, want["clouds"], want["res"]):
        q, ql = le.f32_transform_cloud(w["p"], w["l"], w["off"], w["poses"], m)
        assert np.array_equal(ql, lab)
        differs += not np.array_equal(le.bits(sref.scan_rule(q, ql, w["cfg"])["xyz"]), le.bits(res["xyz"]))
    assert differs > 0


def test_anchors_4097():
    w, want = le.world("anchors-4097"), le.expected("anchors-4097")
    assert np.diff(w["off"]).tolist() == [2, 1, 2] and len(w["kw"]["anchors"]) == 4097 and w["kw"]["anchors"][:4] == [0, 1, 2, 0]
    assert want["merged_points"].tolist() == [5] * 4097 and ref.plan_passes(want["merged_points"], 0) == 2
    # the second pass holds exactly one anchor: 4096 anchors fill the first whatever their sizes
    assert ref.plan_passes(want["merged_points"][:4096], 0) == 1 and ref.plan_passes(want["merged_points"][4096:], 0) == 1
    assert np.all(np.diff(want["kp_off"]) == 3)


def test_euler_poses_keeps_its_draws():
    a, b = le.euler_poses(4, 13), le.euler_poses(4, 13, np.zeros((4, 3)))
    assert np.array_equal(a[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]], b[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]) and not b[:, [3, 7, 11]].any()
