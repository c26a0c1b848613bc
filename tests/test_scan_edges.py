"""The worlds of tests/_scan_edges.py reach their edges, and every mutant of the restatement changes the world named for
it: shown on the CPU with tests/_scan_ref.py alone.  The GPU side is tests/test_gpu_scan_edges.py: a device kernel that is
wrong in the way a mutant is wrong fails there."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _scan_edges as se  # noqa: E402
import _scan_ref as ref  # noqa: E402


def one(name):
    """a one-scan world: points, labels, cfg and the restatement's result"""
    p, l, off, cfg = se.world(name)
    assert len(off) == 2
    return p, l, cfg, se.expected(name)[0][0]


def changed(name, mutant):
    p, l, cfg, want = one(name)
    return not se.same_result(se.scan_rule(p, l, cfg, mutant), want)


def voxels(name):
    p, l, cfg, _ = one(name)
    _, vox, dims = ref.voxel_mode_points(p, l, 15, cfg)
    return vox, dims


@pytest.mark.parametrize("name", list(se.WORLDS))
def test_worlds_are_clear_and_the_unchanged_copy_is_the_restatement(name):
    p, l, off, cfg = se.world(name)
    res = se.expected(name)[0]      # (asserts clear_of_boundaries per scan)
    for s in range(0, len(off) - 1, 16):
        a, b = off[s], off[s + 1]
        assert se.same_result(se.scan_rule(p[a:b], l[a:b], cfg), res[s])


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_big_clusters_at_the_hand_over(n):
    name = "big-%d" % n
    _, _, _, want = one(name)
    assert want["n_points"].tolist() == [n, 300] and se.BIG == 4096
    assert changed(name, "plain_sum")
    p, l, cfg, _ = one(name)
    got = se.scan_rule(p, l, cfg, "block_fold")
    first = not np.array_equal(se.bits(got["xyz"][0]), se.bits(want["xyz"][0]))
    assert first == (n >= se.BIG) and np.array_equal(se.bits(got["xyz"][1]), se.bits(want["xyz"][1]))


def test_big_two():
    _, _, _, want = one("big-two")
    n = want["n_points"]
    big = np.nonzero(n >= se.BIG)[0].tolist()
    assert len(n) == 42 and big == [1, 41] and all(k % 4 for k in big) and np.all(n[2:41] < 256) and n[0] < 256
    assert changed("big-two", "block_fold") and changed("big-two", "plain_sum")


def test_big_instance():
    p, l, cfg, want = one("big-instance")
    assert want["n_points"].tolist() == [21, 4096] and want["grid"][10, 0] == 1 and int((l >> 16).max()) == 0xFFFF
    assert np.all(want["cluster"][l >> 16 == 0xFFFF] == 1) and np.all(want["cluster"][l >> 16 == 0x7FFF] == -1)
    got = se.scan_rule(p, l, cfg, "inst15")
    assert got["n_points"].tolist() == [21, 4116]      # the ids 0x7FFF and 0xFFFF merged
    assert changed("big-instance", "block_fold")


def test_small_sums():
    _, _, cfg, want = one("small-sums")
    assert want["n_points"].tolist() == [1, 63, 64, 65, 255] and cfg["min_seg"][15] == 1
    assert changed("small-sums", "plain_sum") and not changed("small-sums", "block_fold")


def test_block27_reaches_the_cap():
    _, _, _, want = one("block27")
    assert want["n_points"].tolist() == [27]
    vox, dims = voxels("block27")
    order, _, links = se.voxel_links(vox, dims)
    full = [k for k, l in zip(order, links) if len(l) == 26]
    assert len(full) == 1 and max(len(l) for l in links) == 26      # == SGTD_SCAN_NBR
    pit, pol, azi = full[0]
    occupied = set(order)
    assert sum(nb in occupied and nb != full[0] for nb in ref.neighbours(pol, pit, azi, *dims)) == 26
    # a list cut at 25 still gives the one cluster of 27: the world shows that the cap is reached, not that a lower one
    # breaks it (the symmetric link from the dropped neighbour holds the component together)
    assert not changed("block27", "nbr25")
    assert max(len(l) for l in se.voxel_links(vox, dims, cap=25)[2]) == 25


def test_last_azimuth():
    p, l, cfg, want = one("last-azimuth")
    assert want["n_points"].tolist() == [6] and want["grid"][15, 2] == 301
    vox, dims = voxels("last-azimuth")
    assert sorted(set(vox[:6, 2].tolist())) == [0, 299, 300] and sorted(set(vox[:6, 0].tolist())) == [0, 1]
    occupied = set(tuple(int(c) for c in v) for v in vox)
    nb = [t for t in ref.neighbours(vox[1, 1], vox[1, 0], 300, *dims) if t in occupied and t != tuple(int(c) for c in vox[1])]
    assert vox[1, 2] == 300 and len(nb) > len(set(nb)) and nb.count((1, int(vox[1, 1]), 300)) == 2
    got = se.scan_rule(p, l, cfg, "no_wrap")
    assert got["n_points"].tolist() == [] and len(set(se._components(vox[:6], dims, "no_wrap").tolist())) == 2


def test_zigzag():
    p, l, cfg, want = one("zigzag")
    assert want["n_points"].tolist() == [64] and np.all(want["cluster"][:64] == 0)
    assert se.world_rounds(p, l, cfg) == 3
    vox, dims = voxels("zigzag")
    assert len(set(se._components(vox[:64], dims, "hook_once").tolist())) == 32
    assert changed("zigzag", "hook_once")


def test_percolation():
    p, l, cfg, want = one("percolation")
    n = want["n_points"].tolist()
    assert len(n) > 50 and len(set(n)) > 10 and cfg["min_seg"][15] == 2
    vox, _ = voxels("percolation")
    assert len(set(map(tuple, vox.tolist()))) == len(vox)      # one point per voxel
    assert abs((len(vox) - 1) / (se.PERC_ROWS * se.PERC_COLS) - se.PERC_P) < 0.02
    assert se.world_rounds(p, l, cfg) == 5
    assert changed("percolation", "hook_once") and changed("percolation", "min_order_by_voxel")


def test_min_order_by_voxel_changes_the_order_scene():
    # test_gpu_scan.py's "order": the component with the smaller voxel key (azimuth cell 10) has the larger first point index
    p, l = se.scene(se.cell(40, 0, se.R0, 6), se.cell(10, 0, se.R0, 5))
    assert ref.scan_rule(p, l, se.edge_cfg())["n_points"].tolist() == [6, 5]
    assert se.scan_rule(p, l, se.edge_cfg(), "min_order_by_voxel")["n_points"].tolist() == [5, 6]


def test_all_dropped_and_one_live():
    p, l, off, cfg = se.world("all-dropped")
    res, xyz, lab, kp_off, npts = se.expected("all-dropped")
    assert len(res) == 3 and kp_off.tolist() == [0, 0, 0, 0] and len(lab) == 0 and all(not r["grid"].any() for r in res)
    assert not ref.kept_mask(p, l, cfg).any() and all(np.all(r["cluster"] == -1) for r in res)
    assert np.all(cfg["node_label"][l[:40] & 0xFFFF] == 0) and np.all((l[40:70] & 0xFFFF) >= 32) and not np.isfinite(p[70:]).all(axis=1).any()
    res, xyz, lab, kp_off, npts = se.expected("one-live")
    assert kp_off.tolist() == [0, 0, 0, 1] and npts.tolist() == [1] and res[2]["cluster"].tolist() == [-1] * 50 + [0]


def test_257_scans():
    p, l, off, cfg = se.world("257-scans")
    res, xyz, lab, kp_off, npts = se.expected("257-scans")
    n = np.diff(off)
    empty = n == 0
    assert len(off) == 258 and len(kp_off) == 258 and empty.sum() == 16 and np.all(empty[15::16]) and set(n[~empty].tolist()) == set(range(4, 10))
    assert kp_off[-1] > 256 and kp_off[256] <= 256 + 48 and np.all(np.diff(kp_off)[empty] == 0) and np.all(np.diff(kp_off)[~empty] >= 1)
    assert (np.diff(kp_off) == 2).sum() >= 16 and int(npts.sum()) == len(l)


def test_the_concatenation_is_one_batch_of_more_than_260_scans():
    p, l, off, cfg = se.concatenated()
    res, xyz, lab, kp_off, npts = se.expected_concatenated()
    assert len(off) - 1 > 260 and off[-1] == len(l) and np.all(np.diff(off) >= 0)
    assert (npts >= se.BIG).sum() == 3 and kp_off[-1] > 256 + 42 + 50
    # (under the batch's min_seg 2 each world gives what it gives alone, up to clusters of 2 to 4 points)
    alone = se.expected("big-4096")[0][0]
    assert np.array_equal(se.bits(res[0]["xyz"]), se.bits(alone["xyz"]))


def test_rounds_model_on_known_shapes():
    chain = np.array([[0, 40, k] for k in range(10, 40)])
    assert se.rounds_model(chain, (60, 301, 0)) == 2      # an ascending chain: one hooking round, one that hooks nothing
    assert se.rounds_model(chain[:1], (60, 301, 0)) == 1
    ring = np.array([[0, 40, k] for k in range(1, 301)])
    assert se.rounds_model(ring, (60, 301, 0)) == 2


def test_too_many_scans():
    p, l, off = se.too_many_scans()
    assert len(off) - 1 == se.MAX_SCANS + 1 and off[-1] == len(l)
