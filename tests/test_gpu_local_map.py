"""sgtd_local_map_keypoints on the device against the numpy restatement of the rule in include/sgtd_accel.h
(tests/_local_map_ref.py, which ends in tests/_scan_ref.py's scan rule).  Everything is compared exactly: offsets,
labels, counts, member lists and merged sizes as integers, centres bit for bit.

The comparison is exact, so every merged cloud must keep its points away from the rounding boundaries of the scan rule:
every case asserts _scan_ref.clear_of_boundaries on every merged cloud first (the seeds were chosen for that; no case
redraws at run time)."""
import ctypes as C

import numpy as np
import pytest

import _local_map_ref as ref
import _scan_ref as sref
from _local_map_edges import bits, euler_poses, eye_poses, lib_cfg, restate, same_as  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, manager, synth
    return manager, synth, _lib


@pytest.fixture(scope="module")
def g(mods):
    h = mods[0].STDescManager()
    yield h
    h.close()


@pytest.fixture(scope="module")
def tile(mods):
    t = C.c_int(0)
    mods[2].lib().sgtd_scan_tiles(C.byref(t))
    return t.value


def check(h, p, l, off, poses, cfg, dev=False, want=None, **kw):
    """one call on handle h compared with the restatement, which is returned"""
    off = np.asarray(off, np.int64)
    want = want or restate(p, l, off, poses, cfg, **kw)
    if dev:
        import torch
        dp, dl = torch.from_numpy(np.ascontiguousarray(p)).cuda(), torch.from_numpy(l.view(np.int32)).cuda()
        got = h.local_map_keypoints(dp, dl, off, poses, config=lib_cfg(cfg), **kw)
    else:
        got = h.local_map_keypoints(p, l, off, poses, config=lib_cfg(cfg), **kw)
    same_as(h, got, want, kw.get("max_pass_points", 0))
    return want


def scans(synth, counts, stream, **kw):
    kw.setdefault("n_blobs", 12)
    return synth.make_scans(len(counts), counts, stream=stream, **kw)


# ---- shapes ----
SHAPES = {
    # name: (counts, stream, radius, anchors)
    "no-scans": ([], 1, 7.0, None),
    "no-anchors": ([600, 64], 2, 7.0, []),
    "two-in-range": ([600, 700], 3, 7.0, None),
    "three-one-out-of-range": ([500, 400, 300], 4, 4.0, None),
    "empty-anchor-and-empty-neighbours": ([0, 600, 0], 5, 7.0, None),
    "subset-out-of-order-with-a-repeat": ([600, 0, 1023, 1025, 64], 6, 7.0, [3, 0, 3, 2]),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(g, mods, name):
    counts, stream, radius, anchors = SHAPES[name]
    p, l, off = scans(mods[1], counts, stream)
    want = check(g, p, l, off, ref.path_poses(len(counts)), ref.small_cfg(), radius=radius, anchors=anchors)
    if name == "three-one-out-of-range":
        assert want["member"].tolist() == [0, 1, 1, 0, 2, 2, 1]
    if name == "empty-anchor-and-empty-neighbours":
        assert want["merged_points"].tolist() == [600, 600, 600] and np.all(np.diff(want["kp_off"]) > 0)
    if name == "subset-out-of-order-with-a-repeat":
        k = want["kp_off"]
        assert np.array_equal(want["xyz"][k[0]:k[1]], want["xyz"][k[2]:k[3]]) and k[1] > 0
    if counts and anchors is None:
        assert want["kp_off"][-1] > 0


def test_one_scan_equals_scan_keypoints(g, mods):
    p, l, off = scans(mods[1], [900], 7)
    cfg = ref.small_cfg()
    want = check(g, p, l, off, ref.path_poses(1), cfg)
    got = g.local_map_results()
    single = g.scan_keypoints(p, l, off, lib_cfg(cfg))
    assert len(single[1]) > 2 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, single))
    assert want["member"].tolist() == [0]


# ---- tile edges of the gather ----
def test_member_sizes_at_the_tile_edges(g, mods, tile):
    counts = [tile - 1, 1, tile + 1, 0, 2 * tile]
    p, l, off = scans(mods[1], counts, 8)
    want = check(g, p, l, off, ref.path_poses(5), ref.small_cfg(), radius=100.0)
    assert want["merged_points"].tolist() == [sum(counts)] * 5 and np.all(np.diff(want["mem_off"]) == 5)


def test_more_segments_than_lanes_in_a_tile(g, mods, tile):
    counts = (1 + np.arange(70) % 3).tolist()
    p, l, off, poses = mods[1].make_posed_scans(70, counts, stream=9, spacing=0.1, n_blobs=20, sensor_range=30.0, extent=10.0)
    want = check(g, p, l, off, poses, ref.small_cfg(), radius=15.0)
    assert len(want["member"]) == 4900 and int(want["merged_points"][0]) == sum(counts) < tile and want["kp_off"][-1] > 70


# ---- radius ----
def test_radius_is_inclusive_to_the_ulp(g, mods):
    p, l, off = scans(mods[1], [300, 300], 10)
    cfg = ref.small_cfg()
    on = check(g, p, l, off, eye_poses([[0, 0, 0], [3, 4, 0]]), cfg, radius=5.0)
    assert on["member"].tolist() == [0, 1, 1, 0]
    beyond = check(g, p, l, off, eye_poses([[0, 0, 0], [np.nextafter(np.float32(3.0), np.float32(4.0)), 4, 0]]), cfg, radius=5.0)
    assert beyond["member"].tolist() == [0, 1]
    zero = check(g, p, l, off, eye_poses([[1, 2, 3], [1, 2, 3]]), cfg, radius=0.0)
    assert zero["member"].tolist() == [0, 1, 1, 0]


# ---- bad poses ----
def test_bad_poses(g, mods):
    p, l, off = scans(mods[1], [400, 300, 500], 11)
    cfg = ref.small_cfg()
    base = ref.path_poses(3)
    nan_t = base.copy()
    nan_t[1, 7] = np.nan
    want = check(g, p, l, off, nan_t, cfg, radius=7.0)
    assert want["member"].tolist() == [0, 2, 1, 2, 0]
    inf_t = base.copy()
    inf_t[1, 3] = np.inf
    want = check(g, p, l, off, inf_t, cfg, radius=7.0)
    assert want["member"].tolist() == [0, 2, 1, 2, 0]
    # a NaN in scan 1's rotation: its points are dropped from the others' maps, whose keypoints are those of the maps
    # without it; in its own map the others' points are dropped
    nan_r = base.copy()
    nan_r[1, 5] = np.nan
    want = check(g, p, l, off, nan_r, cfg, radius=7.0)
    assert want["member"].tolist() == [0, 1, 2, 1, 0, 2, 2, 0, 1]
    keep = np.r_[0:400, 700:1200]
    without = ref.local_map_rule(p[keep], l[keep], [0, 400, 900], base[[0, 2]], radius=7.0, cfg=cfg)
    alone = sref.scan_rule(p[400:700], l[400:700], cfg)
    k = want["kp_off"]
    assert np.array_equal(bits(want["xyz"][:k[1]]), bits(without["res"][0]["xyz"])) and np.array_equal(bits(want["xyz"][k[2]:]), bits(without["res"][1]["xyz"]))
    assert np.array_equal(bits(want["xyz"][k[1]:k[2]]), bits(alone["xyz"])) and k[1] > 0 and k[2] > k[1]


# ---- max_members ----
def test_max_members(g, mods):
    p, l, off = scans(mods[1], [200] * 5, 12)
    cfg = ref.small_cfg()
    poses = eye_poses([[2, 0, 0], [1, 0, 0], [0, 0, 0], [-1, 0, 0], [-3, 0, 0]])      # 1 and 3 are equally far from 2
    lists = {}
    for m in (1, 2, 3, 9):
        want = check(g, p, l, off, poses, cfg, radius=5.0, max_members=m)
        lists[m] = want["member"][want["mem_off"][2]:want["mem_off"][3]].tolist()
    assert lists == {1: [2], 2: [2, 1], 3: [2, 1, 3], 9: [2, 0, 1, 3, 4]}


# ---- rotations, strides, pointers ----
def test_general_rotations(g, mods):
    p, l, off = scans(mods[1], [500, 300, 400, 200], 13)
    poses = euler_poses(4, 13)
    r = poses[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].astype(np.float64).reshape(4, 3, 3)
    assert not np.array_equal(r @ r.transpose(0, 2, 1), np.tile(np.eye(3), (4, 1, 1)))
    want = check(g, p, l, off, poses, ref.small_cfg(), radius=15.0)
    assert np.all(np.diff(want["mem_off"]) == 4) and want["kp_off"][-1] > 20


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_strides_and_pointers(g, mods, stride, dev):
    p, l, off = scans(mods[1], [700, 0, 500], 14, stride=stride)
    want = check(g, p, l, off, ref.path_poses(3), ref.small_cfg(), dev=dev, radius=7.0)
    assert want["kp_off"][-1] > 10


# ---- passes ----
def test_passes_do_not_change_the_result(mods):
    h = mods[0].STDescManager()
    counts = [600, 0, 1023, 1025, 64, 300]
    p, l, off = scans(mods[1], counts, 15)
    poses, cfg = ref.path_poses(6), ref.small_cfg()
    want = restate(p, l, off, poses, cfg, radius=7.0)
    merged = want["merged_points"].tolist()
    assert merged == [1623, 2648, 2712, 2412, 2412, 1389]
    largest = max(merged)
    # default: one pass; the largest merged size: no two anchors share a pass and none is refused;
    # 2712 + 2412: anchors 0 1 | 2 3 | 4 5, the middle pass filled to the last point
    for cap, passes in ((0, 1), (largest, 6), (2712 + 2412, 3)):
        assert ref.plan_passes(merged, cap) == passes
        check(h, p, l, off, poses, cfg, want=want, radius=7.0, max_pass_points=cap)
    # one below the largest: refused before any clustering, no results, the handle goes on
    with pytest.raises(mods[2].SgtdError) as err:
        h.local_map_keypoints(p, l, off, poses, radius=7.0, max_pass_points=largest - 1, config=lib_cfg(cfg))
    assert err.value.status == -6 and "anchor 2" in str(err.value) and str(largest) in str(err.value)
    n = C.c_int64(0)
    assert h._L.sgtd_result_local_map_keypoints(h._h, None, None, None, None, 0, C.byref(n)) == -7
    assert h._L.sgtd_result_local_map_members(h._h, None, None, 0, C.byref(n), None, None) == -7
    assert h._L.sgtd_local_map_device_view(h._h, None, None) == -7
    check(h, p, l, off, poses, cfg, want=want, radius=7.0)
    h.close()


# ---- state ----
def test_getters_capacity_and_the_scan_results(mods):
    h = mods[0].STDescManager()
    L = h._L
    pv = lambda a: a.ctypes.data_as(C.c_void_p)
    n, passes = C.c_int64(0), C.c_int32(0)
    assert L.sgtd_result_local_map_keypoints(h._h, None, None, None, None, 0, C.byref(n)) == -7
    assert L.sgtd_result_local_map_members(h._h, None, None, 0, C.byref(n), None, None) == -7
    assert L.sgtd_local_map_device_view(h._h, None, None) == -7
    p, l, off = scans(mods[1], [600, 500, 400], 16)
    poses, cfg = ref.path_poses(3), lib_cfg(ref.small_cfg())
    first = h.scan_keypoints(p, l, off, cfg)
    xyz, lab, kp_off, npts = h.local_map_keypoints(p, l, off, poses, radius=7.0, config=cfg)
    k = len(lab)
    assert k > 3
    # the scan results were clustered over: their getters say so until a scan call has run again
    assert L.sgtd_result_scan_keypoints(h._h, None, None, None, None, 0, C.byref(n)) == -7
    assert L.sgtd_scan_device_view(h._h, None, None) == -7
    # capacity too small: the size reported, the first entries written
    o1, x1, l1, n1 = np.zeros(4, np.int64), np.full((k, 3), -1.0, np.float32), np.zeros(k, np.uint32), np.zeros(k, np.int32)
    assert L.sgtd_result_local_map_keypoints(h._h, pv(o1), pv(x1), pv(l1), pv(n1), k - 1, C.byref(n)) == -4 and n.value == k
    assert np.array_equal(o1, kp_off) and np.array_equal(x1[:k - 1], xyz[:k - 1]) and np.all(x1[k - 1] == -1.0)
    assert np.array_equal(n1[:k - 1], npts[:k - 1]) and np.array_equal(l1[:k - 1], lab[:k - 1])
    mem = np.full(9, -1, np.int32)
    mo, merged = np.zeros(4, np.int64), np.zeros(3, np.int64)
    assert L.sgtd_result_local_map_members(h._h, pv(mo), pv(mem), 8, C.byref(n), pv(merged), C.byref(passes)) == -4 and n.value == 9
    assert mem.tolist() == [0, 1, 2, 1, 0, 2, 2, 0, -1] and mo.tolist() == [0, 3, 6, 9] and merged.tolist() == [1500] * 3 and passes.value == 1
    # a scan call makes the scan results valid again and leaves the local-map results alone
    again = h.scan_keypoints(p, l, off, cfg)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    kept = h.local_map_results()
    assert all(np.array_equal(a, b) for a, b in zip(kept, (xyz, lab, kp_off, npts)))
    # bad arguments with a handle: SGTD_ERR_INVALID, and the results stay
    opt = mods[2].LocalMapOptions()
    L.sgtd_default_local_map_options(C.byref(opt))
    args = (pv(p), 4, pv(l), pv(off), pv(poses), 3)
    anch = np.array([0, 3], np.int32)
    assert L.sgtd_local_map_keypoints(h._h, None, C.byref(opt), *args, pv(anch), 2, 0) == -1
    assert L.sgtd_local_map_keypoints(h._h, None, C.byref(opt), *args, pv(anch), -1, 0) == -1
    assert L.sgtd_local_map_keypoints(h._h, None, C.byref(opt), pv(p), 4, pv(l), pv(off), None, 3, None, 0, 0) == -1
    for field, bad in (("radius", float("nan")), ("radius", -1.0), ("radius", float("inf")), ("max_members", -1), ("max_pass_points", -1),
                       ("max_pass_points", (1 << 28) + 1), ("reserved", 1)):
        L.sgtd_default_local_map_options(C.byref(opt))
        setattr(opt, field, bad)
        assert L.sgtd_local_map_keypoints(h._h, None, C.byref(opt), *args, None, 0, 0) == -1, field
    assert all(np.array_equal(a, b) for a, b in zip(h.local_map_results(), (xyz, lab, kp_off, npts)))
    h.close()


# ---- through the manager ----
def world(synth):
    return synth.make_posed_scans(8, 3000, stream=21, spacing=2.0, n_blobs=60, sensor_range=40.0)


def same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("n_cand", "cand_frame", "cand_votes", "pair_off"))


def test_add_and_query_local_maps(mods):
    manager, synth, _ = mods
    cfg = lib_cfg(ref.small_cfg(20))
    p, l, off, poses = world(synth)
    a, b = manager.STDescManager(), manager.STDescManager()
    kw = dict(radius=5.0, config=cfg)
    kp_off = a.add_local_maps(p, l, off, poses, **kw)
    xyz, lab, o, _ = a.local_map_results()
    assert np.array_equal(o, kp_off) and np.all(np.diff(o) >= 20)
    b.add_frames(xyz, lab, o)
    b.set_frame_poses(np.arange(8), poses)
    for x, y in zip(a.table_dump(), b.table_dump()):
        assert np.array_equal(x, y)
    anchors = [2, 5, 6]
    ra = a.query_local_maps(p, l, off, poses, anchors=anchors, radius=3.0, config=cfg)
    qx, ql, qo, _ = a.local_map_results()
    rb = b.query_frames(qx, ql, qo)
    # (every frame of this short path sees the same blobs: which frame wins is not the point, that both sides agree is)
    assert same(ra, rb) and np.all(ra.n_cand > 0) and np.array_equal(ra.cand_frame[:, 0], rb.cand_frame[:, 0])
    a.verify()
    b.verify()
    for q in range(3):
        for x, y in zip(a.result_pairs(q, ra), b.result_pairs(q, rb)):
            assert np.array_equal(x, y)
        wa, wb = a.result_world_poses(q), b.result_world_poses(q)
        assert np.array_equal(bits(wa), bits(wb)) and np.isfinite(wa[0]).all()
    a.close()
    b.close()


def test_view_and_shards(mods):
    manager, synth, _ = mods
    cfg = lib_cfg(ref.small_cfg(20))
    p, l, off, poses = world(synth)
    single, multi, view = manager.STDescManager(), manager.STDescManager(devices=[0, 0, 0]), manager.STDescManager()
    want = single.local_map_keypoints(p, l, off, poses, radius=5.0, config=cfg)
    single.add_frames(want[0], want[1], want[2])
    view.attach_table(single)
    single.query_frames(want[0], want[1], want[2], fetch=False)      # the owner holds a pending batch
    for h in (multi, view):
        got = h.local_map_keypoints(p, l, off, poses, radius=5.0, config=cfg)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(want, got))
    kp_off = multi.add_local_maps(p, l, off, poses, radius=5.0, config=cfg)
    assert np.array_equal(kp_off, want[2])
    assert np.all(single.results().n_cand > 0)
    view.close()
    multi.close()
    single.close()
