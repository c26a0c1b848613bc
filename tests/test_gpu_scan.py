"""sgtd_scan_keypoints on the device against the numpy restatement of the rule in include/sgtd_accel.h
(tests/_scan_ref.py).  Everything is compared exactly: offsets, labels, counts and per-point cluster indices as
integers, centres bit for bit, grids as integers, minPolar / maxPolar bit for bit, the two pitches to 1e-12 degrees (the
device's asin is within a few ulp of numpy's; an ulp at 90 degrees is 1.4e-14).

The comparison is exact, so every scan must keep its points away from the rounding boundaries of the rule: every case
asserts _scan_ref.clear_of_boundaries first (the generator's seeds were chosen for that; the planted scenes sit at cell
centres)."""
import ctypes as C

import numpy as np
import pytest

import _scan_ref as ref
from _scan_edges import R0, R1, R2, bits, cell, edge_cfg, lib_cfg, restate, run, same_as, scene  # noqa: F401

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


def small_cfg(min_seg=2):
    cfg = ref.default_cfg()
    cfg["min_seg"] = np.full(32, min_seg, np.int64)
    return cfg


def check(h, points, labels, off, cfg=None, dev=False):
    """one call on handle h compared with the restatement; returns the restatement's per-scan results"""
    want = restate(points, labels, off, cfg)
    same_as(h, run(h, points, labels, off, cfg, dev), want)
    return want[0]


def scans(synth, counts, stream, **kw):
    kw.setdefault("n_blobs", 12)
    return synth.make_scans(len(counts), counts, stream=stream, **kw)


# ---- shapes ----
def shape_batches(tile):
    return {"one-0": [0], "one-1": [1], "one-64": [64], "two-empty-first": [0, 65], "two-empty-last": [63, 0],
            "one-tile": [tile], "five-tiles": [0, tile - 1, 0, tile + 1, 0], "five-blobs": [0, 20000, 0, 700, 0]}


@pytest.mark.parametrize("name", ["one-0", "one-1", "one-64", "two-empty-first", "two-empty-last", "one-tile", "five-tiles", "five-blobs"])
def test_shapes(g, mods, tile, name):
    counts = shape_batches(tile)[name]
    p, l, off = scans(mods[1], counts, stream=20 + len(name))
    res = check(g, p, l, off, small_cfg())
    if max(counts) >= 64:
        assert sum(len(r["label"]) for r in res) > 0
    if name == "five-blobs":
        assert sum(len(r["label"]) for r in res) >= 12 and max(int(r["n_points"].max()) for r in res if len(r["n_points"])) > 256


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_strides_and_pointers(g, mods, stride, dev):
    p, l, off = scans(mods[1], [3000, 0, 1500], stream=31, stride=stride)
    res = check(g, p, l, off, small_cfg(5), dev=dev)
    assert sum(len(r["label"]) for r in res) > 4


def test_instances_from_the_generator(g, mods):
    p, l, off = scans(mods[1], [4000, 2500], stream=33, instances=True)
    res = check(g, p, l, off)
    assert all((r["grid"][:, 0] == 1).any() and not (r["grid"][:, 0] == 2).any() for r in res)
    assert sum(len(r["label"]) for r in res) >= 20


def test_dropped_points(g, mods):
    p, l, off = scans(mods[1], [800, 800, 800, 800, 800], stream=35, stray=0.0)
    p, l = p.copy(), l.copy()
    p[0:800, :3] *= 40.0                                # scan 0: every point beyond max_range ...
    p[0:100, :3] *= 1e-4                                  # ... or inside min_range
    l[800:1600] = 0                                       # scan 1: every point of a dropped class
    l[1600:2400:2] = 40                                   # scan 2: sem >= 32 on every other point
    l[1601:2400:4] |= 1 << 15                             #         (and sem with a high bit)
    p[2400:3200:3, 0] = np.nan                            # scan 3: a coordinate that is not finite
    p[2401:3200:6, 2] = np.inf
    res = check(g, p, l, off, small_cfg())
    r = np.sqrt((p[:800, :3].astype(np.float64) ** 2).sum(axis=1))
    assert np.all((r >= 120.0) | (r <= 0.5))
    assert len(res[0]["label"]) == 0 and (res[0]["grid"][:, 0] == 2).any() and len(res[1]["label"]) == 0 and not res[1]["grid"].any()
    assert len(res[2]["label"]) > 0 and len(res[3]["label"]) > 0 and len(res[4]["label"]) > 0
    assert np.all(res[2]["cluster"][0::2] == -1) and np.all(res[3]["cluster"][0::3] == -1)


# ---- edges of the rule: scenes at cell centres ----
def edge_scenes():
    """name -> (points, labels, the n_points the rule must give, in keypoint order)"""
    s = {}
    s["min_seg"] = scene(cell(10, 0, R0, 4), cell(20, 0, R0, 5)) + ([5],)
    s["instances_20_21"] = scene(cell(10, 0, R0, 20, cls=10, inst=3), cell(40, 0, R0, 21, cls=10, inst=4)) + ([21],)
    # class 16: the only id is 0, voxel mode (its 30 points in one voxel: >= the 5 set below); class 17: ids {0, 7},
    # instance mode, the id-0 group first
    s["inst_zero"] = scene(cell(10, 0, R0, 30, cls=16), cell(30, 0, R0, 25, cls=17, inst=7), cell(90, 0, R0, 22, cls=17, inst=0),
                           cell(91, 0, R0, 3, cls=17, inst=0)) + ([30, 25, 25],)
    s["seam"] = scene(cell(300, 0, R0, 3), cell(0.25, 0, R0, 3)) + ([6],)
    # the top pitch layer: maxPitch = 3.7 cells, height = 3, the point T lies in layer 4 = height + 1 and reaches both
    # groups of layer 3 (azimuth cells 10 and 12), which do not reach it or each other
    s["top_layer"] = scene(cell(10, 3, R0, 3), cell(12, 3, R0, 3), cell(11, 3.7, R0, 1)) + ([7],)
    s["top_layer_apart"] = scene(cell(10, 3, R0, 5), cell(12, 3, R0, 5), cell(60, 3.7, R0, 1)) + ([5, 5],)
    s["adjacent_rings"] = scene(cell(10, 0, R0, 3), cell(10, 0, R1, 3)) + ([6],)
    s["rings_apart"] = scene(cell(10, 0, R0, 5), cell(10, 0, R2, 5)) + ([5, 5],)
    s["one_voxel_apart"] = scene(cell(10, 0, R0, 5), cell(12, 0, R0, 5)) + ([5, 5],)
    s["full_ring"] = scene(*[cell(k, 0, R0, 1) for k in range(1, 301)]) + ([300],)
    s["two_classes"] = scene(cell(10, 0, R0, 5, cls=15), cell(10, 0, R0, 5, cls=17), cell(11, 0, R0, 5, cls=17)) + ([5, 10],)
    s["sum_fold"] = scene(cell(10, 0, R0, 300, jitter=0.02, seed=1), cell(50, 0, R0, 256, jitter=0.02, seed=2),
                          cell(90, 0, R0, 257, jitter=0.02, seed=3)) + ([300, 256, 257],)
    # the component with the smaller voxel key (azimuth cell 10) has the larger first point index
    s["order"] = scene(cell(40, 0, R0, 6), cell(10, 0, R0, 5)) + ([6, 5],)
    return s


def test_edges_of_the_rule(g):
    sc = edge_scenes()
    names = list(sc)
    off = np.concatenate([[0], np.cumsum([len(sc[k][1]) for k in names])]).astype(np.int64)
    p, l = np.concatenate([sc[k][0] for k in names]), np.concatenate([sc[k][1] for k in names])
    res = check(g, p, l, off, edge_cfg())
    for k, r in zip(names, res):
        assert r["n_points"].tolist() == sc[k][2], k
    full = res[names.index("full_ring")]
    assert full["grid"][15].tolist() == [2, full["grid"][15][1], 301, 0] and np.all(full["cluster"] == 0)
    top = res[names.index("top_layer")]
    assert top["grid"][15][3] == 3
    order = res[names.index("order")]
    assert order["cluster"].tolist() == [0] * 6 + [1] * 5
    # the same scenes, each alone in its batch
    for k in ("seam", "top_layer", "full_ring", "sum_fold"):
        check(g, sc[k][0], sc[k][1], [0, len(sc[k][1])], edge_cfg())


def test_full_ring_at_class_10s_300(g):
    """the chain of 300 single-point voxels is exactly the default min_seg of class 10; one point fewer is dropped"""
    p, l = scene(*[cell(k, 0, R0, 1, cls=10) for k in range(1, 301)])
    off = np.array([0, 300, 599], np.int64)
    res = check(g, np.concatenate([p, p[:299]]), np.concatenate([l, l[:299]]), off)
    assert res[0]["n_points"].tolist() == [300] and res[1]["n_points"].tolist() == []


# ---- behaviour ----
def status(h, fn, *args):
    return getattr(h._L, fn)(h._h, *args)


def test_getters_before_a_run_and_capacity(mods):
    h = mods[0].STDescManager()
    n = C.c_int64(0)
    off = np.zeros(4, np.int64)
    buf = np.zeros(4096, np.int32)
    pv = lambda a: a.ctypes.data_as(C.c_void_p)
    assert status(h, "sgtd_result_scan_keypoints", pv(off), None, None, None, 0, C.byref(n)) == -7
    assert status(h, "sgtd_result_scan_point_clusters", 0, None, 0, C.byref(n)) == -7
    assert status(h, "sgtd_result_scan_grids", 0, None, None) == -7
    assert status(h, "sgtd_scan_device_view", None, None) == -7
    p, l, o = scans(mods[1], [1500, 900], stream=41)
    xyz, lab, kp_off, npts = h.scan_keypoints(p, l, o, lib_cfg(small_cfg()))
    k = len(lab)
    assert k > 2
    x1, l1, n1 = np.full((k, 3), -1.0, np.float32), np.zeros(k, np.uint32), np.zeros(k, np.int32)
    assert status(h, "sgtd_result_scan_keypoints", pv(off), pv(x1), pv(l1), pv(n1), k - 1, C.byref(n)) == -4 and n.value == k
    assert np.array_equal(x1[:k - 1], xyz[:k - 1]) and np.all(x1[k - 1] == -1.0) and np.array_equal(n1[:k - 1], npts[:k - 1])
    assert status(h, "sgtd_result_scan_point_clusters", 1, pv(buf), 899, C.byref(n)) == -4 and n.value == 900
    assert np.array_equal(buf[:899], h.scan_point_clusters(1)[:899])
    assert status(h, "sgtd_result_scan_point_clusters", 2, pv(buf), 4096, C.byref(n)) == -1
    assert status(h, "sgtd_result_scan_grids", -1, None, None) == -1
    # bad arguments with a handle: SGTD_ERR_INVALID, and the earlier results stay
    bad_off = np.array([0, 5, 3], np.int64)
    cfg = h.default_scan_config()
    assert status(h, "sgtd_scan_keypoints", None, pv(p), 4, pv(l), pv(o), -1, 0) == -1
    assert status(h, "sgtd_scan_keypoints", None, None, 4, pv(l), pv(o), 2, 0) == -1
    assert status(h, "sgtd_scan_keypoints", None, pv(p), 4, None, pv(o), 2, 0) == -1
    assert status(h, "sgtd_scan_keypoints", None, pv(p), 4, pv(l), None, 2, 0) == -1
    assert status(h, "sgtd_scan_keypoints", None, pv(p), 2, pv(l), pv(o), 2, 0) == -1
    assert status(h, "sgtd_scan_keypoints", None, pv(p), 4, pv(l), pv(bad_off), 2, 0) == -1
    cfg.min_range = 200.0
    assert status(h, "sgtd_scan_keypoints", C.byref(cfg), pv(p), 4, pv(l), pv(o), 2, 0) == -1
    cfg = h.default_scan_config()
    cfg.delta_r = 0.01
    assert status(h, "sgtd_scan_keypoints", C.byref(cfg), pv(p), 4, pv(l), pv(o), 2, 0) == -6
    assert b"rings" in h._L.sgtd_last_error(h._h)
    assert np.array_equal(h.scan_results()[0], xyz)
    # a second call replaces the first's results
    p2, l2, o2 = scans(mods[1], [700], stream=42)
    second = h.scan_keypoints(p2, l2, o2, lib_cfg(small_cfg()))
    assert len(second[2]) == 2 and status(h, "sgtd_result_scan_grids", 1, None, None) == -1
    again = h.scan_results()
    assert all(np.array_equal(a, b) for a, b in zip(second, again))
    h.close()


def keypoint_scans(synth, n_scans, stream):
    """scans of 40 blobs each: enough keypoints for descriptors"""
    return synth.make_scans(n_scans, 6000, stream=stream, n_blobs=40, sigma=(0.05, 0.12))


def same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("n_cand", "cand_frame", "cand_votes", "pair_off"))


def test_query_scans_equals_query_frames(mods):
    manager, synth, _ = mods
    cfg = lib_cfg(small_cfg(20))
    mp, ml, mo = keypoint_scans(synth, 6, 51)
    a, b = manager.STDescManager(), manager.STDescManager()
    kp_off = a.add_scans(mp, ml, mo, cfg)
    xyz, lab, off, _ = a.scan_results()
    assert np.array_equal(off, kp_off) and np.all(np.diff(off) >= 20)
    b.add_frames(xyz, lab, off)
    q = slice(int(mo[1]), int(mo[4]))
    qo = mo[1:5] - mo[1]
    ra = a.query_scans(mp[q], ml[q], qo, cfg)
    qx, ql, qoff, _ = a.scan_results()
    rb = b.query_frames(qx, ql, qoff)
    assert same(ra, rb) and np.all(ra.n_cand > 0) and ra.cand_frame[:, 0].tolist() == [1, 2, 3]
    for k in range(3):
        for x, y in zip(a.result_pairs(k, ra), b.result_pairs(k, rb)):
            assert np.array_equal(x, y)
    # a pending batch's results are unchanged by a scan call in between
    b.query_frames(qx, ql, qoff, fetch=False)
    b.scan_keypoints(mp[:int(mo[1])], ml[:int(mo[1])], mo[:2], cfg)
    assert same(b.results(), rb)
    assert len(b.scan_results()[2]) == 2
    a.close()
    b.close()


def test_view_and_shards(mods):
    manager, synth, _ = mods
    cfg = lib_cfg(small_cfg(5))
    p, l, o = scans(synth, [5000, 0, 2500], stream=61)
    single, multi, view = manager.STDescManager(), manager.STDescManager(devices=[0, 0, 0]), manager.STDescManager()
    view.attach_table(single)
    want = single.scan_keypoints(p, l, o, cfg)
    assert len(want[1]) > 4
    single.add_frames(want[0], want[1], want[2])      # the owner's table has changed under the view: the call does not look at it
    for h in (multi, view):
        got = h.scan_keypoints(p, l, o, cfg)
        assert all(np.array_equal(bits(a) if a.dtype.kind == "f" else a, bits(b) if b.dtype.kind == "f" else b) for a, b in zip(want, got))
        for s in range(3):
            assert np.array_equal(h.scan_point_clusters(s), single.scan_point_clusters(s))
            assert all(np.array_equal(x, y) for x, y in zip(h.scan_grids(s), single.scan_grids(s)))
    kp_off = multi.add_scans(p, l, o, cfg)
    assert np.array_equal(kp_off, want[2])
    view.close()
    multi.close()
    single.close()
