"""sgtd_register_stored_voxels at its edges, bit for bit against sgtd_register_voxels on the concatenated clouds and the
restatement (tests/_voxel_register_ref.py): sizes around the tiles of the kernels on both sides, a voxel whose points come
from two stored members around the width of VSUM, points that enter no voxel, and the store's history, which must not show:
the same frames in another order, overwritten and forgotten frames (dead slots between the members), a growth and a
compaction between two calls, strides 3 and 4, points from the host and on the device."""
import contextlib

import numpy as np
import pytest

import _register_edges as rx
import _register_ref as ref
import _stored_edges as sx
import _stored_voxel_edges as svx
import _voxel_register_edges as vx
import _voxel_register_ref as vref
import test_gpu_register_stored_edges as se      # (its histories of the store: _arrive, init_points)

pytestmark = pytest.mark.gpu

OPT = dict(k_neighbors=8, neighbor_mode=7, max_iterations=30)


@pytest.fixture(scope="module")
def manager():
    from sgtd_amd import manager
    return manager


@pytest.fixture(scope="module")
def scene():
    """the frames' final clouds (test_gpu_register_stored_edges' ids and sizes), the call's clouds, maps over the frames and
    pairs, and clouds to overwrite with"""
    s, t, R, tm = rx.surfaces(300, 1200, 5)
    rng = np.random.default_rng(8)
    cut = lambda n: t[rng.permutation(len(t))[:n]].copy()      # noqa: E731
    final = {1: cut(127), 4: cut(0), 6: cut(300), 30: cut(129), 31: cut(64)}
    calls = [s[:150], s[150:278]]
    members = [[6], [1, 30, 31], [4], [31, 6, 4, 1], [30, 30]]
    map_off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    map_frame = np.array([f for m in members for f in m], np.uint32)
    rng = np.random.default_rng(2)
    map_pose = np.array([vx.pose_row(rng.normal(0, 1, 3), 0.002 * k, rng.normal(0, 0.02, 3)) for k in range(len(map_frame))])
    src = [a for a in range(2) for _ in members]
    tgt = [m for _ in range(2) for m in range(len(members))]
    init = np.array([ref.near_start(R, tm)] * len(src))
    return dict(final=final, calls=calls, map_off=map_off, map_frame=map_frame, map_pose=map_pose, src=src, tgt=tgt, init=init,
                spare=[cut(400), cut(50), cut(0), cut(310), cut(290)])


def _run(h, scene, **kw):
    return svx.run(h, scene["calls"], scene["map_off"], scene["map_frame"], scene["map_pose"], scene["src"], scene["tgt"], scene["init"], **dict(OPT, **kw))


@pytest.fixture(scope="module")
def want(manager, scene):
    """what one set call gives, checked against sgtd_register_voxels and the restatement"""
    h = manager.STDescManager()
    sx.store(h, scene["final"], k_neighbors=8)
    got, _ = svx.check(h, scene["calls"], scene["final"], scene["map_off"], scene["map_frame"], scene["map_pose"], scene["src"], scene["tgt"],
                       scene["init"], "one call", **OPT)
    h.close()
    print("one call: status", got["status"].tolist(), "iterations", got["iterations"].tolist())
    assert max(len(m["n_points"]) for m in got["maps"]) > 1 and (got["status"] == vref.CONVERGED).any(), "no pair converges"
    assert (got["status"] != vref.NO_POINTS).sum() >= 8 and got["status"][2] == vref.NO_POINTS      # (map 2: the empty frame alone)
    return got


@pytest.mark.parametrize("form", ["reverse", "overwritten", "forgotten", "grown"])
def test_arrival_order_does_not_show(manager, scene, want, form):
    h = manager.STDescManager()
    seen = []
    with se.init_points(64) if form == "grown" else contextlib.nullcontext():
        se._arrive(h, scene, form, seen)
    info = h.frame_clouds_info()
    assert info["n_frames"] == len(scene["final"]) and info["n_points"] == sum(len(c) for c in scene["final"].values())
    if form == "grown":
        steps = np.diff(seen)
        assert (steps > 0).any() and (steps < 0).any(), "the arena neither grew nor was compacted: %r" % seen
    vx.compare(_run(h, scene), want, form)
    h.close()


def test_a_growth_and_a_compaction_between_two_calls(manager, scene, want):
    h = manager.STDescManager()
    final, spare = scene["final"], scene["spare"]
    seen = []

    def note():
        seen.append(h.frame_clouds_info()["device_bytes"])

    with se.init_points(64):
        sx.store(h, final, k_neighbors=8)
    note()
    vx.compare(_run(h, scene), want, "before")
    note()      # (the call's own tail may have made the arena grow)
    h.set_frame_clouds([8, 9], [spare[0], spare[3]], k_neighbors=8)
    note()
    h.set_frame_clouds([8, 9, 40], [spare[3], spare[0], spare[4]], k_neighbors=8)      # dead slots between the members and behind them
    note()
    vx.compare(_run(h, scene), want, "dead slots")
    h.set_frame_clouds([8, 9, 40], None)
    h.set_frame_clouds([41], [spare[1]], k_neighbors=8)      # the dead points outnumber the live ones: a compaction
    note()
    steps = np.diff(seen)
    print("device_bytes:", seen)
    assert (steps > 0).any() and (steps < 0).any(), "the arena neither grew nor was compacted: %r" % seen
    vx.compare(_run(h, scene), want, "after the compaction")
    h.close()


@pytest.mark.parametrize("store_stride,store_dev", [(3, True), (4, False), (4, True)])
def test_strides_and_device_points(manager, scene, want, store_stride, store_dev):
    """stride 4 whose fourth float is 1e30, for the store, for the call, and mixed; points from the host and on the device"""
    h = manager.STDescManager()
    sx.store(h, scene["final"], stride=store_stride, dev=store_dev, k_neighbors=8)
    for stride, dev in ((3, False), (3, True), (4, False), (4, True)):
        vx.compare(_run(h, scene, dev=dev, stride=stride), want, "store %d %s, call %d %s" % (store_stride, store_dev, stride, dev))
    h.close()


def test_sizes_at_the_tile_edges(manager):
    """sources of 127, 128, 129 points (SGTD_REG_SRC_TILE), stored members of 511, 512, 513 (SGTD_REG_TGT_TILE, the set call's
    covariances), a one-point source and fewer points than k on the stored side"""
    s, t, R, tm = rx.surfaces(513, 1200, 5)
    rng = np.random.default_rng(3)
    sizes = [511, 512, 513, 5]
    stored = {10 + k: t[rng.permutation(len(t))[:n]] for k, n in enumerate(sizes)}
    calls = [s[:127], s[:128], s[:129], s[:1]]
    members = [[10], [11], [12], [13], [12, 10, 11]]
    map_off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
    map_frame = np.array([f for m in members for f in m], np.uint32)
    src = [a for a in range(len(calls)) for _ in members]
    tgt = [m for _ in calls for m in range(len(members))]
    h = manager.STDescManager()
    sx.store(h, stored, k_neighbors=8)
    got, _ = svx.check(h, calls, stored, map_off, map_frame, None, src, tgt, np.array([ref.near_start(R, tm)] * len(src)), "sizes", **OPT)
    assert [len(m) for m in got["matches"][::len(members)]] == [7 * 127, 7 * 128, 7 * 129, 7]
    assert [int(m["n_points"].sum()) for m in got["maps"]] == [511, 512, 513, 5, 1536]
    print("sizes: status", got["status"].tolist(), "iterations", got["iterations"].tolist())
    assert (got["status"] == vref.CONVERGED).any(), "no pair converges"
    h.close()


def test_a_voxel_across_two_stored_members(manager):
    """one voxel collects 63, 64 and 65 points (SGTD_VREG_SUM_W) from two stored members: its sums run over the first
    member's points and then the second's, each in point order, whatever the arrival order of the frames"""
    rng = np.random.default_rng(12)
    cell = lambda n: 0.5 + rng.uniform(0.05, 0.95, (n, 3))      # noqa: E731  (the voxel q = (0, 0, 0))
    bulk = lambda n: rng.uniform(3.0, 8.0, (n, 3))              # noqa: E731
    mix = lambda a, b: np.concatenate([a, b])[rng.permutation(len(a) + len(b))].astype(np.float32)      # noqa: E731
    stored = {7: mix(cell(40), bulk(60)), 3: mix(cell(23), bulk(30)), 9: mix(cell(24), bulk(30)), 5: mix(cell(25), bulk(30))}
    src = (np.concatenate([stored[7], stored[9]]).astype(np.float64) + rng.normal(0, 0.01, (154, 3))).astype(np.float32)
    map_off, map_frame = [0, 2, 4, 6, 8], [7, 3, 7, 9, 7, 5, 5, 7]
    h = manager.STDescManager()
    sx.store(h, stored, k_neighbors=6)
    got, _ = svx.check(h, [src], stored, map_off, map_frame, None, [0, 0, 0, 0], [0, 1, 2, 3], None, "a voxel across two members", k_neighbors=6,
                       max_iterations=30)
    assert [int(m["n_points"].max()) for m in got["maps"]] == [63, 64, 65, 65]
    print("a voxel across two members: status", got["status"].tolist(), "iterations", got["iterations"].tolist())
    assert (got["status"] == vref.CONVERGED).any(), "no pair converges"
    # members 5, 7 against 7, 5: the same voxels and counts, the sums in the other order
    a, b = got["maps"][2], got["maps"][3]
    assert np.array_equal(a["coord"], b["coord"]) and np.array_equal(a["n_points"], b["n_points"])
    assert np.allclose(a["mean"], b["mean"], rtol=0, atol=1e-12)
    h.close()


def test_points_that_enter_no_voxel(manager):
    """a coordinate whose q is out of range and non-finite coordinates, on the stored side and on the call's"""
    s, t, R, tm = rx.surfaces(200, 400, 5)
    far = np.float32((32768 + 0.5) * 1.0)
    member, source = t.copy(), s.copy()
    member[5, 0], member[6, 1], member[7, 2], member[8] = far, -far * 2, np.inf, np.nan
    source[3, 2], source[4, 0], source[9, 1] = far, np.nan, -np.inf
    h = manager.STDescManager()
    sx.store(h, {2: member}, k_neighbors=8)
    got, _ = svx.check(h, [source], {2: member}, [0, 1], [2], None, [0], [0], ref.near_start(R, tm)[None], "no voxel", **OPT)
    assert got["maps"][0]["n_points"].sum() == len(member) - 4
    rows = got["matches"][0].reshape(-1, 7)
    assert (rows[[3, 4, 9]] == -1).all() and (rows >= 0).any()
    print("no voxel: status", got["status"].tolist(), "iterations", got["iterations"].tolist())
    assert got["status"].tolist() == [vref.CONVERGED], "the pair does not converge"
    h.close()
