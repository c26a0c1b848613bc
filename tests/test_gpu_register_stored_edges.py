"""The cloud store at its edges: its history must not show.  The same frames and clouds arrive in one call, a frame a call,
with overwrites, with frames stored and forgotten in between, and from a first capacity of 64 points (growth and
compaction): every form gives the same stored clouds and the same registration bits.  Cloud sizes at the kernels' tile
edges, strides, the settings' and the failed calls' rules, forget-all."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import _register_edges as rx
import _register_ref as ref
import _stored_edges as sx

pytestmark = pytest.mark.gpu

OPT = dict(k_neighbors=8, max_corr_dist=2.0, max_iterations=3)


@pytest.fixture(scope="module")
def manager():
    from sgtd_amd import manager
    return manager


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@contextlib.contextmanager
def init_points(n):
    """sets the SGTD_CLOUD_STORE_INIT_POINTS hook (read at a store's first set call) and puts back what was there"""
    old = os.environ.get("SGTD_CLOUD_STORE_INIT_POINTS")
    os.environ["SGTD_CLOUD_STORE_INIT_POINTS"] = str(n)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("SGTD_CLOUD_STORE_INIT_POINTS", None)
        else:
            os.environ["SGTD_CLOUD_STORE_INIT_POINTS"] = old


@pytest.fixture(scope="module")
def scene():
    """the frames' final clouds, the call's clouds and pairs, clouds to overwrite with, and what one set call gives:
    every frame's stored cloud and the registration's bits, checked against sgtd_register_clouds and the restatement"""
    s, t, R, tm = rx.surfaces(300, 1200, 5)
    rng = np.random.default_rng(8)
    cut = lambda n: t[rng.permutation(len(t))[:n]].copy()      # noqa: E731
    final = {1: cut(127), 4: cut(0), 6: cut(300), 30: cut(129), 31: cut(64)}
    calls = [s[:150], s[150:278]]
    src = [a for a in range(2) for _ in final]
    tgt = [f for _ in range(2) for f in final]
    init = np.array([ref.near_start(R, tm)] * len(src))
    return dict(final=final, calls=calls, src=src, tgt=tgt, init=init, spare=[cut(400), cut(50), cut(0), cut(310), cut(290)])


@pytest.fixture(scope="module")
def want(manager, scene):
    h = manager.STDescManager()
    sx.store(h, scene["final"], k_neighbors=8)
    got, direct = sx.check(h, scene["calls"], scene["final"], scene["src"], scene["tgt"], scene["init"], "one call", **OPT)
    got["clouds"] = {f: h.frame_cloud(f) for f in scene["final"]}
    frames = sorted(scene["final"])
    for f, (xyz, cov) in got["clouds"].items():
        assert ref.same(xyz, scene["final"][f]) and ref.same(cov, direct["cov"][2 + frames.index(f)])
    h.close()
    return got


def _arrive(h, scene, form, seen):
    """the store's history in one of its forms; seen: device_bytes after every step"""
    final, spare = scene["final"], scene["spare"]

    def put(frames, clouds):
        h.set_frame_clouds(frames, clouds, k_neighbors=8)
        seen.append(h.frame_clouds_info()["device_bytes"])

    def forget(frames):
        h.set_frame_clouds(frames, None)
        seen.append(h.frame_clouds_info()["device_bytes"])

    if form == "reverse":
        for f in sorted(final, reverse=True):
            put([f], [final[f]])
    elif form == "overwritten":
        put(list(final), [final[f] if f != 6 else spare[4] for f in final])
        for c in spare[:3]:
            put([6], [c])                      # larger, smaller, empty
        put([6, 6], [spare[3], final[6]])      # twice in one call: the last one wins
    elif form == "forgotten":
        put([8, 1, 9], [spare[0], final[1], spare[1]])
        put([4, 6], [spare[2], final[6]])
        forget([8, 4, 77])
        put([4, 30, 31], [final[4], final[30], final[31]])
        forget([9])
    elif form == "grown":
        # from 64 points: growth at the first calls, dead points that outnumber the live ones on the way
        put([6], [spare[0]])
        put([1, 6], [final[1], spare[3]])
        put([8, 9], [spare[4], spare[0]])
        put([6, 30], [final[6], final[30]])
        forget([8, 9])
        put([4, 31], [final[4], final[31]])
    else:
        raise ValueError(form)


@pytest.mark.parametrize("form", ["reverse", "overwritten", "forgotten", "grown"])
def test_arrival_order_does_not_show(manager, scene, want, form):
    h = manager.STDescManager()
    seen = []
    with init_points(64) if form == "grown" else contextlib.nullcontext():
        _arrive(h, scene, form, seen)
    info = h.frame_clouds_info()
    assert info["n_frames"] == len(scene["final"]) and info["n_points"] == sum(len(c) for c in scene["final"].values())
    print(form, "device_bytes after every step:", seen)
    if form == "grown":
        steps = np.diff(seen)
        assert (steps > 0).any() and (steps < 0).any(), "the arena neither grew nor was compacted: %r" % seen
        assert seen[0] < 2 * 64 * 84 + 400 * 84 * 2
    for f, (xyz, cov) in want["clouds"].items():
        sx.same_cloud(h, f, xyz, cov)
    assert h.frame_cloud(8) is None and h.frame_cloud(9) is None and h.frame_cloud(77) is None
    got = sx.run(h, scene["calls"], scene["src"], scene["tgt"], scene["init"], **OPT)
    sx.compare(got, want, scene["src"], form)
    h.close()


def test_sizes_at_the_tile_edges(manager):
    """127, 128, 129 points (the source tile), 511, 512, 513 (the target tile) and fewer points than k, on both sides"""
    s, t, R, tm = rx.surfaces(513, 1200, 5)
    rng = np.random.default_rng(3)
    sizes = [127, 128, 129, 511, 512, 513, 5]
    stored = {10 + k: t[rng.permutation(len(t))[:n]] for k, n in enumerate(sizes)}
    calls = [s[:127], s[:128], s[:129], s[:513], s[:5]]
    src = [a for a in range(len(calls)) for _ in stored]
    tgt = [f for _ in calls for f in stored]
    h = manager.STDescManager()
    sx.store(h, stored, k_neighbors=8)
    sx.check(h, calls, stored, src, tgt, np.array([ref.near_start(R, tm)] * len(src)), "sizes", **OPT)
    h.close()


@pytest.mark.parametrize("store_stride,store_dev", [(3, True), (4, False), (4, True)])
def test_strides_and_device_points(manager, scene, want, store_stride, store_dev):
    """stride 4 whose fourth float is 1e30, for the store, for the call, and mixed; points from the host and on the device"""
    h = manager.STDescManager()
    sx.store(h, scene["final"], stride=store_stride, dev=store_dev, k_neighbors=8)
    for f, (xyz, cov) in want["clouds"].items():
        sx.same_cloud(h, f, xyz, cov)
    for stride, dev in ((3, False), (3, True), (4, False), (4, True)):
        got = sx.run(h, scene["calls"], scene["src"], scene["tgt"], scene["init"], dev=dev, stride=stride, **OPT)
        sx.compare(got, want, scene["src"], "store %d %s, call %d %s" % (store_stride, store_dev, stride, dev))
    h.close()


def test_settings_failed_calls_and_forget_all(manager, scene, want):
    h = manager.STDescManager()
    L = h._L
    final = scene["final"]
    sx.store(h, final, k_neighbors=8)
    first = sx.run(h, scene["calls"], scene["src"], scene["tgt"], scene["init"], **OPT)
    sx.compare(first, want, scene["src"], "before the failed calls")

    def intact():
        info = h.frame_clouds_info()
        assert (info["n_frames"], info["k_neighbors"], info["plane_eps"]) == (len(final), 8, 1e-3)
        for f, (xyz, cov) in want["clouds"].items():
            sx.same_cloud(h, f, xyz, cov)
        sx.compare(sx.getters(h, h.result_stored_registered(), 2), want, scene["src"], "after a failed call")

    # other settings: SGTD_ERR_STATE, for the store and for the calls
    for kw in (dict(k_neighbors=9), dict(k_neighbors=8, plane_eps=2e-3)):
        with pytest.raises(manager.SgtdError) as err:
            h.set_frame_clouds([40], [final[1]], **kw)
        assert err.value.status == -7
        o = dict(OPT)
        o.update(kw)
        with pytest.raises(manager.SgtdError) as err:
            sx.run(h, scene["calls"], scene["src"], scene["tgt"], scene["init"], **o)
        assert err.value.status == -7
    # a pair that names a frame without a cloud: SGTD_ERR_INVALID, and the handle says which
    with pytest.raises(manager.SgtdError) as err:
        sx.run(h, scene["calls"], [0, 1], [6, 40], None, **OPT)
    assert err.value.status == -1 and "frame 40" in str(err.value)
    # the caps, from the offsets alone (the checks come before every read): a cloud, and the store's live points
    pts = np.zeros((4, 3), np.float32)
    ids = np.arange(1025, dtype=np.uint32)
    big = np.array([0, (1 << 17) + 1], np.int64)
    assert L.sgtd_set_frame_clouds(h._h, _ptr(ids), _ptr(big), _ptr(pts), 3, 1, 8, 1e-3, 0) == -6 and b"points a cloud" in L.sgtd_last_error(h._h)
    full = (np.arange(1026, dtype=np.int64) << 17)
    assert L.sgtd_set_frame_clouds(h._h, _ptr(ids), _ptr(full), _ptr(pts), 3, 1025, 8, 1e-3, 0) == -6 and b"live points" in L.sgtd_last_error(h._h)
    src, tgt = np.array([0], np.int32), np.array([6], np.uint32)
    assert L.sgtd_register_stored(h._h, None, _ptr(pts), 3, _ptr(big), 1, _ptr(src), _ptr(tgt), None, 1, 0) == -6
    assert L.sgtd_set_frame_clouds(h._h, _ptr(np.array([20000], np.uint32)), _ptr(big), _ptr(pts), 3, 1, 8, 1e-3, 0) == -5
    intact()
    # forget all: no frames, no device memory, no settings; a store with other values works
    h.set_frame_clouds(None, None)
    info = h.frame_clouds_info()
    assert (info["n_frames"], info["n_points"], info["device_bytes"], info["k_neighbors"], info["plane_eps"]) == (0, 0, 0, 0, 0.0)
    assert h.frame_cloud(6) is None
    h.set_frame_clouds([6, 1], [final[6], final[1]], k_neighbors=9, plane_eps=2e-3)
    o = dict(OPT, k_neighbors=9, plane_eps=2e-3)
    sx.check(h, scene["calls"], final, [0, 1], [6, 1], scene["init"][:2], "new settings", **o)
    h.close()
