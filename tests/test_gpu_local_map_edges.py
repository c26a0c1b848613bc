"""sgtd_local_map_keypoints on the worlds of tests/_local_map_edges.py in every form of the call, against the restatement
(tests/_local_map_ref.py) exactly as tests/test_gpu_local_map.py compares: offsets, labels, counts, member lists, merged
sizes and pass counts as integers, centres bit for bit.  What each world reaches is shown on the CPU in
tests/test_local_map_edges.py."""
import ctypes as C

import numpy as np
import pytest

import _local_map_edges as le
import _local_map_ref as ref

pytestmark = pytest.mark.gpu

FORMS = ("host-3", "host-4", "device-3", "device-4", "device-4-misaligned")


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, manager, synth
    return manager, synth, _lib


@pytest.fixture(scope="module")
def g(mods):
    h = mods[0].STDescManager()
    yield h
    h.close()


def call(h, form, p, l, off, poses, cfg, **kw):
    """one call on handle h in one of FORMS; p is (n, 3) or (n, 4)"""
    stride = int(form.split("-")[1])
    p = le.with_stride(p, stride)
    if form.startswith("host"):
        return h.local_map_keypoints(p, l, off, poses, config=le.lib_cfg(cfg), **kw)
    import torch
    dl = torch.from_numpy(l.view(np.int32)).cuda()
    if form.endswith("misaligned"):
        # a view one float into a flat tensor: contiguous, 4 bytes past a 16-byte boundary — the only way to
        # lm_gather_kernel<4, false>
        n = len(p)
        flat = torch.zeros(4 * n + 4, dtype=torch.float32, device="cuda")
        dp = flat[1:1 + 4 * n].view(n, 4)
        dp.copy_(torch.from_numpy(p))
        assert dp.is_contiguous() and dp.data_ptr() % 16 == 4
    else:
        dp = torch.from_numpy(p).cuda()
        assert dp.data_ptr() % 16 == 0
    return h.local_map_keypoints(dp, dl, off, poses, config=le.lib_cfg(cfg), **kw)


def world_run(h, name, form="host-4", **more):
    w = le.world(name)
    got = call(h, form, w["p"], w["l"], w["off"], w["poses"], w["cfg"], **w["kw"], **more)
    le.same_as(h, got, le.expected(name), more.get("max_pass_points", 0))
    return got


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["lattice-600", "rotated-600", "full-lds"])
def test_worlds_in_every_form(g, name, form):
    world_run(g, name, form)


@pytest.mark.parametrize("form", ["host-4", "device-4-misaligned"])
def test_tile_edge_counts(g, mods, form):
    """test_gpu_local_map.py's test_member_sizes_at_the_tile_edges, also through the gather for misaligned points"""
    t = C.c_int(0)
    mods[2].lib().sgtd_scan_tiles(C.byref(t))
    tile = t.value
    counts = [tile - 1, 1, tile + 1, 0, 2 * tile]
    p, l, off = mods[1].make_scans(5, counts, stream=8, n_blobs=12)
    poses, cfg = ref.path_poses(5), ref.small_cfg()
    want = le.restate(p, l, off, poses, cfg, radius=100.0)
    assert want["merged_points"].tolist() == [sum(counts)] * 5 and np.all(np.diff(want["mem_off"]) == 5)
    le.same_as(g, call(g, form, p, l, off, poses, cfg, radius=100.0), want)


@pytest.mark.parametrize("cut", le.CUTS)
def test_lattice_600_cut(g, cut):
    name = "lattice-600-cut-%d" % cut
    whole = world_run(g, name)
    # one anchor per pass where the sizes allow no more: the same bits as the single pass
    largest = int(le.expected(name)["merged_points"].max())
    assert ref.plan_passes(le.expected(name)["merged_points"], largest) > 1
    passes = world_run(g, name, max_pass_points=largest)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(whole, passes))
    world_run(g, name, "device-3", max_pass_points=largest)


def test_lattice_600_one_anchor_per_pass(g):
    want = le.expected("lattice-600")
    largest = int(want["merged_points"].max())
    assert ref.plan_passes(want["merged_points"], largest) == len(want["merged_points"])
    world_run(g, "lattice-600", max_pass_points=largest)


def test_anchors_4097(mods):
    """4097 anchors: two passes, the first of SGTD_SCAN_MAX_SCANS anchors — scan_device with S = 4096, key_bits(S) = 13,
    the largest drop key, 1 GiB of ring bounds — the second of one.  A handle of its own, closed at once."""
    h = mods[0].STDescManager()
    try:
        world_run(h, "anchors-4097")
        assert h.local_map_members()[3] == 2
    finally:
        h.close()


def test_too_many_scans_is_refused_and_the_results_stay(mods):
    h = mods[0].STDescManager()
    first = world_run(h, "rotated-600")
    p, l, off, poses = le.too_many_scans()
    with pytest.raises(mods[2].SgtdError) as err:
        h.local_map_keypoints(le.with_stride(p, 4), l, off, poses, radius=1.0, config=le.lib_cfg(le.inst_cfg()))
    assert err.value.status == le.UNSUPPORTED and str(le.MAX_SCANS) in str(err.value)
    kept = h.local_map_results()
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(first, kept))
    le.same_as(h, kept, le.expected("rotated-600"))
    h.close()


def test_view_and_shards(mods):
    manager = mods[0]
    single, multi, view = manager.STDescManager(), manager.STDescManager(devices=[0, 0, 0]), manager.STDescManager()
    view.attach_table(single)
    for name in ("lattice-600-cut-17", "rotated-600"):
        want = world_run(single, name)
        for h in (multi, view):
            got = world_run(h, name)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(want, got))
            assert all(np.array_equal(a, b) for a, b in zip(h.local_map_members()[:3], single.local_map_members()[:3]))
    view.close()
    multi.close()
    single.close()
