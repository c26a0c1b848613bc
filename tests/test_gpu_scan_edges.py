"""sgtd_scan_keypoints on the worlds of tests/_scan_edges.py in every form of the call, against the restatement
(tests/_scan_ref.py) exactly as tests/test_gpu_scan.py compares: offsets, labels, counts, per-point cluster indices and
grids as integers, centres and minPolar / maxPolar bit for bit, the two pitches to 1e-12 degrees.  What each world reaches
is shown on the CPU in tests/test_scan_edges.py.  The device's number of hook + jump rounds is not asserted: it reads its
neighbours' parents live and may need fewer than the synchronous model."""
import numpy as np
import pytest

import _scan_edges as se

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, manager
    return manager, _lib


@pytest.fixture(scope="module")
def g(mods):
    h = mods[0].STDescManager()
    yield h
    h.close()


def world_run(h, name, stride=4, dev=False):
    p, l, off, cfg = se.world(name)
    got = se.run(h, se.with_stride(p, stride), l, off, cfg, dev)
    se.same_as(h, got, se.expected(name))
    return got


@pytest.mark.parametrize("name", list(se.WORLDS))
def test_worlds_from_host_arrays(g, name):
    world_run(g, name)


@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("name", se.FIVE)
def test_five_from_device_tensors(g, name, stride):
    world_run(g, name, stride, dev=True)


def test_five_from_host_arrays_at_stride_3(g):
    for name in se.FIVE:
        world_run(g, name, 3)


@pytest.mark.parametrize("form", ["host-4", "device-3", "device-4"])
def test_five_in_one_batch(g, form):
    p, l, off, cfg = se.concatenated()
    got = se.run(g, se.with_stride(p, int(form[-1])), l, off, cfg, dev=form.startswith("device"))
    se.same_as(g, got, se.expected_concatenated())


def same_bits(a, b):
    return all(np.array_equal(se.bits(x) if x.dtype.kind == "f" else x, se.bits(y) if y.dtype.kind == "f" else y) for x, y in zip(a, b))


def test_view_and_shards(mods):
    manager = mods[0]
    single, multi, view = manager.STDescManager(), manager.STDescManager(devices=[0, 0, 0]), manager.STDescManager()
    view.attach_table(single)
    batches = [se.world(k) for k in se.FIVE] + [se.concatenated()]
    wants = [se.expected(k) for k in se.FIVE] + [se.expected_concatenated()]
    for (p, l, off, cfg), want in zip(batches, wants):
        p4 = se.with_stride(p, 4)
        first = se.run(single, p4, l, off, cfg)
        se.same_as(single, first, want)
        for h in (multi, view):
            got = se.run(h, p4, l, off, cfg)
            assert same_bits(first, got)
            for s in range(0, len(off) - 1, 7):
                assert np.array_equal(h.scan_point_clusters(s), single.scan_point_clusters(s))
                assert all(np.array_equal(se.bits(x) if x.dtype.kind == "f" else x, se.bits(y) if y.dtype.kind == "f" else y)
                           for x, y in zip(h.scan_grids(s), single.scan_grids(s)))
    view.close()
    multi.close()
    single.close()


@pytest.mark.parametrize("order", [("all-dropped", "big-4096", "all-dropped"), ("big-4096", "all-dropped", "big-4096")])
def test_calls_in_turn_on_one_handle_equal_a_fresh_handle(mods, order):
    """buffers sized by an earlier call, and the number of keypoints going 0 -> K -> 0 and K -> 0 -> K"""
    used = mods[0].STDescManager()
    for name in order:
        fresh = mods[0].STDescManager()
        a, b = world_run(used, name), world_run(fresh, name)
        assert same_bits(a, b)
        n = len(se.world(name)[2]) - 1
        assert all(np.array_equal(used.scan_point_clusters(s), fresh.scan_point_clusters(s)) for s in range(n))
        fresh.close()
    used.close()


def test_too_many_scans_is_refused_and_the_results_stay(mods):
    h = mods[0].STDescManager()
    first = world_run(h, "one-live")
    p, l, off = se.too_many_scans()
    with pytest.raises(mods[1].SgtdError) as err:
        h.scan_keypoints(se.with_stride(p, 4), l, off)
    assert err.value.status == se.UNSUPPORTED and str(se.MAX_SCANS) in str(err.value)
    assert same_bits(h.scan_results(), first)
    se.same_as(h, first, se.expected("one-live"))
    h.close()
