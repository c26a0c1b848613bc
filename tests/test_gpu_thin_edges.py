"""sgtd_thin_clouds on the device at its structural edges (tests/_thin_edges.py: point counts around the sort's waves,
rounds and tiles and the scans' blocks, every digit of both sorts, 255 .. 65536 clouds, runs of empty clouds, clouds that
meet at a tile boundary, dropped points everywhere, a cell longer than three tiles whose fourth column tells the order of
its sum, and 2^22 points for the second level of the scans): every case bit for bit against tests/_thin_ref.py as
test_gpu_thin.py compares — the points as u32, out_off, n_dropped — with nothing written behind the last output row, and
a named subset in every other form of the call: from a device array, on a view, on a two-shard handle, timed, and on a
handle with a stream of its own."""
import ctypes as C

import numpy as np
import pytest

import _thin_edges as te

pytestmark = pytest.mark.gpu

SENT = np.float32(-7.25)
NAMES = list(te.cases())
FORMS = ("device", "view", "multi", "timed", "stream")


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, manager, synth
    return manager, synth, _lib


@pytest.fixture(scope="module")
def h(mods):
    m = mods[0].STDescManager()
    yield m
    m.close()


def _same(got, want, what):
    assert np.array_equal(got["pt_off"], want["pt_off"]), (what, got["pt_off"], want["pt_off"])
    assert np.array_equal(got["n_dropped"], want["n_dropped"]), (what, got["n_dropped"], want["n_dropped"])
    assert got["points"].shape == want["points"].shape and np.array_equal(te.bits(got["points"]), te.bits(want["points"])), what


def _nothing_behind(g, want, what):
    """the output fetched once more into K + 8 rows of a sentinel: the K rows, and nothing behind them"""
    K, stride = want["points"].shape
    buf = np.full((K + 8, stride), SENT, np.float32)
    n = C.c_int64(-1)
    assert g._L.sgtd_result_thinned(g._h, None, buf.ctypes.data_as(C.c_void_p), None, K + 8, C.byref(n)) == 0 and n.value == K, what
    assert np.array_equal(te.bits(buf[:K]), te.bits(want["points"])), what
    assert np.array_equal(te.bits(buf[K:]), te.bits(np.full((8, stride), SENT, np.float32))), what


def _check(g, arg, off, leaf, want, what):
    got = g.thin_clouds(arg, off, leaf)
    _same(got, want, what)
    _nothing_behind(g, want, what)
    return got


# ---- 1. every case from a host array on a plain handle ----
@pytest.mark.parametrize("name", NAMES)
def test_case_from_a_host_array(h, name):
    c = te.cases()[name]
    pts, off, leaf, _ = c.input()
    _check(h, pts, off, leaf, c.want(), name)


# ---- 2. the named subset in every other form ----
@pytest.fixture(scope="module")
def forms(mods):
    import torch
    manager, synth, _ = mods
    owner, view, multi, timed, streamed = (manager.STDescManager(), manager.STDescManager(), manager.STDescManager(devices=[0, 0]),
                                           manager.STDescManager(), manager.STDescManager())
    view.attach_table(owner)
    m = synth.make_map(12, 80, stream=5)
    owner.add_frames(m.xyz, m.label)      # (the owner's table holds frames and is not finalized)
    timed.set_timing(True)
    stream = torch.cuda.Stream()
    streamed.set_stream(stream.cuda_stream)
    yield {"device": owner, "view": view, "multi": multi, "timed": timed, "stream": streamed, "_stream": stream}
    for g in (view, multi, timed, streamed, owner):
        g.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", te.EVERY_FORM)
def test_case_in_every_other_form(forms, name, form):
    import torch
    c = te.cases()[name]
    pts, off, leaf, _ = c.input()
    g, arg = forms[form], pts
    if form == "device":
        arg = torch.from_numpy(np.array(pts)).cuda()
    elif form == "stream":
        # the device input is written on the handle's stream right before the call; the result is read when the call returns
        host = torch.from_numpy(np.array(pts)).pin_memory()
        with torch.cuda.stream(forms["_stream"]):
            arg = torch.empty(host.shape, dtype=torch.float32, device="cuda")
            arg.copy_(host, non_blocking=True)
    _check(g, arg, off, leaf, c.want(), (name, form))
    if form == "timed":
        ms = g.thin_stage_ms()
        assert ms[0] > 0.0 and ms[2] >= ms[0]
    if form == "stream":
        torch.cuda.synchronize()


# ---- 3. one handle, call after call ----
def test_a_sequence_on_one_handle(mods):
    g = mods[0].STDescManager()
    for k, (name, stride) in enumerate(te.SEQUENCE):
        if name is None:
            got = g.thin_clouds(np.zeros((0, stride), np.float32), [0], 0.25)
            assert got["points"].shape == (0, stride) and got["pt_off"].tolist() == [0] and got["n_dropped"].shape == (0, 2)
            _nothing_behind(g, got, (k, "an empty batch"))
            continue
        c = te.cases()[name]
        pts, off, leaf, st = c.input()
        assert st == stride
        _check(g, pts, off, leaf, c.want(), (k, name))
    g.close()


# ---- 4. a batch is its clouds one by one ----
@pytest.mark.parametrize("name", ["boundary-4096", "boundary-2048", "clouds-257"])
def test_each_cloud_alone_is_its_slice_of_the_batch(h, name):
    c = te.cases()[name]
    pts, off, leaf, _ = c.input()
    want = c.want()
    sizes = np.diff(off)
    some_empty = np.flatnonzero(sizes == 0)[:1].tolist()
    for s in np.flatnonzero(sizes).tolist() + some_empty:
        one = h.thin_clouds(pts[off[s]:off[s + 1]], None, leaf)
        a, b = want["pt_off"][s], want["pt_off"][s + 1]
        assert one["pt_off"].tolist() == [0, b - a] and np.array_equal(one["n_dropped"][0], want["n_dropped"][s]), (name, s)
        assert np.array_equal(te.bits(one["points"]), te.bits(want["points"][a:b])), (name, s)
    if name.startswith("boundary"):
        assert 0 < want["pt_off"][1] < want["pt_off"][2]


@pytest.mark.parametrize("name", ["boundary-4096", "boundary-2048"])
def test_set_frame_scans_stores_the_two_slices(mods, name):
    c = te.cases()[name]
    pts, off, leaf, _ = c.input()
    want = c.want()
    g = mods[0].STDescManager()
    out_off = g.set_frame_scans([5, 9], (pts, off), leaf, k_neighbors=10)
    assert np.array_equal(out_off, want["pt_off"])
    for s, f in enumerate((5, 9)):
        xyz = g.frame_cloud(f)[0]
        a, b = want["pt_off"][s], want["pt_off"][s + 1]
        assert xyz.shape == (b - a, 3) and np.array_equal(te.bits(xyz), te.bits(want["points"][a:b])), (name, f)
    assert g.frame_clouds_info()["n_points"] == int(want["pt_off"][2])
    g.close()


# ---- 5. deep: the scans' second level, grids of 16 384 workgroups ----
@pytest.mark.parametrize("P", te.DEEP_P)
def test_deep_against_the_closed_form(mods, P):
    assert te.deep_reaches(P)
    (pts, off, leaf, _), want = te.deep(P)
    g = mods[0].STDescManager()
    try:
        _check(g, pts, off, leaf, want, "deep %d" % P)
    finally:
        g.close()
