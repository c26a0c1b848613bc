"""Voxel-grid thinning on the device (sgtd_thin_clouds): every case bit for bit against the rule restated in
tests/_thin_ref.py — the points viewed as u32, out_off, n_dropped — at the rule's edges, for the output order, the
sequential sums, the tiling, the call's state, and for the device view fed to the cloud store and the registration calls."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import _thin_ref as tr

pytestmark = pytest.mark.gpu

INVALID, CAPACITY, UNSUPPORTED, STATE = -1, -4, -6, -7


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, ingest, manager, synth
    return manager, synth, _lib, ingest


@pytest.fixture(scope="module")
def h(mods):
    m = mods[0].STDescManager()
    yield m
    m.close()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pack(clouds, stride=3):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = np.concatenate([np.asarray(c, np.float32).reshape(-1, stride) for c in clouds]) if clouds else np.zeros((0, stride), np.float32)
    return np.ascontiguousarray(pts), off


def _same(got, want, what):
    assert np.array_equal(got["pt_off"], want["pt_off"]), (what, got["pt_off"], want["pt_off"])
    assert np.array_equal(got["n_dropped"], want["n_dropped"]), (what, got["n_dropped"], want["n_dropped"])
    assert got["points"].shape == want["points"].shape and np.array_equal(_bits(got["points"]), _bits(want["points"])), what


def _check(h, clouds, leaf, what, stride=3, device=False):
    """the call on these clouds against the restatement -> the call's results"""
    pts, off = _pack(clouds, stride)
    arg = pts
    if device:
        import torch
        arg = torch.from_numpy(pts).cuda()
    got = h.thin_clouds(arg, off, leaf)
    _same(got, tr.thin(pts, off, leaf), what)
    return got


# ---- 1. the edges of the rule ----
def test_empty_batch_and_empty_clouds(h):
    got = h.thin_clouds(np.zeros((0, 3), np.float32), [0], 0.25)
    assert got["points"].shape == (0, 3) and got["pt_off"].tolist() == [0] and got["n_dropped"].shape == (0, 2)
    view = h.thin_results(fetch=False)
    assert len(view["points"]) == 0 and view["pt_off"].tolist() == [0]
    rng = np.random.default_rng(1)
    a, b = rng.uniform(-3, 3, (40, 3)), rng.uniform(-3, 3, (55, 3))
    got = _check(h, [a, np.zeros((0, 3)), b], 0.5, "an empty cloud between two full ones")
    assert got["pt_off"][1] == got["pt_off"][2] and 0 < got["pt_off"][1] < got["pt_off"][3]
    got = _check(h, [np.zeros((0, 3)), np.zeros((0, 3))], 0.5, "empty clouds alone")
    assert got["pt_off"].tolist() == [0, 0, 0]
    got = _check(h, [[[1.5, -2.5, 0.25]]], 0.5, "a one-point cloud")
    assert np.array_equal(_bits(got["points"]), _bits(np.array([[1.5, -2.5, 0.25]], np.float32)))
    nan = np.full((70, 3), np.nan, np.float32)
    nan[::3, 1] = 1.0
    nan[5] = [np.inf, 0.0, 0.0]
    got = _check(h, [a, nan, [[0.0, 0.0, -np.inf]], b], 0.5, "clouds without a finite point")
    assert got["n_dropped"].tolist()[1:3] == [[70, 0], [1, 0]] and got["pt_off"][1] == got["pt_off"][3]


def test_cell_borders_and_the_sign_of_zero(h):
    leaf = 0.25
    k = np.arange(-6, 7, dtype=np.float32)
    on_faces = np.stack([k * np.float32(leaf), np.zeros(13, np.float32), np.zeros(13, np.float32)], 1)
    got = _check(h, [on_faces], leaf, "points at k * leaf")
    assert len(got["points"]) == 13                                   # one cell each
    zeros = np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [0.1, 0.1, 0.1]], np.float32)
    got = _check(h, [zeros], leaf, "-0.0 lies in cell 0")
    assert len(got["points"]) == 1
    sides = np.array([[-0.1, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, -0.1, 0.0], [0.0, 0.0, -0.1]], np.float32)
    got = _check(h, [sides], leaf, "floor, not truncation")
    assert len(got["points"]) == 4
    # a leaf that is no power of two: the division's rounding decides the cell of 0.3 / 0.1 and its like
    grid = (np.arange(-20, 21, dtype=np.float64) * 0.1).astype(np.float32)
    pts = np.stack([grid, grid[::-1], np.zeros(41, np.float32)], 1)
    _check(h, [pts], 0.1, "multiples of a leaf of 0.1")
    _check(h, [pts.astype(np.float64) * 3.0], 0.30000000000000004, "a leaf with a full f64 mantissa")


def test_the_cell_range(h):
    m = float(tr.MAX_CELL)
    pts = np.array([[m - 0.5, 0.0, 0.0],          # cell MAX - 1: kept
                    [m, 0.0, 0.0],                # cell MAX: out
                    [0.0, -m, 0.0],               # cell -MAX: kept
                    [0.0, -m - 1.0, 0.0],         # cell -MAX - 1: out
                    [0.0, 0.0, m - 0.5], [0.0, 0.0, m + 7.0], [3e6, 0.0, 0.0], [1e30, -1e30, 0.0],
                    [m - 0.5, m - 0.5, m - 0.5],  # the corner cell, whose key is all ones
                    [np.nan, m, 0.0],             # not finite comes first
                    [0.5, 0.5, 0.5]], np.float32)
    got = _check(h, [pts, pts[::-1]], 1.0, "the cell range")
    assert got["n_dropped"].tolist() == [[1, 5], [1, 5]] and got["pt_off"].tolist() == [0, 5, 10]
    # a tiny leaf: the division overflows to infinity, which is out of range
    got = _check(h, [[[1e30, 0.0, 0.0], [0.0, 0.0, 0.0], [1e-30, 0.0, 0.0]]], 1e-300, "a division that overflows")
    assert got["n_dropped"].tolist() == [[0, 2]]


def test_clouds_with_the_same_coordinates_do_not_merge(h):
    rng = np.random.default_rng(2)
    a = rng.uniform(-2, 2, (300, 3)).astype(np.float32)
    got = _check(h, [a, a, a[:1], a], 0.5, "the same cloud three times")
    o = got["pt_off"]
    n = o[1]
    assert o.tolist() == [0, n, 2 * n, 2 * n + 1, 3 * n + 1]
    assert np.array_equal(_bits(got["points"][:n]), _bits(got["points"][n:2 * n]))


# ---- 2. order ----
def test_cells_come_out_by_their_first_point(h):
    # the cells' first points arrive in descending cell order, then every cell is visited again in ascending order
    k = np.arange(40, dtype=np.float32)
    first = np.stack([39.0 - k, 39.0 - k, 39.0 - k], 1) + np.float32(0.25)
    again = np.stack([k, k, k], 1) + np.float32(0.75)
    cloud = np.concatenate([first, again]).astype(np.float32)
    got = _check(h, [cloud], 1.0, "descending cells")
    assert np.array_equal(got["points"][:, 0], (39.0 - k) + np.float32(0.5))      # by first index, not by key
    rng = np.random.default_rng(3)
    base = rng.uniform(-4, 4, (900, 4)).astype(np.float32)
    perm = rng.permutation(900)
    a = _check(h, [base], 0.5, "a cloud", stride=4)
    b = _check(h, [base[perm]], 0.5, "its permutation", stride=4)
    assert a["points"].shape == b["points"].shape and not np.array_equal(_bits(a["points"]), _bits(b["points"]))


# ---- 3. sums ----
def _one_cell_cloud(stride, n=3000):
    """n points of one cell (leaf 1e5) whose coordinates span 1e-3 .. 1e4, with the last three x values chosen so that the
    exact mean of x lies within a rounding error of the midpoint of two neighbouring f32 values: there the sequential f64
    sum and a pairwise (tree) sum round to different f32 means.  Returns the cloud; raises where no such tail is found."""
    rng = np.random.default_rng(77)
    p = np.exp(rng.uniform(np.log(1e-3), np.log(1e4), (n, stride))).astype(np.float32)
    head = sum(Fraction(float(v)) for v in p[:n - 3, 0])
    for trial in range(200):
        f = np.float32(float((head + 1000 + 37 * trial) / n))
        mid = Fraction(float(f)) + (Fraction(float(np.nextafter(f, np.float32(np.inf)))) - Fraction(float(f))) / 2
        rest = mid * n - head                                          # what the last three must add, exactly
        tail = []
        for step in (1.0, 2e-3, 0.0):
            v = np.float32(float(rest) - step)
            tail.append(v)
            rest -= Fraction(float(v))
        if not all(1e-3 <= float(v) <= 1e4 for v in tail):
            continue
        p[n - 3:, 0] = tail
        seq = tr.thin_cloud(p, 1e5)[0]
        if _bits(seq)[0, 0] != _bits(tr.pairwise_mean(p[:, 0].astype(np.float64), n)):
            return p
    raise AssertionError("no tail separates the sequential from the pairwise sum")


@pytest.mark.parametrize("stride", [3, 4])
def test_one_cell_holding_a_whole_cloud(h, stride):
    p = _one_cell_cloud(stride)
    assert p.min() >= 1e-3 and p.max() <= 1e4 and p.max() / p.min() > 1e6
    want = tr.thin_cloud(p, 1e5)[0]
    assert want.shape == (1, stride)
    tree = np.array([tr.pairwise_mean(p[:, a].astype(np.float64), len(p)) for a in range(stride)], np.float32)
    assert (_bits(tree) != _bits(want[0])).any(), "a pairwise sum gives the same bits: the case proves nothing"
    got = _check(h, [p], 1e5, "one cell, %d columns" % stride, stride=stride)
    assert np.array_equal(_bits(got["points"]), _bits(want))
    # the same cloud among others, and split over two cells
    rng = np.random.default_rng(4)
    _check(h, [rng.uniform(-1, 1, (100, stride)), p, rng.uniform(-1, 1, (1, stride))], 1e5, "the one-cell cloud in a batch", stride=stride)
    _check(h, [p], 50.0, "the same points in many cells", stride=stride)


# ---- 4. tiling ----
@pytest.mark.parametrize("device", [False, True])
def test_a_batch_is_its_clouds_one_by_one(h, device):
    rng = np.random.default_rng(8)
    sizes = (257, 1, 0, 1023, 4096)
    clouds = [rng.normal(0.0, 2.0, (n, 4)).astype(np.float32) for n in sizes]
    clouds[0][100, 2] = np.nan
    clouds[3][::97, 0] = 1e7
    batch = _check(h, clouds, 0.25, "the batch", stride=4, device=device)
    assert batch["n_dropped"].tolist() == [[1, 0], [0, 0], [0, 0], [0, 11], [0, 0]]
    for s, c in enumerate(clouds):
        one = _check(h, [c], 0.25, "cloud %d alone" % s, stride=4, device=device)
        a, b = batch["pt_off"][s], batch["pt_off"][s + 1]
        assert np.array_equal(_bits(one["points"]), _bits(batch["points"][a:b])) and np.array_equal(one["n_dropped"][0], batch["n_dropped"][s]), s
    # and in another order, with another leaf
    _check(h, clouds[::-1], 0.7, "the batch reversed", stride=4, device=device)


# ---- 5. state ----
def test_state_capacity_and_rejected_calls(mods):
    manager = mods[0]
    g = manager.STDescManager()
    L, hd = g._L, g._h
    n, stride = C.c_int64(-5), C.c_int(-5)
    ptr = C.c_void_p()
    ms = [C.c_float(-1.0) for _ in range(3)]
    # the getters before a run
    assert L.sgtd_result_thinned(hd, None, None, None, 0, C.byref(n)) == STATE and n.value == -5
    assert L.sgtd_thinned_device_view(hd, C.byref(ptr), C.byref(stride), C.byref(n)) == STATE and stride.value == -5
    assert L.sgtd_thin_stage_ms(hd, *[C.byref(v) for v in ms]) == STATE
    assert b"sgtd_thin_clouds" in L.sgtd_last_error(hd)
    rng = np.random.default_rng(9)
    a = rng.uniform(-3, 3, (500, 3)).astype(np.float32)
    off = np.array([0, 200, 500], np.int64)
    first = g.thin_clouds(a, off, 0.5)
    want = tr.thin(a, off, 0.5)
    _same(first, want, "the first call")
    k = len(want["points"])
    # a capacity one short: the size needed, the prefix written and nothing behind it
    buf = np.full((k, 3), 7.0, np.float32)
    assert L.sgtd_result_thinned(hd, None, _ptr(buf), None, k - 1, C.byref(n)) == CAPACITY and n.value == k
    assert np.array_equal(_bits(buf[:k - 1]), _bits(want["points"][:k - 1])) and np.all(buf[k - 1] == 7.0)
    assert L.sgtd_result_thinned(hd, None, None, None, 0, C.byref(n)) == 0 and n.value == k      # (no array: only the size)
    assert L.sgtd_result_thinned(hd, None, None, None, -1, C.byref(n)) == INVALID
    # rejected calls keep the results
    bad_off = np.array([0, 300, 200], np.int64)
    from_one = np.array([1, 200, 500], np.int64)
    for args in ((_ptr(a), 2, _ptr(off), 2, 0.5, 0), (_ptr(a), 5, _ptr(off), 2, 0.5, 0), (_ptr(a), 3, _ptr(bad_off), 2, 0.5, 0),
                 (_ptr(a), 3, _ptr(from_one), 2, 0.5, 0), (_ptr(a), 3, _ptr(off), -1, 0.5, 0), (None, 3, _ptr(off), 2, 0.5, 0),
                 (_ptr(a), 3, None, 2, 0.5, 0), (_ptr(a), 3, _ptr(off), 2, 0.0, 0), (_ptr(a), 3, _ptr(off), 2, -1.0, 0),
                 (_ptr(a), 3, _ptr(off), 2, float("nan"), 0), (_ptr(a), 3, _ptr(off), 2, float("inf"), 0)):
        assert L.sgtd_thin_clouds(hd, *args) == INVALID, args[1:]
    too_many = np.zeros((1 << 16) + 2, np.int64)
    assert L.sgtd_thin_clouds(hd, _ptr(a), 3, _ptr(too_many), (1 << 16) + 1, 0.5, 0) == UNSUPPORTED
    too_long = np.array([0, (1 << 28) + 1], np.int64)
    assert L.sgtd_thin_clouds(hd, _ptr(a), 3, _ptr(too_long), 1, 0.5, 0) == UNSUPPORTED
    _same(g.thin_results(), want, "after the rejected calls")
    # a second call replaces the first; the view names its output
    b = rng.uniform(-3, 3, (300, 4)).astype(np.float32)
    second = g.thin_clouds(b, None, 0.25)
    _same(second, tr.thin(b, [0, 300], 0.25), "the second call")
    assert L.sgtd_thinned_device_view(hd, C.byref(ptr), C.byref(stride), C.byref(n)) == 0
    assert ptr.value and stride.value == 4 and n.value == len(second["points"])
    # (S, N, 3) without offsets
    c = rng.uniform(-3, 3, (3, 100, 3)).astype(np.float32)
    _same(g.thin_clouds(c, leaf=0.5), tr.thin(c.reshape(-1, 3), [0, 100, 200, 300], 0.5), "(S, N, 3)")
    g.close()


def test_views_shards_and_stage_times(mods):
    manager, synth = mods[:2]
    rng = np.random.default_rng(10)
    a = rng.uniform(-3, 3, (700, 3)).astype(np.float32)
    off = np.array([0, 300, 700], np.int64)
    want = tr.thin(a, off, 0.5)
    owner, view, multi = manager.STDescManager(), manager.STDescManager(), manager.STDescManager(devices=[0, 0])
    view.attach_table(owner)                      # (the owner's table: not even finalized)
    n = C.c_int64(0)
    for g in (view, owner, multi):
        assert g._L.sgtd_result_thinned(g._h, None, None, None, 0, C.byref(n)) == STATE
        _same(g.thin_clouds(a, off, 0.5), want, "a view, its owner, a multi-device handle")
    # the call leaves a pending batch alone, and a batch leaves the thinned clouds alone
    m = synth.make_map(12, 80, stream=5)
    owner.add_frames(m.xyz, m.label)
    before = owner.query_frames(m.xyz[:3], m.label[:3])
    _same(owner.thin_results(), want, "after a batch")
    _same(view.thin_results(), want, "the view's own results")
    owner.thin_clouds(a[:10], None, 0.5)
    after = owner.results()
    assert np.array_equal(before.cand_frame, after.cand_frame) and np.array_equal(before.n_cand, after.n_cand)
    _same(view.thin_results(), want, "after the owner's next call")
    # times: zeros unless asked for; the same bits either way
    assert owner.thin_stage_ms() == (0.0, 0.0, 0.0)
    owner.set_timing(True)
    try:
        timed = owner.thin_clouds(a, off, 0.5)
        ms = owner.thin_stage_ms()
    finally:
        owner.set_timing(False)
    _same(timed, want, "timed")
    assert ms[0] > 0.0 and ms[1] > 0.0 and abs(ms[0] + ms[1] - ms[2]) <= 1e-3 * ms[2]
    view.close()
    multi.close()
    owner.close()


# ---- 6. the view feeds the stage ----
@pytest.fixture(scope="module")
def scene(mods):
    """test_gpu_register_stored.py's small verified batch, built here: 20 posed scans as the map (scan 3 twice), 3 of them
    jittered as the queries, and the host-thinned clouds of both"""
    manager, synth, _, ingest = mods
    cfg = {"min_seg": [20] * 32}
    p, l, off, _ = synth.make_posed_scans(20, 6000, stream=33, spacing=2.0, n_blobs=60, sensor_range=40.0, sigma=(0.05, 0.12))
    rng = np.random.default_rng(6)
    picks = [3, 9, 15]
    qp = np.concatenate([p[off[f]:off[f + 1]] for f in picks]).copy()
    qp[:, :3] += rng.normal(0.0, 0.01, (len(qp), 3)).astype(np.float32)
    ql = np.concatenate([l[off[f]:off[f + 1]] for f in picks])
    qo = np.arange(4, dtype=np.int64) * 6000
    frames = [f for f in range(20) if f not in (4, 10)]
    map_thin = {f: ingest.voxel_downsample(p[off[f]:off[f + 1], :3], 0.25) for f in frames}
    q_thin = [ingest.voxel_downsample(qp[qo[q]:qo[q + 1], :3], 0.25) for q in range(3)]
    return dict(cfg=cfg, p=p, l=l, off=off, qp=qp, ql=ql, qo=qo, frames=frames, map_thin=map_thin, q_thin=q_thin)


def _same_dict(got, want, what):
    assert set(got) == set(want), what
    for f in want:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, f)


def test_set_frame_scans_is_set_frame_clouds_of_the_thinned_clouds(mods, scene):
    manager = mods[0]
    a, b = manager.STDescManager(), manager.STDescManager()
    frames, p, off = scene["frames"], scene["p"], scene["off"]
    scans = [p[off[f]:off[f + 1], :3] for f in frames]
    out_off = a.set_frame_scans(frames, scans, 0.25, k_neighbors=10)
    b.set_frame_clouds(frames, [scene["map_thin"][f] for f in frames], k_neighbors=10)
    assert np.array_equal(np.diff(out_off), [len(scene["map_thin"][f]) for f in frames])
    ia, ib = a.frame_clouds_info(), b.frame_clouds_info()
    assert (ia["n_frames"], ia["n_points"]) == (ib["n_frames"], ib["n_points"]) == (len(frames), int(out_off[-1]))
    for f in frames:
        (xa, ca), (xb, cb) = a.frame_cloud(f), b.frame_cloud(f)
        assert np.array_equal(_bits(xa), _bits(scene["map_thin"][f])) and np.array_equal(_bits(xa), _bits(xb)), f
        assert ca.tobytes() == cb.tobytes(), f
    assert a.frame_cloud(4) is None
    # from scans of four floats a point, as (points, pt_off): the store keeps x y z of the thinned points
    pts4, off4 = _pack([p[off[f]:off[f + 1]] for f in frames[:3]], 4)
    a.set_frame_scans([40, 41, 42], (pts4, off4), 0.25, k_neighbors=10)
    for k, f in enumerate(frames[:3]):
        assert np.array_equal(_bits(a.frame_cloud(40 + k)[0]), _bits(scene["map_thin"][f])), f
    a.close()
    b.close()


def test_the_leaf_forms_register_from_the_view(mods, scene):
    import torch
    manager = mods[0]
    cfg, p, l, off = scene["cfg"], scene["p"], scene["l"], scene["off"]
    qp, ql, qo, frames = scene["qp"], scene["ql"], scene["qo"], scene["frames"]
    h = manager.STDescManager()
    h.add_scans(p, l, off, cfg)
    h.add_scans(p[off[3]:off[4]], l[off[3]:off[4]], np.array([0, 6000], np.int64), cfg)      # frame 20 repeats scan 3
    res = h.query_scans(qp, ql, qo, cfg)
    assert np.all(res.n_cand > 0)
    h.set_frame_scans(frames + [20], [p[off[f]:off[f + 1], :3] for f in frames + [3]], 0.25, k_neighbors=10)
    tq, to = _pack(scene["q_thin"])
    raw = np.ascontiguousarray(qp[:, :3])
    opt = dict(k_neighbors=10, max_iterations=5, max_corr_dist=3.0)
    # register_stored: chosen pairs
    src, tgt = [0, 1, 2, 0], [3, 9, 15, 20]
    want = h.register_stored(tq, to, src, tgt, **opt)
    want_cov = [h.stored_covariances(c) for c in range(3)]
    want_matches = [h.stored_matches(k) for k in range(4)]
    for points in (raw, torch.from_numpy(raw).cuda(), qp):      # (host, device, and four floats a point)
        got = h.register_stored(points, qo, src, tgt, leaf=0.25, **opt)
        _same_dict(got, want, "register_stored")
        for c in range(3):
            assert h.stored_covariances(c).tobytes() == want_cov[c].tobytes(), c
        for k in range(4):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(h.stored_matches(k), want_matches[k])), k
    assert want["n_matched"].min() > 50
    # register_stored_voxels: one map of two frames
    vopt = dict(k_neighbors=10, max_iterations=5)
    want = h.register_stored_voxels(tq, to, [0, 2], [3, 5], None, [0, 1], [0, 0], **vopt)
    _same_dict(h.register_stored_voxels(raw, qo, [0, 2], [3, 5], None, [0, 1], [0, 0], leaf=0.25, **vopt), want, "register_stored_voxels")
    # the loops forms, after verify()
    h.verify()
    want = h.register_loops_stored(tq, to, max_per_query=4, **opt)
    assert len(want["query"]) >= 3
    _same_dict(h.register_loops_stored(raw, qo, max_per_query=4, leaf=0.25, **opt), want, "register_loops_stored")
    _same_dict(h.register_loops_stored(torch.from_numpy(qp).cuda(), qo, max_per_query=4, leaf=0.25, **opt), want, "register_loops_stored, device")
    poses = np.zeros((21, 3, 4), np.float32)      # (rows of the row-major 3x4 [R | t]: the frames 2 m apart along x)
    poses[:, :, :3] = np.eye(3)
    poses[:, 0, 3] = np.arange(21) * 2.0
    h.set_frame_poses(np.arange(21), poses.reshape(21, 12))
    want = h.register_loops_local_stored(tq, to, radius=5.0, max_per_query=2, **vopt)
    got = h.register_loops_local_stored(raw, qo, radius=5.0, max_per_query=2, leaf=0.25, **vopt)
    assert len(want["query"]) >= 1 and set(got) == set(want)
    for f in want:
        if f == "members":
            assert all(np.array_equal(x, y) for x, y in zip(got[f], want[f]))
        elif f == "map_frames":
            assert got[f] == want[f]
        else:
            assert np.asarray(got[f]).tobytes() == np.asarray(want[f]).tobytes(), f
    # the thinned queries are still what the view holds, after all those calls
    view = h.thin_results()
    assert np.array_equal(_bits(view["points"]), _bits(tq)) and np.array_equal(view["pt_off"], to)
    h.close()
