"""sgtd_register_voxels at its structural edges, bit for bit against the restatement (tests/_voxel_register_ref.py): the
ways one map can be given, sizes around the tiles of the kernels, voxel runs around the width of VSUM, points on voxel
boundaries and at the ends of the coordinate range, non-finite coordinates, duplicates, resolutions."""
import numpy as np
import pytest

import _register_ref as ref
import _voxel_register_edges as vx
import _voxel_register_ref as vref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    from sgtd_amd import manager
    h = manager.STDescManager()
    yield h
    h.close()


def _scene(n, seed):
    s, t, Rm, tm = ref.planted_scene(n, seed)
    return s, t, ref.near_start(Rm, tm)


def test_the_ways_to_give_one_map(g):
    s, t, near = _scene(200, 9)
    empty = np.zeros((0, 3), np.float32)
    clouds = [s, t, empty]
    opt = dict(k_neighbors=8, neighbor_mode=7)
    null, _ = vx.check(g, clouds, [0, 1], [1], None, [0], [0], near[None], "NULL map_pose", **opt)
    eye, _ = vx.check(g, clouds, [0, 1], [1], vx.EYE[None], [0], [0], near[None], "identity map_pose", **opt)
    more, _ = vx.check(g, clouds, [0, 3], [2, 1, 2], np.array([vx.EYE] * 3), [0], [0], near[None], "empty members", **opt)
    for other in (eye, more):
        assert vx.same_maps(other["maps"][0], null["maps"][0]) and np.array_equal(other["matches"][0], null["matches"][0])
        for f in vx.FIELDS:
            assert ref.same(other[f], null[f]), f
    # two members in either order: the voxels are the same, the sums are taken in member order: both as restated
    a, b = t[:110], t[90:]
    pa, pb = vx.pose_row([0.2, 1.0, 0.1], 0.003, [0.02, 0.0, -0.01]), vx.pose_row([1.0, 0.1, 0.0], -0.002, [0.0, 0.01, 0.0])
    ab, _ = vx.check(g, [s, a, b], [0, 2], [1, 2], np.array([pa, pb]), [0], [0], near[None], "members a, b", **opt)
    ba, _ = vx.check(g, [s, a, b], [0, 2], [2, 1], np.array([pb, pa]), [0], [0], near[None], "members b, a", **opt)
    assert np.array_equal(ab["maps"][0]["coord"], ba["maps"][0]["coord"]) and np.array_equal(ab["maps"][0]["n_points"], ba["maps"][0]["n_points"])
    assert np.allclose(ab["maps"][0]["mean"], ba["maps"][0]["mean"], rtol=0, atol=1e-12)
    # a cloud twice in one map: every voxel counts its points twice
    twice, _ = vx.check(g, clouds, [0, 2], [1, 1], None, [0], [0], near[None], "a member twice", **opt)
    assert np.array_equal(twice["maps"][0]["n_points"], 2 * null["maps"][0]["n_points"])


def test_source_sizes_around_the_tiles(g):
    s, t, near = _scene(300, 5)
    sizes = [127, 128, 129, 255, 256, 257, 1]
    clouds = [s[:n] for n in sizes] + [t]
    n = len(sizes)
    got, _ = vx.check(g, clouds, [0, 1], [n], None, list(range(n)), [0] * n, np.array([near] * n), "source sizes", k_neighbors=6, neighbor_mode=7,
                      max_iterations=4)
    assert [len(m) for m in got["matches"]] == [7 * k for k in sizes]


def test_a_map_across_sort_blocks(g):
    """4900 member points: more than one block of the radix sort (4096) and of the scan (2048); seven posed copies of
    one cloud, so the covariances are computed once"""
    s, t, near = _scene(600, 3)
    rng = np.random.default_rng(1)
    poses = np.array([vx.pose_row(rng.normal(0, 1, 3), 0.002 * k, rng.normal(0, 0.05, 3)) for k in range(7)])
    got, _ = vx.check(g, [s[:150], t], [0, 7], [1] * 7, poses, [0], [0], near[None], "4900 member points", k_neighbors=6, max_iterations=3)
    assert got["maps"][0]["n_points"].sum() == 7 * 700


def test_voxel_runs_around_the_width_of_the_sum(g):
    rng = np.random.default_rng(12)
    runs = [1, 2, 63, 64, 65, 127, 128, 129, 200]
    corner = np.array([[3 * k, -2 * k, k] for k in range(len(runs))], np.float64)
    pts = np.concatenate([corner[k] + 0.5 + rng.uniform(0.05, 0.95, (n, 3)) for k, n in enumerate(runs)])
    pts = pts[rng.permutation(len(pts))].astype(np.float32)
    src = (pts[::3].astype(np.float64) + rng.normal(0, 0.01, (len(pts[::3]), 3))).astype(np.float32)
    got, _ = vx.check(g, [src, pts], [0, 1], [1], None, [0], [0], None, "voxel runs", k_neighbors=6, max_iterations=3)
    assert sorted(got["maps"][0]["n_points"].tolist()) == sorted(runs)


def _edge_cloud(res):
    """points exactly on voxel boundaries (x / res - 0.5 integral) and one f32 step either side, negative coordinates, the
    ends of the coordinate range and just outside, non-finite coordinates, duplicates, and a bulk that gives them
    neighbours"""
    f32 = np.float32
    rows = []
    for k in (-3, -1, 0, 1, 2):
        b = f32((k + 0.5) * res)
        for v in (b, np.nextafter(b, f32(np.inf)), np.nextafter(b, f32(-np.inf))):
            rows += [[v, f32(0.25 * res), f32(-1.25 * res)], [f32(0.75 * res), v, v]]
    lo, hi = f32((-32768 + 0.5) * res), f32((32767 + 0.5) * res)
    out_lo, out_hi = np.nextafter(lo, f32(-np.inf)), f32((32768 + 0.5) * res)
    for v in (lo, hi, out_lo, out_hi, np.nextafter(f32((32767 + 1.5) * res), f32(-np.inf))):
        rows += [[v, f32(0.1), f32(0.2)], [f32(0.3), v, f32(-0.4)], [f32(-0.2), f32(0.6), v]]
    rows += [[lo, lo, lo], [hi, hi, hi], [lo, hi, f32(0.0)]]
    rows += [[np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [1.0, 2.0, -np.inf], [np.nan, np.nan, np.nan]]
    rng = np.random.default_rng(77)
    bulk = rng.uniform(-3.0, 3.0, (60, 3)) * res
    rows += bulk.tolist() + bulk[:9].tolist() + [[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0]]      # duplicates, both zeros
    return np.array(rows, np.float32)


@pytest.mark.parametrize("res", [1.0, 0.5])
@pytest.mark.parametrize("mode", [1, 27])
def test_voxel_edges(g, res, mode):
    cloud = _edge_cloud(res)
    shift = vx.pose_row([0.0, 0.0, 1.0], 0.0, [0.25 * res, 0.0, -0.5 * res])      # moves boundary points across and range ends out
    got, want = vx.check(g, [cloud, cloud[::-1].copy()], [0, 1, 2], [0, 1], None, [0, 1, 0], [0, 0, 1], np.array([vx.EYE, vx.EYE, shift]),
                         "voxel edges", k_neighbors=5, neighbor_mode=mode, voxel_resolution=res, max_iterations=2)
    m = got["maps"][0]
    assert m["coord"].min() == -32768 and m["coord"].max() == 32767
    n_in = int(vref.coords(cloud.astype(np.float64), res)[1].sum())
    assert m["n_points"].sum() == n_in < len(cloud)
    # a source point that enters no voxel has no correspondence: pair 2 ends where it started if nothing matched, and
    # whatever the poses, every row of a non-finite source point is -1
    bad = ~np.isfinite(cloud).all(1)
    for k, c in ((0, 0), (1, 1), (2, 0)):
        rows = got["matches"][k].reshape(-1, mode)
        assert (rows[(bad if c == 0 else bad[::-1])] == -1).all()


@pytest.mark.parametrize("res", [0.5, 1.0, 4.0])
def test_resolutions(g, res):
    s, t, near = _scene(300, 7)
    got, _ = vx.check(g, [s, t], [0, 1], [1], None, [0, 0], [0, 0], np.array([vx.EYE, near]), "resolution %g" % res, k_neighbors=10,
                      neighbor_mode=7, voxel_resolution=res)
    assert (got["n_corr"] > 0).all()


def test_status_paths(g):
    """rejected trials and "LM failed": overshoot_case's clouds started 3 degrees off (test_voxel_register_host.py measures
    the restatement there); from its own start, 10 degrees off, no source point lands near a voxel"""
    s, t, off = ref.overshoot_case()
    init = np.array([np.concatenate([ref.rot_axis([0.0, 0.0, 1.0], np.deg2rad(3.0)).reshape(9), np.zeros(3)]), off])
    opt = dict(k_neighbors=10, max_iterations=30, neighbor_mode=27, voxel_resolution=4.0)
    got, _ = vx.check(g, [s, t], [0, 1], [1], None, [0, 0], [0, 0], init, "overshoot", **opt)
    assert got["status"].tolist() == [vref.CONVERGED, vref.NO_CORRESPONDENCE] and got["iterations"][0] > 5
    one, _ = vx.check(g, [s, t], [0, 1], [1], None, [0, 0], [0, 0], init, "overshoot, one trial", lm_max_trials=1, **opt)
    assert one["status"].tolist() == [vref.LM_FAILED, vref.NO_CORRESPONDENCE] and one["iterations"][0] < got["iterations"][0]
    few, _ = vx.check(g, [s, t], [0, 1], [1], None, [0], [0], init[:1], "overshoot, three iterations", **dict(opt, max_iterations=3))
    assert few["status"].tolist() == [vref.ITERATION_LIMIT] and few["iterations"].tolist() == [3]
