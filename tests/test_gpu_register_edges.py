"""sgtd_register_clouds at its structural edges, bit for bit against the restatement (tests/_register_ref.py): sizes around
the source tile, the target tile and the slice, tiny clouds, k above n, duplicates and exact ties, the max_corr_dist
edge, NaN and infinite coordinates, rejected trials and "LM failed", the stride and the side the points lie on."""
import os

import numpy as np
import pytest

import _register_edges as rx
import _register_ref as ref

pytestmark = pytest.mark.gpu

EYE = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import manager
    return manager


@pytest.fixture(scope="module")
def g(mods):
    h = mods.STDescManager()
    yield h
    h.close()


@pytest.fixture(scope="module")
def tiles(g):
    return g.register_tiles()


@pytest.fixture()
def slice_hook():
    """sets the SGTD_REG_SLICE_TILES hook for one test and puts back what was there"""
    old = os.environ.get("SGTD_REG_SLICE_TILES")

    def set_tiles(n):
        if n is None:
            os.environ.pop("SGTD_REG_SLICE_TILES", None)
        else:
            os.environ["SGTD_REG_SLICE_TILES"] = str(n)

    yield set_tiles
    set_tiles(old)


# ---- tile edges ----
def test_source_tile_edges(g, tiles):
    T = tiles[0]
    sizes = [T - 1, T, T + 1, 2 * T + 1]
    clouds, near = [], None
    for k, n in enumerate(sizes):
        s, t, Rm, tm = rx.surfaces(n, 400, 20 + k)
        clouds += [s, t]
        near = ref.near_start(Rm, tm)
    got, _ = rx.check(g, clouds, [0, 2, 4, 6], [1, 3, 5, 7], np.array([near] * 4), "source tiles", k_neighbors=8, max_corr_dist=2.0,
                      max_iterations=3)
    assert [len(m[0]) for m in got["matches"]] == sizes and (got["n_matched"] > 0).all()


def test_target_tile_and_slice_edges(g, tiles, slice_hook):
    T, S = tiles[1], tiles[2]
    assert S == 2 * T
    sizes = [T - 1, T, T + 1, 2 * T + 1]                    # (2 T + 1 = S + 1: a second slice of one point)
    clouds, near = [], None
    for k, n in enumerate(sizes):
        s, t, Rm, tm = rx.surfaces(130, n, 40 + k)
        clouds += [s, t]
        near = ref.near_start(Rm, tm)
    args = (clouds, [0, 2, 4, 6], [1, 3, 5, 7], np.array([near] * 4))
    opt = dict(k_neighbors=8, max_corr_dist=2.0, max_iterations=3)
    got, want = rx.check(g, *args, "target tiles", **opt)
    # the same under other splits of the target: slices of one tile (three of them for 2 T + 1) and one slice for all
    for n in (1, 64):
        slice_hook(n)
        assert g.register_tiles()[2] == n * T
        rx.compare(rx.run(g, *args, **opt), want, "slices of %d tiles" % n)
    slice_hook(None)
    # a match in the second slice wins only when it is strictly nearer: the target's last point a copy of its first
    # (the source is part of the target, so the pose stays the identity exactly)
    _, t, _, _ = rx.surfaces(60, S + 1, 50)
    t = t.copy()
    t[S] = t[0]
    got, _ = rx.check(g, [t[:60], t], [0], [1], None, "a tie across slices", k_neighbors=8, max_iterations=1)
    assert np.array_equal(got["pose"][0], EYE) and got["matches"][0][0].tolist() == list(range(60)) and got["fitness"][0] == 0.0


# ---- small clouds and repeats ----
def test_tiny_clouds_on_either_side(g):
    rng = np.random.default_rng(3)
    big = rng.normal(0.0, 1.0, (40, 3)).astype(np.float32)
    tiny = [(big[:n] + np.float32(0.05)).astype(np.float32) for n in range(5)]
    clouds = [big] + tiny
    src = [1, 2, 3, 4, 5, 0, 0, 0, 0, 0, 3, 2]
    tgt = [0, 0, 0, 0, 0, 1, 2, 3, 4, 5, 3, 4]
    got, _ = rx.check(g, clouds, src, tgt, None, "tiny", k_neighbors=20, max_iterations=4)      # (k above n everywhere)
    assert got["status"][0] == ref.NO_POINTS and got["status"][5] == ref.NO_POINTS and got["iterations"][0] == 0
    assert np.isnan(got["fitness"][[0, 5]]).all() and got["matches"][0][0].size == 0 and (got["matches"][5][0] == -1).all()
    assert (got["n_matched"][1:5] == [1, 2, 3, 4]).all()
    # "no points" keeps the start pose bit for bit
    init = np.array([ref.near_start(np.eye(3), np.zeros(3))] * 2)
    got, _ = rx.check(g, clouds, [1, 0], [0, 1], init, "no points, a start pose", k_neighbors=5)
    assert ref.same(got["pose"], init) and np.isnan(got["cost"]).all()


def test_duplicates_ties_and_the_distance_edge(g):
    rng = np.random.default_rng(4)
    lattice = rng.integers(-3, 4, (60, 3)).astype(np.float32)
    cloud = np.concatenate([lattice, lattice[:9], lattice[5:6]])        # duplicates: equal d2, equal points
    got, want = rx.check(g, [cloud, lattice], [0, 1], [1, 0], None, "lattice", k_neighbors=10, max_iterations=2)
    assert (got["matches"][0][0][60:69] == want["matches"][0][0][:9]).all()
    # equidistant targets go to the lowest index; d2 == max_corr_dist^2 is excluded, the next double above it is not
    tgt = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, 2], [0, 0, 2], [7, 7, 7], [7, 8, 7], [8, 7, 7], [7, 7, 8]], np.float32)
    src = np.array([[0, 0, 0], [0, 0, 4], [0, 0, 1.5], [50, 0, 0], [7, 7, 7.5]], np.float32)
    for mcd, j in ((2.0, [0, -1, 3, -1, 5]), (float(np.nextafter(2.0, 3.0)), [0, 3, 3, -1, 5]), (float("inf"), [0, 3, 3, 7, 5])):
        got, _ = rx.check(g, [src, tgt], [0], [1], None, "max_corr_dist %r" % mcd, k_neighbors=3, max_corr_dist=mcd, max_iterations=1,
                          lm_max_trials=1)
        assert got["iterations"][0] == 1
        first = ref.correspondences(np.eye(3), np.zeros(3), src.astype(np.float64), tgt.astype(np.float64), mcd * mcd)[0]
        assert first.tolist() == j


def test_nan_and_infinite_coordinates(g):
    s, t, Rm, tm = rx.surfaces(150, 200, 60)
    s, t = s.copy(), t.copy()
    s[7, 0] = np.nan
    s[30] = [np.inf, 0.0, 0.0]
    s[31, 2] = -np.inf
    t[3, 1] = np.nan
    t[90, 0] = np.inf
    t[91] = [np.nan, np.nan, np.nan]
    got, _ = rx.check(g, [s, t], [0, 1], [1, 0], np.array([ref.near_start(Rm, tm), EYE]), "NaN and inf", k_neighbors=8, max_corr_dist=2.0,
                      max_iterations=4)
    j, d2 = got["matches"][0]
    assert (j[[7, 30, 31]] == -1).all() and (d2[[7, 30, 31]] == np.inf).all() and not np.isin(j, [3, 90, 91]).any()
    assert 100 < got["n_matched"][0] == (j >= 0).sum() <= 147 and np.isfinite(got["pose"]).all() and np.isfinite(got["fitness"]).all()
    flat = np.diag([1.0, 1.0, 1e-3])
    assert all(np.array_equal(got["cov"][0][i], flat) for i in (7, 30, 31)) and np.array_equal(got["cov"][1][91], flat)
    # a cloud of nothing but bad points: no correspondence
    bad = np.full((5, 3), np.nan, np.float32)
    got, _ = rx.check(g, [bad, t], [0, 1], [1, 0], None, "all NaN", k_neighbors=8)
    assert got["status"].tolist() == [ref.NO_CORRESPONDENCE] * 2 and got["iterations"].tolist() == [1, 1]


# ---- control ----
def test_rejected_trials_and_lm_failed(g):
    s, t, init = ref.overshoot_case()
    opt = dict(k_neighbors=10, max_iterations=30)
    got, want = rx.check(g, [s, t], [0], [1], init[None], "overshoot", **opt)
    assert got["status"][0] == ref.CONVERGED
    one, _ = rx.check(g, [s, t], [0], [1], init[None], "one trial", lm_max_trials=1, **opt)
    assert one["status"][0] == ref.LM_FAILED and 1 < one["iterations"][0] < got["iterations"][0]
    two, _ = rx.check(g, [s, t], [0], [1], init[None], "two trials", lm_max_trials=2, **opt)
    assert two["status"][0] == ref.LM_FAILED


@pytest.mark.parametrize("n_pairs", [1, 5, 7])
def test_pair_counts_off_the_group(g, n_pairs):
    """pair counts that are no multiple of the rounds enqueued at once (4), the pairs ending in different rounds"""
    s, t, Rm, tm = rx.surfaces(140, 180, 70)
    near = ref.near_start(Rm, tm)
    init = np.array([near if k % 2 else EYE for k in range(n_pairs)])
    src, tgt = [0, 1, 0, 0, 1, 0, 0][:n_pairs], [1, 0, 1, 0, 1, 1, 1][:n_pairs]
    got, _ = rx.check(g, [s, t], src, tgt, init, "%d pairs" % n_pairs, k_neighbors=8, max_corr_dist=2.0, max_iterations=6)
    if n_pairs > 1:
        assert len(set(got["iterations"].tolist())) > 1


# ---- stride and input side ----
def test_stride_and_device_points(g):
    s, t, Rm, tm = rx.surfaces(200, 260, 80)
    args = ([s, t], [0, 1], [1, 0], np.array([ref.near_start(Rm, tm), EYE]))
    opt = dict(k_neighbors=8, max_corr_dist=2.0, max_iterations=5)
    got, want = rx.check(g, *args, "stride 3", **opt)
    rx.compare(rx.run(g, *args, stride=4, **opt), want, "stride 4")
    rx.compare(rx.run(g, *args, dev=True, **opt), want, "device points")
    rx.compare(rx.run(g, *args, dev=True, stride=4, **opt), want, "device points, stride 4")
