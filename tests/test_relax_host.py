"""sgtd_relax_poses without a device: the numpy restatement of the rule (tests/_relax_ref.py) on hand-made graphs and on
planted worlds, an independent least-squares solve of the same residual, the header's prototypes and the ctypes binding."""
import ctypes
import os
import re

import numpy as np
import pytest

import _relax_edges as rx
import _relax_ref as rr
from sgtd_amd import _lib, manager

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_relax_poses": ["sgtd_handle h", "int64_t n_nodes", "const double *pose0", "const uint8_t *fixed", "int64_t n_edges",
                         "const int32_t *node_i", "const int32_t *node_j", "const double *meas", "const double *w_trans",
                         "const double *w_rot", "const sgtd_relax_options *opt", "sgtd_relax_report *report"],
    "sgtd_result_relaxed": ["sgtd_handle h", "double *pose", "double *edge_cost"],
}


def test_header_declares_the_calls():
    header = open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()
    for name, want in DECLS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, name + " is not declared"
        text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        assert [" ".join(a.split()) for a in text.split(",")] == want, name
    assert re.search(r"void\s+sgtd_default_relax_options\s*\(\s*sgtd_relax_options\s*\*\s*opt\s*\)\s*;", header)
    assert re.search(r"^#define\s+SGTD_RELAX_SUM_W\s+%d\b" % rr.W, header, re.M)
    assert re.search(r"^#define\s+SGTD_RELAX_GROUP\s+%d\b" % rx.GROUP, header, re.M)
    m = re.search(r"enum\s*\{\s*SGTD_RELAX_CONVERGED = (\d), SGTD_RELAX_OUTER_LIMIT = (\d), SGTD_RELAX_DAMPING_LIMIT = (\d), "
                  r"SGTD_RELAX_NOTHING_FREE = (\d)\s*\}", header)
    assert m and [int(v) for v in m.groups()] == [rr.CONVERGED, rr.OUTER_LIMIT, rr.DAMPING_LIMIT, rr.NOTHING_FREE]
    # the structs' fields, in order
    for struct, cls in (("sgtd_relax_options", _lib.RelaxOptions), ("sgtd_relax_report", _lib.RelaxReport)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [v.strip() for v in decl.split(None, 1)[1].split(",")]
        assert names == [f[0].rstrip("_") for f in cls._fields_], struct


def test_binding_declares_the_calls():
    for name in list(DECLS) + ["sgtd_default_relax_options"]:
        assert name in _lib.SYMBOLS, name
    L = _lib.lib()
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    assert L.sgtd_relax_poses.argtypes == [vp, i64, vp, vp, i64, vp, vp, vp, vp, vp, ctypes.POINTER(_lib.RelaxOptions),
                                           ctypes.POINTER(_lib.RelaxReport)]
    assert L.sgtd_result_relaxed.argtypes == [vp, vp, vp]
    for name, want in DECLS.items():
        assert len(getattr(L, name).argtypes) == len(want) and getattr(L, name).restype is ctypes.c_int
    o = _lib.RelaxOptions()
    L.sgtd_default_relax_options(ctypes.byref(o))
    assert {f[0]: getattr(o, f[0]) for f in _lib.RelaxOptions._fields_} == rr.DEFAULTS
    assert ctypes.sizeof(_lib.RelaxOptions) == 48 and ctypes.sizeof(_lib.RelaxReport) == 40
    # a NULL handle is SGTD_ERR_INVALID without a device
    assert L.sgtd_relax_poses(None, 0, None, None, 0, None, None, None, None, None, None, None) == -1
    assert L.sgtd_result_relaxed(None, None, None) == -1


def test_ordered_sum_is_its_plain_loop():
    rng = np.random.default_rng(5)
    for n in (0, 1, 5, rr.W - 1, rr.W, rr.W + 1, 3 * rr.W + 17):
        v = rng.normal(0.0, 1.0, n) * 10.0 ** rng.integers(-8, 8, n)
        assert rr.ordered_sum(v).tobytes() == np.float64(rr.ordered_sum_loop(v)).tobytes(), n
    # the order matters: element 0 and element W share an accumulator, element 1 does not
    v = np.zeros(rr.W + 1)
    v[0], v[1], v[rr.W] = 1e16, 1.0, -1e16
    assert rr.ordered_sum(v) == 1.0 and rr.ordered_sum(v[[0, rr.W, 1]]) == 0.0
    assert rr.ordered_max(np.array([0.5, 3.0, 2.0])) == 3.0 and rr.ordered_max(np.zeros(0)) == 0.0


def test_quaternion_branches_and_products():
    rng = np.random.default_rng(9)
    # rotations by 170 degrees about axes near x, y, z and a small one: the four branches of QUAT
    axes = [np.array(a, float) for a in ([1, .1, .1], [.1, 1, .1], [.1, .1, 1])]
    Rs = [rr.rot_vec(a / np.linalg.norm(a) * np.deg2rad(170.0)) for a in axes] + [rr.rot_vec([0.1, -0.2, 0.05])]
    R = np.array(Rs)
    tr = np.trace(R, axis1=1, axis2=2)
    assert (tr[:3] < 0).all() and tr[3] > 0 and [int(np.argmax(np.diag(r))) for r in Rs[:3]] == [0, 1, 2]
    q = rr.quat_of(R)
    assert np.allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-15)
    assert np.allclose(rr.rot_of(q), R, atol=1e-14)
    X = rx.random_poses(4, rng)
    I = rr.mul(rr.inv(X), X)
    assert np.allclose(I[0], np.eye(3), atol=1e-14) and np.allclose(I[1], 0.0, atol=1e-13)


def test_jacobian_blocks_match_finite_differences():
    """the header's first-order blocks against central differences of the residual, at a state with a small rotational
    residual (the blocks are exact at zero): 5e-2 of the block's scale covers the second-order term of a 0.03 rad residual"""
    g = rx.random_graph(5, 8, 21)
    n = 5
    held = np.zeros(n, bool)
    q = rr.quat_of(g["pose0"].reshape(n, 3, 4)[:, :, :3])
    t = g["pose0"].reshape(n, 3, 4)[:, :, 3].copy()
    R = rr.rot_of(q)
    G = rr.Graph(n, g["node_i"], g["node_j"], g["meas"], None, None, held)
    ev = G.evaluate(q, t, R)
    lin = G.linearise(ev)
    eps = 1e-6

    def res(x):
        q2, t2, R2 = rr.retract(q, t, R, x, ~held)
        e = G.evaluate(q2, t2, R2)
        return np.concatenate([e["rt"], e["rR"]], 1)

    for v in range(n):
        for a in range(6):
            x = np.zeros((n, 6))
            x[v, a] = eps
            num = (res(x) - res(-x)) / (2 * eps)                # [m, 6]: d residual / d x[v][a]
            for k in range(G.m):
                col = np.zeros(6)
                if G.i[k] == v:
                    J = np.zeros((6, 6))
                    J[:3, :3], J[:3, 3:], J[3:, 3:] = -lin["A"][k], lin["B"][k], -lin["DR"][k].T
                    col = J[:, a]
                elif G.j[k] == v:
                    J = np.zeros((6, 6))
                    J[:3, :3], J[3:, 3:] = lin["ER"][k], np.eye(3)
                    col = J[:, a]
                assert np.allclose(num[k], col, atol=5e-2 * max(1.0, np.abs(col).max())), (v, a, k)
    # and the matrix-free product is the blocks': apply() against the dense J^T W J (+ lambda diag blocks)
    H = G.blocks(lin)
    p = np.random.default_rng(1).normal(0.0, 1.0, (n, 6))
    dense = np.zeros((G.m * 6, n * 6))
    for k in range(G.m):
        dense[k * 6:k * 6 + 3, G.i[k] * 6:G.i[k] * 6 + 3] = -lin["A"][k]
        dense[k * 6:k * 6 + 3, G.i[k] * 6 + 3:G.i[k] * 6 + 6] = lin["B"][k]
        dense[k * 6 + 3:k * 6 + 6, G.i[k] * 6 + 3:G.i[k] * 6 + 6] = -lin["DR"][k].T
        dense[k * 6:k * 6 + 3, G.j[k] * 6:G.j[k] * 6 + 3] = lin["ER"][k]
        dense[k * 6 + 3:k * 6 + 6, G.j[k] * 6 + 3:G.j[k] * 6 + 6] = np.eye(3)
    JtJ = dense.T @ dense
    lam = 0.5
    want = JtJ @ p.reshape(-1)
    for v in range(n):
        assert np.allclose(H[v], JtJ[v * 6:v * 6 + 6, v * 6:v * 6 + 6], atol=1e-9)
        want[v * 6:v * 6 + 6] += lam * (H[v] @ p[v])
    assert np.allclose(G.apply(lin, H, lam, p).reshape(-1), want, atol=1e-9)
    L, ok = rr.cholesky(H + lam * H)
    assert ok.all()
    for v in range(n):
        assert np.allclose(L[v] @ L[v].T, H[v] + lam * H[v], atol=1e-9)
        assert np.allclose(rr.solve(L, ok, p)[v], np.linalg.solve(H[v] + lam * H[v], p[v]), rtol=1e-8, atol=1e-10)


def test_noise_free_graph_starts_converged():
    g = rx.random_graph(9, 14, 3, noise=False)
    # the start is the state's own pose (R = ROT(QUAT(.))) only to rounding, so the cost is rounding's: below 1e-24
    ref = rx.reference(g)
    assert ref["status"] == rr.CONVERGED and ref["cost_after"] <= ref["cost_before"] < 1e-24
    # half turns about the axes and whole translations are exact in every step of the rule (their quaternions are
    # unit vectors of the basis): cost 0.0, no iteration
    R = np.array([np.diag(d) for d in ([1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1])])
    t = np.array([[0, 0, 0], [2, 0, 0], [2, 3, 0], [0, 3, 1]], float)
    i, j = [0, 1, 2, 3], [1, 2, 3, 0]
    g = rx.graph(rr.rows34(R, t), i, j, rx.measure(R, t, i, j, None))
    ref = rx.reference(g)
    assert ref["cost_before"] == 0.0 and ref["cost_after"] == 0.0 and ref["status"] == rr.CONVERGED
    assert ref["outer"] == 0 and ref["cg"] == 0 and np.array_equal(ref["pose"], g["pose0"])


def test_hand_made_cases():
    # everything held: the cost is evaluated, nothing moves
    g = rx.random_graph(4, 5, 8, fixed=np.ones(4, np.uint8))
    ref = rx.reference(g)
    assert ref["status"] == rr.NOTHING_FREE and ref["cost_before"] == ref["cost_after"] > 0 and ref["outer"] == 0
    # empty graphs
    for g in (rx.graph(np.zeros((0, 12)), [], [], np.zeros((0, 12))), rx.graph(rx.random_graph(3, 2, 1)["pose0"], [], [], np.zeros((0, 12)))):
        ref = rx.reference(g)
        assert ref["status"] == rr.NOTHING_FREE and ref["cost_before"] == 0.0 and ref["pose"].shape == (0, 12)
    # an isolated free node stays where it is, bit for bit, while the others move
    g = rx.random_graph(5, 6, 13)
    lone = rx.graph(np.concatenate([g["pose0"], g["pose0"][2:3] * 1.0]), g["node_i"], g["node_j"], g["meas"])
    ref, ref5 = rx.reference(lone), rx.reference(g)
    start = rr.rows34(rr.rot_of(rr.quat_of(lone["pose0"].reshape(-1, 3, 4)[:, :, :3])), lone["pose0"].reshape(-1, 3, 4)[:, :, 3])
    assert np.array_equal(ref["pose"][5], start[5]) and np.array_equal(ref["pose"][0], start[0])
    assert np.array_equal(ref["pose"][:5], ref5["pose"]) and ref["cost_after"] < ref["cost_before"]
    # a zero-weight edge has no say: with it or without it the poses are the same (its own cost is 0)
    g = rx.random_graph(6, 9, 17)
    bad = rx.graph(g["pose0"], list(g["node_i"]) + [0], list(g["node_j"]) + [5], np.concatenate([g["meas"], g["meas"][:1]]),
                   w_trans=np.array([1.0] * 9 + [0.0]), w_rot=np.array([1.0] * 9 + [0.0]))
    a, b = rx.reference(g), rx.reference(bad)
    assert np.allclose(a["pose"], b["pose"], atol=1e-9) and (b["edge_cost"][9] == 0.0).all()
    # a block is taken whole: a node whose edges all have w_rot == 0 is not solvable and does not move at all
    touching = (g["node_i"] == 5) | (g["node_j"] == 5)
    ref = rx.reference(dict(g, w_trans=np.ones(9), w_rot=np.where(touching, 0.0, 1.0)))
    R, t = rr.poses_of(g["pose0"])
    assert np.array_equal(ref["pose"][5], rr.rows34(rr.rot_of(rr.quat_of(R)), t)[5]) and ref["cost_after"] < ref["cost_before"]
    # cost_after <= cost_before whatever the limits
    for opt in (dict(max_outer=1), dict(max_outer=2, max_inner=1), dict(lambda_init=1e6), dict(lambda_init=1e-9, lambda_max=1e-8)):
        ref = rx.reference(g, **opt)
        assert ref["cost_after"] <= ref["cost_before"], opt


WORLDS = {"self": dict(n=60, n_loops=12, seed=3), "map": dict(n=40, n_loops=10, seed=11, odo_t=0.04, odo_r=np.deg2rad(1.2))}


def _map_world():
    """a session of 40 frames localised against a held map: the map frames are the ground truth of every fourth frame
    (another session's poses of the same places), each tied to the query frame at that place by a loop"""
    w = rr.planted_world(**WORLDS["map"])
    rng = np.random.default_rng(77)
    Rg, tg = rr.poses_of(w["truth"])
    Ro, to = rr.poses_of(w["odom"])
    places = np.arange(0, 40, 4)
    map_ids = 1000 + places
    fa, fb, rel = [], [], []
    for p in places:                                        # loop (frame_a = p, frame_b = 1000 + p): T = inv(B) X_p
        fa.append(int(p))
        fb.append(1000 + int(p))
        rel.append(np.concatenate([rr.rot_vec(rng.normal(0.0, 1e-3, 3)).reshape(9), rng.normal(0.0, 0.005, 3)]))
    edges = dict(frame_a=np.array(fa, np.uint32), frame_b=np.array(fb, np.uint32), rel_pose=np.array(rel))
    g = manager.relax_graph(np.arange(40), w["odom"], edges, None, held=(map_ids, w["truth"][places]))
    return w, g


def test_planted_worlds_converge_and_pull_the_drift_out():
    w = rr.planted_world(**WORLDS["self"])
    ref = rr.relax(w["odom"], None, w["node_i"], w["node_j"], w["meas"])
    before, after = rr.mean_trans_error(w["odom"], w["truth"]), rr.mean_trans_error(ref["pose"], w["truth"])
    assert ref["status"] == rr.CONVERGED and ref["cost_after"] < ref["cost_before"]
    assert before > 0.5 and after < 0.2 * before, (before, after)      # (measured: 1.00 m -> 0.057 m)
    w, g = _map_world()
    assert g["fixed"][:40].sum() == 0 and g["fixed"][40:].all() and g["pose0"].shape[0] == 50
    ref = rx.reference(g)
    odo_in_map = g["pose0"][:40]
    before, after = rr.mean_trans_error(odo_in_map, w["truth"]), rr.mean_trans_error(ref["pose"][:40], w["truth"])
    assert ref["status"] == rr.CONVERGED and ref["cost_after"] < ref["cost_before"]
    assert np.array_equal(ref["pose"][40:, [3, 7, 11]], g["pose0"][40:, [3, 7, 11]])      # held nodes keep their place
    assert before > 0.3 and after < 0.2 * before, (before, after)


def test_relax_graph_orientation():
    """relax_graph's edges are Z ~ inv(X_i) X_j at the truth: odometry from the poses, loops as i = frame_b, j = frame_a"""
    rng = np.random.default_rng(4)
    R, t = rx.random_poses(6, rng)
    ids = np.array([10, 11, 12, 13, 14, 15])
    T = rx.measure(R, t, [1, 0], [4, 5], rng)               # loops (a = 14, b = 11) and (a = 15, b = 10): T = inv(X_b) X_a
    edges = dict(frame_a=np.array([14, 15, 12]), frame_b=np.array([11, 10, 13]), rel_pose=np.concatenate([T, T[:1]]))
    g = manager.relax_graph(ids, rr.rows34(R, t), edges, in_set=[1, 1, 0])
    assert g["node_i"].tolist() == [0, 1, 2, 3, 4, 1, 0] and g["node_j"].tolist() == [1, 2, 3, 4, 5, 4, 5]
    assert g["fixed"].tolist() == [1, 0, 0, 0, 0, 0]
    ref = rx.reference(g)
    assert ref["cost_before"] < 1e-24 and ref["status"] == rr.CONVERGED


def test_relax_graph_map_ids_may_overlap_the_session_ids():
    """a map numbers its frames from 0 as a session does: frame_b resolves through the map alone"""
    rng = np.random.default_rng(6)
    R, t = rx.random_poses(8, rng)
    mR, mt = rx.random_poses(3, rng)
    odom = rr.rows34(R, t)
    T = rx.measure(R, t, [0, 0, 0, 0], [1, 1, 1, 1], rng)
    # map frames 3, 6 and 2; loops (a = 2, b = 3), (a = 5, b = 6), (a = 2, b = 2: the map's frame 2, not the session's),
    # (a = 7, b = 3: map frame 3 again)
    edges = dict(frame_a=np.array([2, 5, 2, 7]), frame_b=np.array([3, 6, 2, 3]), rel_pose=T)
    g = manager.relax_graph(np.arange(8), odom, edges, held=([3, 6, 2], rr.rows34(mR, mt)))
    assert g["pose0"].shape == (11, 12) and g["n_session"] == 8
    assert g["fixed"].tolist() == [0] * 8 + [1] * 3
    assert g["node_i"].tolist() == list(range(7)) + [8, 9, 10, 8] and g["node_j"].tolist() == list(range(1, 8)) + [2, 5, 2, 7]
    assert np.array_equal(g["pose0"][8:], rr.rows34(mR, mt))
    assert g["w_trans"].tolist() == [1.0] * 11
    # the same graph as with map ids far from the session's
    far = manager.relax_graph(np.arange(8), odom, dict(edges, frame_b=np.array([1003, 1006, 1002, 1003])),
                              held=([1003, 1006, 1002], rr.rows34(mR, mt)))
    for k in g:
        assert np.array_equal(g[k], far[k]), k
    # only the map frames the chosen loops name become nodes; the loop weights go to the loops alone
    g = manager.relax_graph(np.arange(8), odom, edges, in_set=[0, 1, 0, 0], held=([3, 6, 2], rr.rows34(mR, mt)), w_loop=(4.0, 9.0))
    assert g["fixed"].tolist() == [0] * 8 + [1] and g["node_i"].tolist() == list(range(7)) + [8] and g["node_j"][-1] == 5
    assert g["w_trans"].tolist() == [1.0] * 7 + [4.0] and g["w_rot"].tolist() == [1.0] * 7 + [9.0]
    assert np.array_equal(g["pose0"][8], rr.rows34(mR, mt)[1])
    # frames nobody holds
    with pytest.raises(ValueError, match="frame_a 9 is not a frame of the session"):
        manager.relax_graph(np.arange(8), odom, dict(edges, frame_a=np.array([9, 5, 2, 7])), held=([3, 6, 2], rr.rows34(mR, mt)))
    with pytest.raises(ValueError, match="map frame 6"):
        manager.relax_graph(np.arange(8), odom, edges, held=([3, 2], rr.rows34(mR, mt)[:2]))
    with pytest.raises(ValueError, match="frame_b 12 is not a frame of the session"):
        manager.relax_graph(np.arange(8), odom, dict(edges, frame_b=np.array([3, 6, 12, 3])))
    # no frames, one frame
    none = dict(frame_a=np.zeros(0, np.uint32), frame_b=np.zeros(0, np.uint32), rel_pose=np.zeros((0, 12)))
    g = manager.relax_graph(np.zeros(0, int), np.zeros((0, 12)), none, w_loop=(2.0, 2.0))
    assert g["pose0"].shape == (0, 12) and g["node_i"].size == 0 and g["w_trans"].size == 0 and g["fixed"].size == 0
    g = manager.relax_graph([4], odom[:1], none, w_loop=(2.0, 2.0))
    assert g["pose0"].shape == (1, 12) and g["node_i"].size == 0 and g["fixed"].tolist() == [1]


GAP_BOUND = 3.3e-10      # ten times the relative gap measured below (3.3e-11)


def test_independent_least_squares_agrees():
    """scipy's trust-region solve of the same residual function from the same start, on one small world.  Measured here:
    the restatement's cost 3.4607020321e-3, scipy's 3.4607020320e-3, relative gap 3.3e-11 (the two stop by different
    rules); asserted with a tenfold margin over that"""
    scipy_opt = pytest.importorskip("scipy.optimize")
    w = rr.planted_world(16, 4, 2)
    held = np.arange(16) == 0
    ref = rr.relax(w["odom"], None, w["node_i"], w["node_j"], w["meas"])
    assert ref["status"] == rr.CONVERGED
    fun = lambda x: rr.residuals_of(x, w["odom"], held, w["node_i"], w["node_j"], w["meas"], None, None)
    assert np.isclose(np.sum(fun(np.zeros(15 * 6)) ** 2), ref["cost_before"], rtol=1e-12)
    sol = scipy_opt.least_squares(fun, np.zeros(15 * 6), xtol=1e-14, ftol=1e-14, gtol=1e-14)
    best = 2.0 * sol.cost
    gap = abs(ref["cost_after"] - best) / best
    print("restatement %.10e scipy %.10e gap %.3e" % (ref["cost_after"], best, gap))
    assert gap < GAP_BOUND
