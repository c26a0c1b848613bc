"""sgtd_relax_poses at its edges, bit for bit against the restatement (tests/_relax_ref.py): node and edge counts at the
boundaries of the kernels' geometry (the workgroup, one grid pass, SUM's W accumulators over 6 n vector elements and over
m edge costs), gathers longer than a wave and a workgroup, the sign flip of the rotational residual, and every control
path: a rejected step, each status, the outer limit inside, at and across a group of enqueued iterations."""
import numpy as np
import pytest

import _relax_edges as rx
import _relax_ref as rr

pytestmark = pytest.mark.gpu

SHORT = dict(max_outer=3, max_inner=6)      # the geometry cases need every kernel to run, not the optimum


@pytest.fixture(scope="module")
def g():
    from sgtd_amd import manager
    h = manager.STDescManager()
    yield h
    h.close()


@pytest.mark.parametrize("degree", [63, 64, 65, 300])
def test_star_hub_gathers_across_waves_and_workgroups(g, degree):
    got, _ = rx.check(g, rx.star(degree, 100 + degree))
    assert got["status"] == rr.CONVERGED and got["cost_after"] < got["cost_before"]


# nodes: the workgroup (256), SUM over 6 n elements (6 n = W between n = 170 and 171), W itself, and a few thousand
NODE_COUNTS = [rx.THREADS - 1, rx.THREADS, rx.THREADS + 1, rx.W // 6, rx.W // 6 + 1, rx.W - 1, rx.W, rx.W + 1, 4099]


@pytest.mark.parametrize("n", NODE_COUNTS)
def test_node_counts_at_the_boundaries(g, n):
    got, _ = rx.check(g, rx.random_graph(n, n + 7, 200 + n), n, **SHORT)
    assert got["steps_accepted"] >= 1 and got["cg_iterations"] >= 6


# edges: the same boundaries for the per-edge kernels and for SUM over the m edge costs; m = n - 1 is the bare chain
EDGE_COUNTS = [rx.THREADS - 1, rx.THREADS, rx.THREADS + 1, rx.W // 6, rx.W // 6 + 1, rx.W - 1, rx.W, rx.W + 1, 4101]


@pytest.mark.parametrize("m", EDGE_COUNTS)
def test_edge_counts_at_the_boundaries(g, m):
    n = max(m // 3, 2)
    got, _ = rx.check(g, rx.random_graph(n, m, 300 + m, weights=True), m, **SHORT)
    assert got["steps_accepted"] >= 1
    if m in (rx.THREADS, rx.W):
        rx.check(g, rx.random_graph(m + 1, m, 400 + m), "chain of %d edges" % m, **SHORT)


@pytest.mark.parametrize("blocks", [1, 3])
def test_more_nodes_and_edges_than_one_grid_pass(g, monkeypatch, blocks):
    """the SGTD_RELAX_MAX_BLOCKS hook caps a fresh handle's grids at 1 and 3 workgroups: 1000 nodes and 1500 edges then take
    four and two passes of the grid-stride loops (the last one partial), and the answer is the uncapped handle's"""
    from sgtd_amd import manager
    gr = rx.random_graph(1000, 1500, 77, weights=True)
    base, ref = rx.check(g, gr, **SHORT)
    monkeypatch.setenv("SGTD_RELAX_MAX_BLOCKS", str(blocks))
    h = manager.STDescManager()
    try:
        rx.same(rx.run(h, gr, **SHORT), ref, blocks)
        rx.check(h, rx.star(300, 405), "a hub in a capped grid")
    finally:
        h.close()


def _far_start(seed):
    """a graph whose start is turned by up to some 150 degrees at every other node"""
    rng = np.random.default_rng(seed)
    gr = rx.random_graph(12, 20, seed)
    R, t = rr.poses_of(gr["pose0"])
    for k in range(1, 12, 2):
        R[k] = R[k] @ rr.rot_vec(rng.normal(0.0, 1.0, 3) * 2.6 / 1.7)
    gr["pose0"] = rr.rows34(R, t)
    return gr


def test_rotation_residual_beyond_90_degrees_flips_sign(g):
    gr = _far_start(0)
    G = rr.Graph(12, gr["node_i"], gr["node_j"], gr["meas"], None, None, np.arange(12) == 0)
    R, t = rr.poses_of(gr["pose0"])
    q = rr.quat_of(R)
    Rs = rr.rot_of(q)
    E = rr.mul(G.IZ, rr.mul(rr.inv((Rs[G.i], t[G.i])), (Rs[G.j], t[G.j])))
    qe = rr.quat_of(E[0])
    assert (qe[:, 0] < 0).sum() >= 2 and (np.trace(E[0], axis1=1, axis2=2) < 0).sum() >= 2      # flips, and QUAT's other branches
    start = rx.start_costs(gr)
    assert (start[:, 1] <= 4.0 + 1e-12).all() and (start[:, 1] > 2.0).sum() >= 2       # |r_R| = 2 sin(angle / 2): beyond 90 degrees
    got, _ = rx.check(g, gr, max_outer=1)
    assert got["edge_cost"].tobytes() == start.tobytes() or got["steps_accepted"] == 1
    got, _ = rx.check(g, gr)
    assert got["status"] == rr.CONVERGED


def test_rejected_steps_restore_the_state(g):
    """from the far start the first steps overshoot: the restatement rejects four before it accepts one.  Stopped inside
    those, the outputs are the start's; the damping has tripled each time"""
    gr = _far_start(0)
    trace = []
    ref = rr.relax(gr["pose0"], None, gr["node_i"], gr["node_j"], gr["meas"], trace=trace)
    assert [s["accepted"] for s in trace[:5]] == [False, False, False, False, True] and ref["accepted"] < ref["outer"]
    got, _ = rx.check(g, gr, "whole run")
    assert got["steps_accepted"] == ref["accepted"] and got["status"] == rr.CONVERGED
    got, _ = rx.check(g, gr, "inside the rejections", max_outer=3)
    assert got["status"] == rr.OUTER_LIMIT and got["steps_accepted"] == 0 and got["cost_after"] == got["cost_before"]
    assert got["lambda"] == 3.0 * (3.0 * (3.0 * rr.DEFAULTS["lambda_init"]))
    R, t = rr.poses_of(gr["pose0"])
    assert got["pose"].tobytes() == rr.rows34(rr.rot_of(rr.quat_of(R)), t).tobytes()
    assert got["edge_cost"].tobytes() == rx.start_costs(gr).tobytes()
    got, _ = rx.check(g, gr, "the first accepted step", max_outer=5)
    assert got["steps_accepted"] == 1 and got["cost_after"] < got["cost_before"]


@pytest.mark.parametrize("max_outer", [1, rx.GROUP - 1, rx.GROUP, rx.GROUP + 1, 2 * rx.GROUP, 2 * rx.GROUP + 1])
def test_outer_limit_inside_at_and_across_a_group(g, max_outer):
    got, _ = rx.check(g, _far_start(0), max_outer, max_outer=max_outer)
    assert got["status"] == rr.OUTER_LIMIT and got["outer_iterations"] == max_outer


def test_every_status(g):
    w = rr.planted_world(30, 6, 5)
    gr = rx.graph(w["odom"], w["node_i"], w["node_j"], w["meas"])
    got, ref = rx.check(g, gr, "converged", step_tol=1e-12, max_outer=40)
    assert got["status"] == rr.CONVERGED and got["steps_accepted"] < got["outer_iterations"]
    # from the optimum no step lowers the cost: the damping climbs past its bound
    at_opt = dict(gr, pose0=ref["pose"])
    got, _ = rx.check(g, at_opt, "damping limit", lambda_init=1.0, lambda_max=2.0)
    assert got["status"] == rr.DAMPING_LIMIT and got["steps_accepted"] == 0 and got["lambda"] == 3.0
    got, _ = rx.check(g, at_opt, "damping limit after three", lambda_init=1e-4, lambda_max=2e-3, max_inner=4, cg_tol=0.5)
    got, _ = rx.check(g, gr, "outer limit", max_outer=2)
    assert got["status"] == rr.OUTER_LIMIT
    got, _ = rx.check(g, dict(gr, fixed=np.ones(30, np.uint8)), "nothing free")
    assert got["status"] == rr.NOTHING_FREE
    # an exact graph (half turns, whole translations): cost 0.0, converged before any iteration
    R = np.array([np.diag(d) for d in ([1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1])])
    t = np.array([[0, 0, 0], [2, 0, 0], [2, 3, 0], [0, 3, 1]], float)
    i, j = [0, 1, 2, 3], [1, 2, 3, 0]
    exact = rx.graph(rr.rows34(R, t), i, j, rx.measure(R, t, i, j, None))
    got, _ = rx.check(g, exact, "exact")
    assert got["status"] == rr.CONVERGED and got["cost_before"] == 0.0 and got["outer_iterations"] == 0
    assert np.array_equal(got["pose"], exact["pose0"])


def test_damping_floor_and_cg_limits(g):
    gr = rx.random_graph(30, 45, 61, weights=True)
    got, _ = rx.check(g, gr, "lambda_min clamps", lambda_init=2e-9)
    got, _ = rx.check(g, gr, "one CG iteration a step", max_inner=1, max_outer=12)
    assert got["cg_iterations"] == got["outer_iterations"]
    got, _ = rx.check(g, gr, "loose CG", cg_tol=0.5)
    tight, _ = rx.check(g, gr, "tight CG", cg_tol=1e-9, max_inner=200)
    assert tight["cg_iterations"] > got["cg_iterations"]
