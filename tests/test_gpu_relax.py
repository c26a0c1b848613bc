"""sgtd_relax_poses on the device against the numpy restatement of the rule in include/sgtd_accel.h (tests/_relax_ref.py):
the poses, the report and the per-edge costs are compared bit for bit (the rule uses +, -, *, / and sqrt only, each rounded
once on both sides, in one stated order).  The handles here need no table."""
import ctypes as C

import numpy as np
import pytest

import _relax_edges as rx
import _relax_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, evaluate, manager, synth
    return manager, synth, _lib, evaluate


@pytest.fixture(scope="module")
def g(mods):
    h = mods[0].STDescManager()
    yield h
    h.close()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(h, _lib, gr, opt=None, n=None, m=None, report=True, **swap):
    """the C call itself: -> (status, report); swap replaces an argument (None = a NULL pointer)"""
    a = dict(pose0=gr["pose0"], fixed=gr["fixed"], node_i=gr["node_i"], node_j=gr["node_j"], meas=gr["meas"],
             w_trans=gr["w_trans"], w_rot=gr["w_rot"])
    a.update(swap)
    rep = _lib.RelaxReport()
    st = h._L.sgtd_relax_poses(h._h, gr["pose0"].shape[0] if n is None else n, _ptr(a["pose0"]), _ptr(a["fixed"]),
                               gr["node_i"].size if m is None else m, _ptr(a["node_i"]), _ptr(a["node_j"]), _ptr(a["meas"]),
                               _ptr(a["w_trans"]), _ptr(a["w_rot"]), None if opt is None else C.byref(opt),
                               C.byref(rep) if report else None)
    return st, rep


def _fetch(h, n, m):
    pose, cost = np.zeros((n, 12)), np.zeros((m, 2))
    st = h._L.sgtd_result_relaxed(h._h, _ptr(pose), _ptr(cost))
    return st, pose, cost


# ---- basic shapes ----
def test_two_nodes_one_edge(g):
    got, ref = rx.check(g, rx.random_graph(2, 1, 1))
    assert got["status"] == rr.CONVERGED and got["cost_after"] < 1e-20 < got["cost_before"]
    # one edge determines the free node: it sits at X_0 Z
    gr = rx.random_graph(2, 1, 1)
    R0, t0 = rr.poses_of(got["pose"][:1])
    Z = gr["meas"][0]
    assert np.allclose(rr.poses_of(got["pose"][1:])[0][0], R0[0] @ Z[:9].reshape(3, 3), atol=1e-9)
    assert np.allclose(rr.poses_of(got["pose"][1:])[1][0], R0[0] @ Z[9:] + t0[0], atol=1e-9)


def test_chain_with_a_loop_and_weights(g):
    rx.check(g, rx.random_graph(3, 3, 2), "3 nodes")
    gr = rx.random_graph(12, 20, 3)
    a, _ = rx.check(g, gr, "weights NULL")
    ones = dict(gr, w_trans=np.ones(20), w_rot=np.ones(20))
    b, _ = rx.check(g, ones, "weights of 1.0")
    assert a["pose"].tobytes() == b["pose"].tobytes() and a["cost_after"] == b["cost_after"]
    c, _ = rx.check(g, rx.random_graph(12, 20, 3, weights=True), "weights given")
    assert c["pose"].tobytes() != a["pose"].tobytes()


def test_fixed_null_is_node_zero_held(g):
    gr = rx.random_graph(9, 12, 5)
    a, _ = rx.check(g, gr, "fixed NULL")
    first = np.zeros(9, np.uint8)
    first[0] = 1
    b, _ = rx.check(g, dict(gr, fixed=first), "node 0 held")
    assert a["pose"].tobytes() == b["pose"].tobytes()
    other = np.zeros(9, np.uint8)
    other[[2, 7]] = 1
    c, ref = rx.check(g, dict(gr, fixed=other), "nodes 2 and 7 held")
    start = rr.rot_of(rr.quat_of(rr.poses_of(gr["pose0"])[0]))
    assert np.array_equal(rr.poses_of(c["pose"])[0][[2, 7]], start[[2, 7]])
    assert np.array_equal(c["pose"][[2, 7]][:, [3, 7, 11]], gr["pose0"][[2, 7]][:, [3, 7, 11]])
    assert not np.array_equal(c["pose"][0], a["pose"][0])


def test_everything_held_and_empty_graphs(g, mods):
    gr = rx.random_graph(4, 5, 8, fixed=np.ones(4, np.uint8))
    got, _ = rx.check(g, gr, "all held")
    assert got["status"] == rr.NOTHING_FREE and got["cost_before"] == got["cost_after"] > 0 and got["outer_iterations"] == 0
    assert (got["edge_cost"].sum(1) > 0).all()
    one = rx.random_graph(2, 1, 1)
    got, _ = rx.check(g, rx.graph(one["pose0"][:1], [], [], np.zeros((0, 12))), "one node, no edge")
    for gr in (rx.graph(np.zeros((0, 12)), [], [], np.zeros((0, 12))), rx.graph(one["pose0"], [], [], np.zeros((0, 12)))):
        got, _ = rx.check(g, gr, "empty")
        assert got["status"] == rr.NOTHING_FREE and got["cost_before"] == 0.0 and got["lambda"] == rr.DEFAULTS["lambda_init"]
    # after an empty run the result call writes nothing
    st, pose, cost = _fetch(g, 2, 1)
    assert st == 0 and not pose.any() and not cost.any()


def test_isolated_free_node_stays_put(g):
    gr = rx.random_graph(5, 6, 13)
    lone = rx.graph(np.concatenate([gr["pose0"], gr["pose0"][2:3]]), gr["node_i"], gr["node_j"], gr["meas"])
    got, _ = rx.check(g, lone)
    base, _ = rx.check(g, gr)
    R, t = rr.poses_of(lone["pose0"])
    assert np.array_equal(got["pose"][5], rr.rows34(rr.rot_of(rr.quat_of(R)), t)[5])
    assert got["pose"][:5].tobytes() == base["pose"].tobytes() and got["cost_after"] < got["cost_before"]


def test_zero_weight_and_duplicate_edges(g):
    gr = rx.random_graph(6, 9, 17)
    base, _ = rx.check(g, gr)
    zero = rx.graph(gr["pose0"], list(gr["node_i"]) + [0], list(gr["node_j"]) + [5], np.concatenate([gr["meas"], gr["meas"][:1]]),
                    w_trans=np.array([1.0] * 9 + [0.0]), w_rot=np.array([1.0] * 9 + [0.0]))
    got, _ = rx.check(g, zero, "zero weight")
    assert (got["edge_cost"][9] == 0.0).all() and np.allclose(got["pose"], base["pose"], atol=1e-9)
    # a node whose edges all weigh nothing is as good as isolated
    touching = (gr["node_i"] == 5) | (gr["node_j"] == 5)
    w = np.where(touching, 0.0, 1.0)
    got, _ = rx.check(g, dict(gr, w_trans=w, w_rot=w), "node 5 weightless")
    R, t = rr.poses_of(gr["pose0"])
    assert np.array_equal(got["pose"][5], rr.rows34(rr.rot_of(rr.quat_of(R)), t)[5])
    # every edge twice: the same optimum as weights of 2, and the order of the copies is part of the rule
    dup = rx.graph(gr["pose0"], np.tile(gr["node_i"], 2), np.tile(gr["node_j"], 2), np.tile(gr["meas"], (2, 1)))
    got, _ = rx.check(g, dup, "duplicates")
    two, _ = rx.check(g, dict(gr, w_trans=np.full(9, 2.0), w_rot=np.full(9, 2.0)), "weights of 2")
    assert np.allclose(got["pose"], two["pose"], atol=1e-9) and np.isclose(got["cost_after"], two["cost_after"], rtol=1e-9)


def test_planted_worlds(g, mods):
    """the two uses of the header: a session closed against itself, and one against a held map"""
    w = rr.planted_world(60, 12, 3)
    got, _ = rx.check(g, rx.graph(w["odom"], w["node_i"], w["node_j"], w["meas"]), "self-closed")
    assert got["status"] == rr.CONVERGED
    assert rr.mean_trans_error(got["pose"], w["truth"]) < 0.2 * rr.mean_trans_error(w["odom"], w["truth"])
    w = rr.planted_world(40, 10, 11, odo_t=0.04, odo_r=np.deg2rad(1.2))
    places = np.arange(0, 40, 4)
    rng = np.random.default_rng(77)
    rel = np.array([np.concatenate([rr.rot_vec(rng.normal(0.0, 1e-3, 3)).reshape(9), rng.normal(0.0, 0.005, 3)]) for _ in places])
    # the map numbers its frames as the session does: the ids overlap, the nodes do not
    edges = dict(frame_a=places.astype(np.uint32), frame_b=places.astype(np.uint32), rel_pose=rel)
    res = g.relax_session(np.arange(40), w["odom"], edges, None, held=(places, w["truth"][places]))
    assert res["graph"]["fixed"].tolist() == [0] * 40 + [1] * 10 and res["graph"]["node_i"][39:].tolist() == list(range(40, 50))
    rx.same(res, rx.reference(res["graph"]), "against a map")
    assert res["status"] == rr.CONVERGED and sorted(res["poses"]) == list(range(40))
    assert rr.mean_trans_error(res["pose"][:40], w["truth"]) < 0.2 * rr.mean_trans_error(res["graph"]["pose0"][:40], w["truth"])


# ---- the calls ----
def test_invalid_arguments_keep_the_earlier_results(g, mods):
    _lib = mods[2]
    gr = rx.random_graph(6, 9, 17, weights=True)
    gr["fixed"] = np.array([1, 0, 0, 0, 0, 0], np.uint8)
    base = rx.run(g, gr)

    def kept():
        st, pose, cost = _fetch(g, 6, 9)
        assert st == 0 and pose.tobytes() == base["pose"].tobytes() and cost.tobytes() == base["edge_cost"].tobytes()

    def bad(v, k, x):
        v = v.copy()
        v.reshape(-1)[k] = x
        return v

    cases = [dict(n=-1), dict(m=-1), dict(pose0=None), dict(node_i=None), dict(node_j=None), dict(meas=None),
             dict(node_i=bad(gr["node_i"], 3, 6)), dict(node_j=bad(gr["node_j"], 0, -1)), dict(node_j=bad(gr["node_j"], 2, gr["node_i"][2])),
             dict(pose0=bad(gr["pose0"], 17, np.nan)), dict(pose0=bad(gr["pose0"], 3, np.inf)), dict(meas=bad(gr["meas"], 40, -np.inf)),
             dict(w_trans=bad(gr["w_trans"], 1, np.nan)), dict(w_rot=bad(gr["w_rot"], 8, np.inf)),
             dict(w_trans=bad(gr["w_trans"], 0, -1e-300)), dict(w_rot=bad(gr["w_rot"], 5, -1.0))]
    for c in cases:
        st, _ = _raw(g, _lib, gr, **c)
        assert st == -1, c
        kept()
    for field, value in (("max_outer", 0), ("max_outer", -3), ("max_inner", 0), ("lambda_init", 0.0), ("lambda_init", np.nan),
                         ("lambda_min", -1.0), ("lambda_max", np.inf), ("lambda_max", 0.0), ("cg_tol", 0.0), ("cg_tol", -1e-3),
                         ("step_tol", 0.0), ("step_tol", np.nan)):
        o = _lib.RelaxOptions()
        g._L.sgtd_default_relax_options(C.byref(o))
        setattr(o, field, value)
        st, _ = _raw(g, _lib, gr, opt=o)
        assert st == -1, (field, value)
        kept()
    assert g._L.sgtd_relax_poses(None, 0, None, None, 0, None, None, None, None, None, None, None) == -1
    assert g._L.sgtd_result_relaxed(None, None, None) == -1
    kept()
    # NULL options are the defaults, a NULL report is allowed, either result array may be NULL
    st, rep = _raw(g, _lib, gr)
    assert st == 0 and rep.cost_after == base["cost_after"] and rep.status == base["status"]
    st, _ = _raw(g, _lib, gr, report=False)
    assert st == 0
    assert g._L.sgtd_result_relaxed(g._h, None, None) == 0
    kept()


def test_results_before_a_run_are_a_state_error(mods):
    manager, _, _lib, _ = mods
    h = manager.STDescManager()
    try:
        st, _, _ = _fetch(h, 1, 1)
        assert st == -7 and b"sgtd_relax_poses" in h._L.sgtd_last_error(h._h)
        gr = rx.random_graph(3, 3, 2)
        st, _ = _raw(h, _lib, gr, node_i=np.array([0, 1, 9], np.int32))
        assert st == -1 and _fetch(h, 3, 3)[0] == -7
        rx.check(h, gr)
    finally:
        h.close()


def test_second_call_reuses_the_buffers(g):
    big, small = rx.random_graph(300, 420, 31), rx.random_graph(7, 9, 32)
    opt = dict(max_outer=3, max_inner=10)
    a, _ = rx.check(g, big, "big", **opt)
    allocs = g.stats()["device_allocs_total"]
    b, _ = rx.check(g, small, "small after big")
    c, _ = rx.check(g, big, "big again", **opt)
    assert g.stats()["device_allocs_total"] == allocs
    assert a["pose"].tobytes() == c["pose"].tobytes() and a["edge_cost"].tobytes() == c["edge_cost"].tobytes()


def test_view_and_single_device_group(mods, g):
    manager, synth, _lib, _ = mods
    gr = rx.random_graph(40, 60, 41)
    base, ref = rx.check(g, gr)
    m = synth.make_map(16, 120, stream=3)
    owner, view = manager.STDescManager(), manager.STDescManager()
    grp = manager.STDescManager(devices=[0])
    try:
        owner.add_frames(m.xyz[:8], m.label[:8])
        owner.finalize()
        view.attach_table(owner)
        owner.add_frames(m.xyz[8:], m.label[8:])           # the owner's table changes: the view's table calls are STATE now
        with pytest.raises(_lib.SgtdError) as ei:
            view.query_frames(m.xyz[:1], m.label[:1])
        assert ei.value.status == -7
        rx.same(rx.run(view, gr), ref, "view")
        rx.same(rx.run(owner, gr), ref, "owner")
        rx.same(rx.run(grp, gr), ref, "group of one device")
        st, pose, cost = _fetch(grp, 40, 60)
        assert st == 0 and pose.tobytes() == base["pose"].tobytes() and cost.tobytes() == base["edge_cost"].tobytes()
    finally:
        view.close()
        owner.close()
        grp.close()


def test_the_pending_batch_is_untouched(mods):
    """the call is independent of the batch: the candidates and the verification of a pending batch read the same after"""
    manager, synth, _lib, _ = mods
    m = synth.make_map(24, 120, stream=3)
    qs = synth.make_queries(m, 3, stream=3)
    h = manager.STDescManager()
    try:
        h.add_frames(m.xyz, m.label)
        res = h.query_frames(qs.xyz, qs.label)
        h.verify()
        before = [h.result_verify(q) for q in range(3)]
        rx.check(h, rx.random_graph(12, 20, 3))
        after = [h.result_verify(q) for q in range(3)]
        for b, a in zip(before, after):
            assert all(np.array_equal(x, y) for x, y in zip(b, a))
        again = h.results()
        assert np.array_equal(again.cand_frame, res.cand_frame) and np.array_equal(again.cand_votes, res.cand_votes)
    finally:
        h.close()


# ---- end to end ----
def test_loop_session_end_to_end(mods):
    """a closed session of 120 frames 4 m apart (synth's trajectory runs out along an arc and back over it): its odometry
    is the truth with every step's motion disturbed (5 mm, 0.02 degrees a step: over the 60 steps between a loop's frames
    some 4 cm and 0.15 degrees of walk, the rotation over a lever arm of up to 100 m some 0.3 m), so the loops stay
    mutually consistent within 2 m and 5 degrees while the odometry disagrees with them by far more than their refined
    poses' own error (millimetres): relaxing must lower the cost.  loop_frames -> verify -> refine_poses ->
    loop_edges(refined) -> consistent_loops -> relax_session, against the restatement fed the same graph."""
    manager, synth, _lib, ev = mods
    F = 120
    m = synth.make_map(F, 200, stream=431, spacing=4.0)
    truth = np.stack([ev.pose_row(*p) for p in m.pose]).astype(np.float64)
    Rg, tg = rr.poses_of(truth)
    rng = np.random.default_rng(12)
    Ro, to = [Rg[0]], [tg[0]]
    for k in range(F - 1):
        dR = Rg[k].T @ Rg[k + 1] @ rr.rot_vec(rng.normal(0.0, np.deg2rad(0.02), 3))
        dt = Rg[k].T @ (tg[k + 1] - tg[k]) + rng.normal(0.0, 0.005, 3)
        Ro.append(Ro[-1] @ dR)
        to.append(Ro[-2] @ dt + to[-1])
    odom = rr.rows34(np.array(Ro), np.array(to))
    h = manager.STDescManager()
    try:
        h.set_frame_poses(np.arange(F), odom.astype(np.float32))
        h.loop_frames(m.xyz, m.label, skip_near=30, batch=F)
        h.verify()
        h.refine_poses(1)
        e = h.loop_edges(refined=True)
        assert e["query"].size >= 3
        cons = h.consistent_loops(e["frame_a"], e["frame_b"], e["rel_pose"], 2.0, np.deg2rad(5.0))
        assert cons["n_set"] >= 3
        res = h.relax_session(np.arange(F), odom, e, cons["in_set"])
        gr = res["graph"]
        assert gr["node_i"].size == F - 1 + cons["n_set"] and gr["fixed"].tolist() == [1] + [0] * (F - 1)
        rx.same(res, rx.reference(gr), "session")
        assert res["cost_after"] < res["cost_before"]
        assert sorted(res["poses"]) == list(range(F)) and np.array_equal(res["poses"][7], res["pose"][7])
        # the chosen loops fit the relaxed trajectory better than they fit the odometry
        loops = slice(F - 1, None)
        assert res["edge_cost"][loops].sum() < rx.start_costs(gr)[loops].sum()
    finally:
        h.close()
