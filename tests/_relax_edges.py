"""Graphs for the sgtd_relax_poses tests and the exact comparison of a device run with the restatement
(tests/_relax_ref.py).  Every graph is a dict(pose0, fixed, node_i, node_j, meas, w_trans, w_rot) as relax_poses takes it."""
import numpy as np

import _relax_ref as rr

THREADS = 256        # SGTD_RELAX_THREADS
GROUP = 4            # SGTD_RELAX_GROUP
W = rr.W

REPORT = (("cost_before", "cost_before"), ("cost_after", "cost_after"), ("lambda", "lam"), ("outer_iterations", "outer"),
          ("steps_accepted", "accepted"), ("cg_iterations", "cg"), ("status", "status"))


def graph(pose0, node_i, node_j, meas, fixed=None, w_trans=None, w_rot=None):
    return dict(pose0=np.ascontiguousarray(pose0, np.float64).reshape(-1, 12), fixed=fixed,
                node_i=np.asarray(node_i, np.int32), node_j=np.asarray(node_j, np.int32),
                meas=np.ascontiguousarray(meas, np.float64).reshape(-1, 12), w_trans=w_trans, w_rot=w_rot)


def random_poses(n, rng, spread=5.0, angle=1.0):
    R = np.array([rr.rot_vec(rng.normal(0.0, angle, 3)) for _ in range(n)]).reshape(n, 3, 3)
    return R, rng.normal(0.0, spread, (n, 3))


def measure(R, t, i, j, rng, noise_t=0.0, noise_r=0.0):
    """Z = inv(X_i) X_j, with noise"""
    out = []
    for a, b in zip(i, j):
        Rz = R[a].T @ R[b] @ rr.rot_vec(rng.normal(0.0, noise_r, 3) if noise_r else np.zeros(3))
        tz = R[a].T @ (t[b] - t[a]) + (rng.normal(0.0, noise_t, 3) if noise_t else 0.0)
        out.append(np.concatenate([Rz.reshape(9), tz]))
    return np.array(out).reshape(-1, 12)


def perturbed(R, t, rng, dt=0.1, dr=0.03):
    n = R.shape[0]
    R2 = np.array([R[k] @ rr.rot_vec(rng.normal(0.0, dr, 3)) for k in range(n)]).reshape(n, 3, 3)
    return rr.rows34(R2, t + rng.normal(0.0, dt, (n, 3)))


def random_graph(n, m, seed, fixed=None, noise=True, weights=False, extra_chain=True):
    """n nodes, a chain through all of them (so nothing is isolated) topped up to m edges between random pairs, the start a
    perturbed truth"""
    rng = np.random.default_rng(seed)
    R, t = random_poses(n, rng)
    i = list(range(n - 1)) if extra_chain else []
    j = list(range(1, n)) if extra_chain else []
    while len(i) < m:
        a, b = rng.integers(0, n, 2)
        if a != b:
            i.append(int(a))
            j.append(int(b))
    i, j = i[:m], j[:m]
    Z = measure(R, t, i, j, rng, 0.01 if noise else 0.0, 0.002 if noise else 0.0)
    p0 = perturbed(R, t, rng) if noise else rr.rows34(R, t)
    wt = rng.uniform(0.5, 4.0, m) if weights else None
    wr = rng.uniform(0.5, 40.0, m) if weights else None
    return graph(p0, i, j, Z, fixed, wt, wr)


def star(degree, seed, hub_as_i=None):
    """a free hub (node 0) with `degree` edges to held leaves; the hub is the edge's i or j by turns"""
    rng = np.random.default_rng(seed)
    n = degree + 1
    R, t = random_poses(n, rng)
    i = [0 if k % 2 == 0 else k + 1 for k in range(degree)]
    j = [k + 1 if k % 2 == 0 else 0 for k in range(degree)]
    Z = measure(R, t, i, j, rng, 0.02, 0.004)
    p0 = rr.rows34(R, t)
    p0[0] = perturbed(R[:1], t[:1], rng, 0.5, 0.2)[0]
    fixed = np.ones(n, np.uint8)
    fixed[0] = 0
    return graph(p0, i, j, Z, fixed)


def reference(g, **opt):
    return rr.relax(g["pose0"], g["fixed"], g["node_i"], g["node_j"], g["meas"], g["w_trans"], g["w_rot"], opt or None)


def start_costs(g):
    """the per-edge costs [m, 2] at the start"""
    n = g["pose0"].shape[0]
    held = (np.arange(n) == 0) if g["fixed"] is None else np.asarray(g["fixed"]).astype(bool)
    R, t = rr.poses_of(g["pose0"])
    q = rr.quat_of(R)
    return rr.Graph(n, g["node_i"], g["node_j"], g["meas"], g["w_trans"], g["w_rot"], held).evaluate(q, t, rr.rot_of(q))["ec"]


def run(h, g, **opt):
    return h.relax_poses(g["pose0"], g["node_i"], g["node_j"], g["meas"], g["fixed"], g["w_trans"], g["w_rot"], **opt)


def same(got, ref, where=None):
    """bit for bit: the report, the poses, the per-edge costs"""
    for a, b in REPORT:
        x, y = got[a], ref[b]
        assert (np.float64(x).tobytes() == np.float64(y).tobytes()) if isinstance(y, float) else x == y, (where, a, x, y)
    for k in ("pose", "edge_cost"):
        assert got[k].shape == ref[k].shape, (where, k, got[k].shape, ref[k].shape)
        assert got[k].tobytes() == np.ascontiguousarray(ref[k]).tobytes(), (where, k, float(np.max(np.abs(got[k] - ref[k]))))


def check(h, g, where=None, **opt):
    got, ref = run(h, g, **opt), reference(g, **opt)
    same(got, ref, where)
    assert got["cost_after"] <= got["cost_before"]
    return got, ref
