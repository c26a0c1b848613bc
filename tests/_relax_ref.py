"""numpy restatement of sgtd_relax_poses' rule, written from the comment in include/sgtd_accel.h and from nothing else.
It does not call the library.  Every elementwise numpy operation on float64 arrays (+, -, *, /, sqrt) is one IEEE
rounding, the sums are taken in the header's order, so every number here is the device's to the bit.

Poses are (R, t) pairs of arrays [., 3, 3] and [., 3]; node vectors are [n, 6] (dt, dtheta), element e = 6 * node + a."""
import numpy as np

W = 1024
CONVERGED, OUTER_LIMIT, DAMPING_LIMIT, NOTHING_FREE = 0, 1, 2, 3
DEFAULTS = dict(max_outer=50, max_inner=64, lambda_init=1e-4, lambda_min=1e-9, lambda_max=1e9, cg_tol=1e-4, step_tol=1e-6)


# ---- ordered reductions

def _fold(acc, op):
    s = W // 2
    while s >= 1:
        acc[:s] = op(acc[:s], acc[s:2 * s])
        s //= 2
    return acc[0]


def ordered_sum(v):
    """SUM of the header: W accumulators, element e into accumulator e mod W in ascending e, then the halving tree"""
    v = np.asarray(v, np.float64).reshape(-1)
    rows = -(-v.size // W)
    v = np.concatenate([v, np.zeros(rows * W - v.size)])      # (an accumulator is never -0.0: + 0.0 changes nothing)
    acc = np.zeros(W)
    for r in range(rows):
        acc = acc + v[r * W:(r + 1) * W]
    return _fold(acc, np.add)


def ordered_sum_loop(v):
    """the same, as a plain loop straight from the header's words (slow: for the test of ordered_sum)"""
    acc = [np.float64(0.0)] * W
    for e, x in enumerate(np.asarray(v, np.float64).reshape(-1)):
        acc[e % W] = acc[e % W] + x
    s = W // 2
    while s >= 1:
        for l in range(s):
            acc[l] = acc[l] + acc[l + s]
        s //= 2
    return acc[0]


def ordered_max(v):
    """MAX of the header over non-negative terms: m = v > m ? v : m, from 0.0"""
    v = np.asarray(v, np.float64).reshape(-1)
    rows = -(-v.size // W)
    v = np.concatenate([v, np.zeros(rows * W - v.size)])
    acc = np.zeros(W)
    for r in range(rows):
        x = v[r * W:(r + 1) * W]
        acc = np.where(x > acc, x, acc)
    return _fold(acc, lambda a, b: np.where(b > a, b, a))


def dot(u, v):
    return ordered_sum(u.reshape(-1) * v.reshape(-1))


# ---- poses

def inv(X):
    R, t = X
    Ri = np.swapaxes(R, -1, -2).copy()
    ti = np.stack([-((Ri[..., r, 0] * t[..., 0] + Ri[..., r, 1] * t[..., 1]) + Ri[..., r, 2] * t[..., 2]) for r in range(3)], -1)
    return Ri, ti


def mul(X, Y):
    Xr, Xt = X
    Yr, Yt = Y
    R = np.stack([np.stack([(Xr[..., r, 0] * Yr[..., 0, c] + Xr[..., r, 1] * Yr[..., 1, c]) + Xr[..., r, 2] * Yr[..., 2, c]
                            for c in range(3)], -1) for r in range(3)], -2)
    t = np.stack([((Xr[..., r, 0] * Yt[..., 0] + Xr[..., r, 1] * Yt[..., 1]) + Xr[..., r, 2] * Yt[..., 2]) + Xt[..., r]
                  for r in range(3)], -1)
    return R, t


def quat_of(R):
    """QUAT of the header: [., 3, 3] -> [., 4] (w, x, y, z)"""
    R = np.asarray(R, np.float64)
    r = lambda a, b: R[..., a, b]
    with np.errstate(all="ignore"):
        tr = (r(0, 0) + r(1, 1)) + r(2, 2)
        s = np.sqrt(tr + 1.0) * 2.0
        q0 = np.stack([0.25 * s, (r(2, 1) - r(1, 2)) / s, (r(0, 2) - r(2, 0)) / s, (r(1, 0) - r(0, 1)) / s], -1)
        s = np.sqrt(((1.0 + r(0, 0)) - r(1, 1)) - r(2, 2)) * 2.0
        q1 = np.stack([(r(2, 1) - r(1, 2)) / s, 0.25 * s, (r(0, 1) + r(1, 0)) / s, (r(0, 2) + r(2, 0)) / s], -1)
        s = np.sqrt(((1.0 + r(1, 1)) - r(0, 0)) - r(2, 2)) * 2.0
        q2 = np.stack([(r(0, 2) - r(2, 0)) / s, (r(0, 1) + r(1, 0)) / s, 0.25 * s, (r(1, 2) + r(2, 1)) / s], -1)
        s = np.sqrt(((1.0 + r(2, 2)) - r(0, 0)) - r(1, 1)) * 2.0
        q3 = np.stack([(r(1, 0) - r(0, 1)) / s, (r(0, 2) + r(2, 0)) / s, (r(1, 2) + r(2, 1)) / s, 0.25 * s], -1)
        b0 = (tr > 0.0)[..., None]
        b1 = ((r(0, 0) > r(1, 1)) & (r(0, 0) > r(2, 2)))[..., None]
        b2 = (r(1, 1) > r(2, 2))[..., None]
        q = np.where(b0, q0, np.where(b1, q1, np.where(b2, q2, q3)))
        return unit(q)


def unit(q):
    nn = ((q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]) + q[..., 3] * q[..., 3]
    return q / np.sqrt(nn)[..., None]


def rot_of(q):
    """ROT of the header: [., 4] -> [., 3, 3]"""
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    rows = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
            [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
            [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]
    return np.stack([np.stack(row, -1) for row in rows], -2)


def dot3(M, v, transpose=False):
    """(M v)[r] or (M^T v)[r] = (m0 * v0 + m1 * v1) + m2 * v2"""
    g = (lambda r, k: M[..., k, r]) if transpose else (lambda r, k: M[..., r, k])
    return np.stack([(g(r, 0) * v[..., 0] + g(r, 1) * v[..., 1]) + g(r, 2) * v[..., 2] for r in range(3)], -1)


def sq3(v):
    return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


# ---- the graph

class Graph:
    def __init__(self, n, node_i, node_j, meas, w_trans, w_rot, held):
        self.n, self.m = n, len(node_i)
        self.i, self.j = np.asarray(node_i, np.int64), np.asarray(node_j, np.int64)
        meas = np.asarray(meas, np.float64).reshape(-1, 12)
        self.IZ = inv((meas[:, :9].reshape(-1, 3, 3).copy(), meas[:, 9:].copy()))
        self.wt = np.ones(self.m) if w_trans is None else np.asarray(w_trans, np.float64)
        self.wr = np.ones(self.m) if w_rot is None else np.asarray(w_rot, np.float64)
        self.held = held
        # node -> incident (edge, side) in ascending edge index; side 0: the node is the edge's i, 1: its j
        node = np.concatenate([self.i, self.j])
        edge = np.concatenate([np.arange(self.m), np.arange(self.m)])
        side = np.concatenate([np.zeros(self.m, np.int64), np.ones(self.m, np.int64)])
        order = np.lexsort((edge, node))
        self.e_node, self.e_edge, self.e_side = node[order], edge[order], side[order]
        start = np.searchsorted(self.e_node, np.arange(n))
        self.e_rank = np.arange(2 * self.m) - start[self.e_node]
        self.max_deg = int(self.e_rank.max()) + 1 if self.m else 0

    def evaluate(self, q, t, R):
        """-> dict(rt, rR, ER, DR, u, ec [m, 2], c [m])"""
        D = mul(inv((R[self.i], t[self.i])), (R[self.j], t[self.j]))
        E = mul(self.IZ, D)
        qe = quat_of(E[0])
        v = np.where((qe[:, 0] < 0.0)[:, None], -qe[:, 1:], qe[:, 1:])
        rR = 2.0 * v
        ec = np.stack([self.wt * sq3(E[1]), self.wr * sq3(rR)], -1)
        return dict(rt=E[1], rR=rR, ER=E[0], DR=D[0], u=D[1], ec=ec, c=ec[:, 0] + ec[:, 1])

    def linearise(self, ev):
        A, u = self.IZ[0], ev["u"]
        B = np.stack([np.stack([A[:, r, 1] * u[:, 2] - A[:, r, 2] * u[:, 1],
                                A[:, r, 2] * u[:, 0] - A[:, r, 0] * u[:, 2],
                                A[:, r, 0] * u[:, 1] - A[:, r, 1] * u[:, 0]], -1) for r in range(3)], -2)
        return dict(A=A, B=B, ER=ev["ER"], DR=ev["DR"])

    def gather(self, lin, yt, yR):
        """J^T y per node, the incident edges in ascending index; a held node gets 0"""
        ci = np.concatenate([-dot3(lin["A"], yt, True), dot3(lin["B"], yt, True) - dot3(lin["DR"], yR)], -1)
        cj = np.concatenate([dot3(lin["ER"], yt, True), yR], -1)
        con = np.where((self.e_side == 0)[:, None], ci[self.e_edge], cj[self.e_edge])
        out = np.zeros((self.n, 6))
        for d in range(self.max_deg):
            idx = np.flatnonzero(self.e_rank == d)
            out[self.e_node[idx]] = out[self.e_node[idx]] + con[idx]
        out[self.held] = 0.0
        return out

    def blocks(self, lin):
        """H_nn [n, 6, 6]: sum over the incident edges (ascending) and the residual rows r (ascending) of
        (w_r * J[r][a]) * J[r][b]"""
        m = self.m
        Ji = np.zeros((m, 6, 6))
        Ji[:, :3, :3] = -lin["A"]
        Ji[:, :3, 3:] = lin["B"]
        Ji[:, 3:, 3:] = -np.swapaxes(lin["DR"], -1, -2)
        Jj = np.zeros((m, 6, 6))
        Jj[:, :3, :3] = lin["ER"]
        Jj[:, 3:, 3:] = np.eye(3)
        J = np.where((self.e_side == 0)[:, None, None], Ji[self.e_edge], Jj[self.e_edge])
        w6 = np.concatenate([np.repeat(self.wt[:, None], 3, 1), np.repeat(self.wr[:, None], 3, 1)], 1)[self.e_edge]
        H = np.zeros((self.n, 6, 6))
        for d in range(self.max_deg):
            idx = np.flatnonzero(self.e_rank == d)
            nd = self.e_node[idx]
            for r in range(6):
                H[nd] = H[nd] + (w6[idx, r, None, None] * J[idx, r, :, None]) * J[idx, r, None, :]
        H[self.held] = 0.0
        return H

    def apply(self, lin, H, lam, p):
        """(H + lam * diag-blocks(H)) p, matrix-free"""
        a, b, c, d = p[self.i, :3], p[self.i, 3:], p[self.j, :3], p[self.j, 3:]
        et = (dot3(lin["B"], b) - dot3(lin["A"], a)) + dot3(lin["ER"], c)
        eR = d - dot3(lin["DR"], b, True)
        g = self.gather(lin, self.wt[:, None] * et, self.wr[:, None] * eR)
        hp = np.stack([((((H[:, a_, 0] * p[:, 0] + H[:, a_, 1] * p[:, 1]) + H[:, a_, 2] * p[:, 2]) + H[:, a_, 3] * p[:, 3])
                        + H[:, a_, 4] * p[:, 4]) + H[:, a_, 5] * p[:, 5] for a_ in range(6)], -1)
        out = g + lam * hp
        out[self.held] = 0.0
        return out


def cholesky(M):
    """-> (L, ok): column by column; ok = every pivot > 0"""
    n = M.shape[0]
    L = np.zeros_like(M)
    ok = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for c in range(6):
            s = M[:, c, c].copy()
            for k in range(c):
                s = s - L[:, c, k] * L[:, c, k]
            ok &= s > 0.0
            L[:, c, c] = np.sqrt(s)
            for r in range(c + 1, 6):
                s = M[:, r, c].copy()
                for k in range(c):
                    s = s - L[:, r, k] * L[:, c, k]
                L[:, r, c] = s / L[:, c, c]
    return L, ok


def solve(L, ok, r):
    """z = M^-1 r by the two triangular solves; 0 where ok is false"""
    y = np.zeros_like(r)
    z = np.zeros_like(r)
    with np.errstate(all="ignore"):
        for a in range(6):
            s = r[:, a].copy()
            for k in range(a):
                s = s - L[:, a, k] * y[:, k]
            y[:, a] = s / L[:, a, a]
        for a in range(5, -1, -1):
            s = y[:, a].copy()
            for k in range(a + 1, 6):
                s = s - L[:, k, a] * z[:, k]
            z[:, a] = s / L[:, a, a]
    z[~ok] = 0.0
    return z


def retract(q, t, R, x, move):
    """the trial state: nodes of `move` by the header's update, the others unchanged"""
    dt, h = x[:, :3], 0.5 * x[:, 3:]
    t2 = dot3(R, dt) + t
    w, a, b, c = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    q2 = np.stack([((w - a * h[:, 0]) - b * h[:, 1]) - c * h[:, 2],
                   ((a + w * h[:, 0]) + b * h[:, 2]) - c * h[:, 1],
                   ((b + w * h[:, 1]) + c * h[:, 0]) - a * h[:, 2],
                   ((c + w * h[:, 2]) + a * h[:, 1]) - b * h[:, 0]], -1)
    q2 = unit(q2)
    m = move[:, None]
    q2 = np.where(m, q2, q)
    return q2, np.where(m, t2, t), np.where(m[:, :, None], rot_of(q2), R)


def relax(pose0, fixed, node_i, node_j, meas, w_trans=None, w_rot=None, opt=None, trace=None):
    """the whole rule -> dict(pose [n, 12], edge_cost [m, 2], cost_before, cost_after, outer, accepted, cg, lam, status).
    trace: a list that receives one dict per outer iteration (accepted, cost, cost_new, lam, cg, maxd)"""
    o = dict(DEFAULTS)
    o.update(opt or {})
    pose0 = np.asarray(pose0, np.float64).reshape(-1, 3, 4)
    n, m = pose0.shape[0], len(node_i)
    lam = np.float64(o["lambda_init"])
    if n == 0 or m == 0:
        return dict(pose=np.zeros((0, 12)), edge_cost=np.zeros((0, 2)), cost_before=0.0, cost_after=0.0, outer=0, accepted=0,
                    cg=0, lam=float(lam), status=NOTHING_FREE)
    held = (np.arange(n) == 0) if fixed is None else np.asarray(fixed).astype(bool)
    G = Graph(n, node_i, node_j, meas, w_trans, w_rot, held)
    q = quat_of(pose0[:, :, :3])
    t = pose0[:, :, 3].copy()
    R = rot_of(q)
    ev = G.evaluate(q, t, R)
    cost = cost_before = ordered_sum(ev["c"])
    outer = accepted = cg_total = 0
    status = None
    if held.all():
        status = NOTHING_FREE
    tol2 = np.float64(o["cg_tol"]) * np.float64(o["cg_tol"])
    while status is None:
        lin = G.linearise(ev)
        g = G.gather(lin, G.wt[:, None] * ev["rt"], G.wr[:, None] * ev["rR"])
        H = G.blocks(lin)
        L, ok = cholesky(H + lam * H)
        ok &= ~held
        r = np.where(held[:, None], 0.0, -g)
        x = np.zeros((n, 6))
        p = np.zeros((n, 6))
        z = solve(L, ok, r)
        rz = rz0 = dot(r, z)
        if not rz0 > 0.0:
            status = CONVERGED
            break
        thr = tol2 * rz0
        beta = np.float64(0.0)
        cg = 0
        for _ in range(int(o["max_inner"])):
            p = z + beta * p
            ap = G.apply(lin, H, lam, p)
            pq = dot(p, ap)
            if not pq > 0.0:
                break
            alpha = rz / pq
            x = x + alpha * p
            r = r - alpha * ap
            z = solve(L, ok, r)
            rz_new = dot(r, z)
            cg += 1
            if rz_new <= thr:
                break
            beta = rz_new / rz
            rz = rz_new
        cg_total += cg
        q2, t2, R2 = retract(q, t, R, x, ok)
        ev2 = G.evaluate(q2, t2, R2)
        cost_new = ordered_sum(ev2["c"])
        maxd = ordered_max(np.abs(x))
        acc = bool(cost_new < cost)
        if trace is not None:
            trace.append(dict(accepted=acc, cost=float(cost), cost_new=float(cost_new), lam=float(lam), cg=cg, maxd=float(maxd)))
        outer += 1
        if acc:
            q, t, R, ev, cost = q2, t2, R2, ev2, cost_new
            accepted += 1
            lam = max(lam / 3.0, np.float64(o["lambda_min"]))
            if maxd <= o["step_tol"]:
                status = CONVERGED
        else:
            lam = 3.0 * lam
            if lam > o["lambda_max"]:
                status = DAMPING_LIMIT
        if status is None and outer >= int(o["max_outer"]):
            status = OUTER_LIMIT
    pose = np.concatenate([R, t[:, :, None]], 2).reshape(n, 12)
    return dict(pose=pose, edge_cost=ev["ec"], cost_before=float(cost_before), cost_after=float(cost), outer=outer,
                accepted=accepted, cg=cg_total, lam=float(lam), status=status)


# ---- the residual as a plain function (for the independent check) and planted worlds

def poses_of(pose12):
    p = np.asarray(pose12, np.float64).reshape(-1, 3, 4)
    return p[:, :, :3].copy(), p[:, :, 3].copy()


def rows34(R, t):
    return np.concatenate([R, t[:, :, None]], 2).reshape(-1, 12)


def rel_rows(R, t):
    return np.concatenate([R.reshape(-1, 9), t], 1)


def rot_vec(v):
    """Rodrigues' formula (world making only; not part of the rule)"""
    v = np.asarray(v, np.float64)
    a = np.linalg.norm(v)
    if a == 0.0:
        return np.eye(3)
    k = v / a
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def planted_world(n, n_loops, seed, step=0.5, odo_t=0.02, odo_r=np.deg2rad(0.4), loop_t=0.005, loop_r=np.deg2rad(0.05), gap=8):
    """a ground-truth walk of n frames, its dead-reckoned odometry (every step's noise accumulates into drift), and
    n_loops loops between frames at least `gap` apart measured almost exactly.
    -> dict(truth, odom: (n, 12) rows; node_i, node_j, meas: the odometry edges then the loops in the sgtd_relax_poses
    orientation (loop (a, b, T): i = b, j = a, Z = T = inv(X_b) X_a); n_odo)"""
    rng = np.random.default_rng(seed)
    Rg, tg = [np.eye(3)], [np.zeros(3)]
    rel = []
    for k in range(1, n):
        dR = rot_vec([0.0, 0.0, rng.normal(0.0, 0.15)] + rng.normal(0.0, 0.01, 3))
        dt = np.array([step, 0.0, 0.0]) + rng.normal(0.0, 0.02, 3)
        rel.append((dR, dt))
        Rg.append(Rg[-1] @ dR)
        tg.append(Rg[-2] @ dt + tg[-1])
    Ro, to = [np.eye(3)], [np.zeros(3)]
    for dR, dt in rel:
        nR = dR @ rot_vec(rng.normal(0.0, odo_r, 3))
        nt = dt + rng.normal(0.0, odo_t, 3)
        Ro.append(Ro[-1] @ nR)
        to.append(Ro[-2] @ nt + to[-1])
    Rg, tg, Ro, to = map(np.array, (Rg, tg, Ro, to))
    ni, nj, Z = [], [], []
    for k in range(n - 1):                       # odometry: Z = inv(A_k) A_{k+1}
        ni.append(k)
        nj.append(k + 1)
        Z.append(np.concatenate([(Ro[k].T @ Ro[k + 1]).reshape(9), Ro[k].T @ (to[k + 1] - to[k])]))
    loops = 0
    while loops < n_loops:
        a, b = sorted(rng.integers(0, n, 2))
        if b - a < gap:
            continue

        Rt = Rg[a].T @ Rg[b] @ rot_vec(rng.normal(0.0, loop_r, 3))
        tt = Rg[a].T @ (tg[b] - tg[a]) + rng.normal(0.0, loop_t, 3)
        ni.append(a)
        nj.append(b)
        Z.append(np.concatenate([Rt.reshape(9), tt]))
        loops += 1
    return dict(truth=rows34(Rg, tg), odom=rows34(Ro, to), node_i=np.array(ni, np.int32), node_j=np.array(nj, np.int32),
                meas=np.array(Z), n_odo=n - 1)


def mean_trans_error(pose, truth):
    return float(np.mean(np.linalg.norm(poses_of(pose)[1] - poses_of(truth)[1], axis=1)))


def residuals_of(params, pose0, held, node_i, node_j, meas, w_trans, w_rot):
    """sqrt(w) * (r_t, r_R) of every edge, the free nodes moved from pose0 by the header's update with `params`
    [n_free * 6] (for scipy.optimize.least_squares: half its cost is not the rule's; the caller sums squares)"""
    pose0 = np.asarray(pose0, np.float64).reshape(-1, 3, 4)
    n = pose0.shape[0]
    x = np.zeros((n, 6))
    x[~held] = np.asarray(params).reshape(-1, 6)
    q = quat_of(pose0[:, :, :3])
    t = pose0[:, :, 3].copy()
    q2, t2, R2 = retract(q, t, rot_of(q), x, ~held)
    G = Graph(n, node_i, node_j, meas, w_trans, w_rot, held)
    ev = G.evaluate(q2, t2, R2)
    return np.concatenate([np.sqrt(G.wt)[:, None] * ev["rt"], np.sqrt(G.wr)[:, None] * ev["rR"]], 1).reshape(-1)
