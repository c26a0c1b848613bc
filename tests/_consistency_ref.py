"""numpy restatement of sgtd_consistent_loops' rule, written from the comment in include/sgtd_accel.h: f64 throughout,
every sum spelled out in the stated order (no dot products, no matrix products), plus the planted worlds the consistency
tests and tools/consistency_bench.py share.

A pose here is (R, t) with R[..., 3, 3] and t[..., 3]; a stored pose or a pose_a row is the row-major 3x4 [R | t] in f32;
a rel_pose row is rot row-major (9), t (3) in f64."""
import numpy as np


def from_rows34(m):
    """(n, 12) row-major 3x4 [R | t] -> (R, t), widened exactly to f64"""
    m = np.asarray(m).astype(np.float64).reshape(-1, 3, 4)
    return m[:, :, :3].copy(), m[:, :, 3].copy()


def from_rel(rel):
    """(n, 12) rot row-major (9), t (3) -> (R, t)"""
    rel = np.asarray(rel, np.float64).reshape(-1, 12)
    return rel[:, :9].reshape(-1, 3, 3).copy(), rel[:, 9:].copy()


def inv(X):
    R, t = X
    Ri = np.empty_like(R)
    for r in range(3):
        for c in range(3):
            Ri[..., r, c] = R[..., c, r]
    ti = np.empty_like(t)
    for r in range(3):
        ti[..., r] = -((Ri[..., r, 0] * t[..., 0] + Ri[..., r, 1] * t[..., 1]) + Ri[..., r, 2] * t[..., 2])
    return Ri, ti


def mul(X, Y):
    Xr, Xt = X
    Yr, Yt = Y
    shape = np.broadcast(Xr, Yr).shape
    R = np.empty(shape, np.float64)
    t = np.empty(shape[:-1], np.float64)
    for r in range(3):
        for c in range(3):
            R[..., r, c] = (Xr[..., r, 0] * Yr[..., 0, c] + Xr[..., r, 1] * Yr[..., 1, c]) + Xr[..., r, 2] * Yr[..., 2, c]
        t[..., r] = ((Xr[..., r, 0] * Yt[..., 0] + Xr[..., r, 1] * Yt[..., 1]) + Xr[..., r, 2] * Yt[..., 2]) + Xt[..., r]
    return R, t


def edges(store_ids, store_poses, frame_a, frame_b, rel_pose, pose_a=None):
    """-> (P, A, valid): P_i = mul(B_i, T_i), A_i, and the edges whose poses exist with all 36 numbers finite.
    store_ids / store_poses: what set_frame_poses holds ((m,) ids, (m, 12) f32)."""
    frame_b = np.asarray(frame_b, np.int64).reshape(-1)
    n = frame_b.size
    T = from_rel(rel_pose)
    store = {int(i): k for k, i in enumerate(np.asarray(store_ids).reshape(-1))}
    sp = np.asarray(store_poses, np.float32).reshape(-1, 12)

    def gather(ids):
        rows = np.zeros((n, 12), np.float32)
        have = np.zeros(n, bool)
        for i, f in enumerate(ids):
            k = store.get(int(f))
            if k is not None:
                rows[i] = sp[k]
                have[i] = True
        return rows, have

    b_rows, valid = gather(frame_b)
    if pose_a is not None:
        a_rows = np.asarray(pose_a, np.float32).reshape(-1, 12)
    else:
        a_rows, have_a = gather(np.asarray(frame_a, np.int64).reshape(-1))
        valid &= have_a
    valid &= np.isfinite(b_rows).all(1) & np.isfinite(a_rows).all(1) & np.isfinite(np.asarray(rel_pose, np.float64).reshape(-1, 12)).all(1)
    B, A = from_rows34(b_rows), from_rows34(a_rows)
    with np.errstate(all="ignore"):
        P = mul(B, T)
    return P, A, valid


def adjacency(P, A, valid, tt, min_trace, block=64):
    """-> (adj, gap_d2, gap_tr): adj (n, n) bool, symmetric, zero diagonal, empty rows and columns for invalid edges;
    gap_d2[i, j] = |d2 - tt| and gap_tr[i, j] = |tr - min_trace| for the pairs i < j of valid edges, +inf elsewhere"""
    n = valid.size
    adj = np.zeros((n, n), bool)
    gap_d2 = np.full((n, n), np.inf)
    gap_tr = np.full((n, n), np.inf)
    if n == 0:
        return adj, gap_d2, gap_tr
    iP, iA = inv(P), inv(A)
    with np.errstate(all="ignore"):
        for i0 in range(0, n, block):
            i1 = min(n, i0 + block)
            row = lambda X: (X[0][i0:i1, None], X[1][i0:i1, None])      # noqa: E731
            col = lambda X: (X[0][None, :], X[1][None, :])              # noqa: E731
            U = mul(row(iP), col(P))            # mul(inv(P_i), P_j)
            V = mul(col(iA), row(A))            # mul(inv(A_j), A_i)
            Zr, Zt = mul(U, V)
            d2 = (Zt[..., 0] * Zt[..., 0] + Zt[..., 1] * Zt[..., 1]) + Zt[..., 2] * Zt[..., 2]
            tr = (Zr[..., 0, 0] + Zr[..., 1, 1]) + Zr[..., 2, 2]
            ok = (d2 <= tt) & (tr >= min_trace)
            pair = (np.arange(i0, i1)[:, None] < np.arange(n)[None, :]) & valid[i0:i1, None] & valid[None, :]
            adj[i0:i1] = ok & pair
            gap_d2[i0:i1] = np.where(pair, np.abs(d2 - tt), np.inf)
            gap_tr[i0:i1] = np.where(pair, np.abs(tr - min_trace), np.inf)
    adj |= adj.T
    return adj, gap_d2, gap_tr


def greedy(adj, valid, shortcut=False):
    """the choice: -> (in_set, degree, pick, n_set).  shortcut=True takes the rest of P in ascending order as soon as
    every d(u) equals |P| - 1 (what the library may do); the outcome must be the same"""
    n = valid.size
    in_set = np.zeros(n, np.int32)
    pick = np.full(n, -1, np.int32)
    degree = np.where(valid, adj.sum(1), -1).astype(np.int32)
    P = valid.copy()
    n_set = 0
    while P.any():
        idx = np.flatnonzero(P)
        d = adj[np.ix_(idx, idx)].sum(1)
        if shortcut and (d == idx.size - 1).all():
            pick[idx] = n_set + np.arange(idx.size)
            in_set[idx] = 1
            n_set += idx.size
            break
        v = idx[int(np.argmax(d))]        # (argmax: the first of the largest = the lowest index)
        pick[v] = n_set
        in_set[v] = 1
        n_set += 1
        P &= adj[v]
    return in_set, degree, pick, n_set


def adjacency_rows(P, A, valid, tt, min_trace, rows, block=16):
    """the rule for the rows `rows` only -> (adj, gap_d2, gap_tr), each (len(rows), n): entry (k, j) is the decision of the
    pair (rows[k], j) taken with the lower index first, as adjacency() gives it after mirroring; the gaps are those of the
    ordered pair, +inf on the diagonal and for invalid edges"""
    rows = np.asarray(rows, np.int64).reshape(-1)
    n = valid.size
    adj = np.zeros((rows.size, n), bool)
    gap_d2 = np.full((rows.size, n), np.inf)
    gap_tr = np.full((rows.size, n), np.inf)
    iP, iA = inv(P), inv(A)
    col = lambda X: (X[0][None, :], X[1][None, :])                      # noqa: E731
    with np.errstate(all="ignore"):
        for k0 in range(0, rows.size, block):
            r = rows[k0:k0 + block]
            row = lambda X: (X[0][r, None], X[1][r, None])              # noqa: E731
            col_hi = r[:, None] < np.arange(n)[None, :]
            d2 = np.empty((r.size, n))
            tr = np.empty((r.size, n))
            for row_is_lo in (True, False):
                if row_is_lo:
                    U, V = mul(row(iP), col(P)), mul(col(iA), row(A))      # mul(inv(P_row), P_col), mul(inv(A_col), A_row)
                else:
                    U, V = mul(col(iP), row(P)), mul(row(iA), col(A))
                Zr, Zt = mul(U, V)
                take = col_hi == row_is_lo
                d2[take] = ((Zt[..., 0] * Zt[..., 0] + Zt[..., 1] * Zt[..., 1]) + Zt[..., 2] * Zt[..., 2])[take]
                tr[take] = ((Zr[..., 0, 0] + Zr[..., 1, 1]) + Zr[..., 2, 2])[take]
            pair = (r[:, None] != np.arange(n)[None, :]) & valid[r, None] & valid[None, :]
            adj[k0:k0 + block] = (d2 <= tt) & (tr >= min_trace) & pair
            gap_d2[k0:k0 + block] = np.where(pair, np.abs(d2 - tt), np.inf)
            gap_tr[k0:k0 + block] = np.where(pair, np.abs(tr - min_trace), np.inf)
    return adj, gap_d2, gap_tr


GREEDY_PARTS = dict(tie_high=False, total_degree=False, col_limit=None, row_limit=None, no_wave_prefix=False, psize_limit=None)
WAVE_BITS = 64 * 64      # the columns whose words one wave of the library's select pass owns


def greedy_fast(adj, valid, shortcut=False, parts=None):
    """the choice with the degrees kept incrementally -> (in_set, degree, pick, n_set, rounds); adj symmetric.  rounds is
    what consistency_rounds reports: one per pick, one for the shortcut when it fires (shortcut=True).
    parts replaces pieces of the rule, for the mutants of tests/_consistency_edges.py (None: the rule itself):
      tie_high        the highest index among equal degrees
      total_degree    after round 0 the choice looks at the edge's degree, not at d(u) inside P
      col_limit       d(u) counts the columns below col_limit only
      row_limit       the rows u >= row_limit are never counted (no candidates, no degree)
      no_wave_prefix  the shortcut's positions start again at |C| in every block of WAVE_BITS columns
      psize_limit     after a pick |P| is taken over the columns below psize_limit only"""
    p = dict(GREEDY_PARTS, **(parts or {}))
    n = valid.size
    idx_all = np.arange(n)
    in_set = np.zeros(n, np.int32)
    pick = np.full(n, -1, np.int32)
    degree = np.full(n, -1, np.int32)
    cols = np.ones(n, bool) if p["col_limit"] is None else idx_all < p["col_limit"]
    rows_ok = np.ones(n, bool) if p["row_limit"] is None else idx_all < p["row_limit"]
    P = np.asarray(valid, bool).copy()
    counted = P & cols
    D = np.count_nonzero(adj, axis=1) if counted.all() else np.count_nonzero(adj[np.flatnonzero(counted)], axis=0)
    D = D.astype(np.int64)
    deg0 = D.copy()
    psize = int(P.sum())
    n_set = rounds = 0
    while psize > 0:
        cand = P & rows_ok
        if rounds == 0:
            degree[cand] = D[cand]
        if not cand.any():
            break
        key = np.where(cand, deg0 if (p["total_degree"] and rounds > 0) else D, -1)
        if shortcut and int(np.count_nonzero(key == psize - 1)) == psize:
            members = np.flatnonzero(P)
            rank = np.arange(members.size)
            if p["no_wave_prefix"]:
                blk = members // WAVE_BITS
                rank = rank - np.searchsorted(blk, blk, side="left")
            pick[members] = n_set + rank
            in_set[members] = 1
            n_set += psize
            rounds += 1
            break
        v = int(n - 1 - np.argmax(key[::-1])) if p["tie_high"] else int(np.argmax(key))
        pick[v] = n_set
        in_set[v] = 1
        n_set += 1
        rounds += 1
        new_P = P & adj[v]
        gone = np.flatnonzero(P & ~new_P & cols)
        left = np.flatnonzero(new_P & cols)
        if gone.size <= left.size:
            D -= np.count_nonzero(adj[gone], axis=0)
        else:
            D = np.zeros(n, np.int64)
            members = np.flatnonzero(new_P)
            D[members] = np.count_nonzero(adj[np.ix_(members, left)], axis=1)
        P = new_P
        psize = int(P.sum()) if p["psize_limit"] is None else int(P[:p["psize_limit"]].sum())
    return in_set, degree, pick, n_set, rounds


def unpack_rows(rows, n):
    """the inverse of pack_rows: (n, ceil(n / 64)) uint64 -> (n, n) bool (the padding bits are dropped)"""
    bits = np.unpackbits(np.ascontiguousarray(rows, "<u8").view(np.uint8).reshape(rows.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)


def pack_rows(adj):
    """(n, n) bool -> (n, ceil(n / 64)) uint64: bit j of row i = bit j & 63 of word j >> 6, padding bits 0"""
    n = adj.shape[0]
    words = (n + 63) // 64
    padded = np.zeros((n, words * 64), np.uint8)
    padded[:, :n] = adj
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(n, words).astype(np.uint64)


def consistent(store_ids, store_poses, frame_a, frame_b, rel_pose, tt, min_trace, pose_a=None, shortcut=False):
    """the whole rule -> dict of in_set, degree, pick, n_set, rows, adj, valid and the smallest gaps to the thresholds"""
    P, A, valid = edges(store_ids, store_poses, frame_a, frame_b, rel_pose, pose_a)
    adj, g2, gt = adjacency(P, A, valid, tt, min_trace)
    in_set, degree, pick, n_set = greedy(adj, valid, shortcut)
    return {"in_set": in_set, "degree": degree, "pick": pick, "n_set": n_set, "rows": pack_rows(adj), "adj": adj,
            "valid": valid, "gap_d2": g2, "gap_tr": gt,
            "min_gap_d2": float(g2.min()) if g2.size else np.inf, "min_gap_tr": float(gt.min()) if gt.size else np.inf}


def thresholds(max_trans, max_rot):
    """tt and min_trace as the header states them (the library hands its own back; the GPU tests use those)"""
    return max_trans * max_trans, 1.0 + 2.0 * np.cos(max_rot)


def clear_of_thresholds(ref, tt, min_trace, rel=1e-9):
    """no pair within rel * max(1, |threshold|) of either threshold"""
    return ref["min_gap_d2"] > rel * max(1.0, abs(tt)) and ref["min_gap_tr"] > rel * max(1.0, abs(min_trace))


# ---- planted worlds (inputs only: ordinary numpy is fine here) ----
def rot_axis_angle(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def rows34(R, t):
    return np.concatenate([R, t[:, :, None]], axis=2).reshape(-1, 12)


def _compose(Ra, ta, Rb, tb):
    return Ra @ Rb, (Ra @ tb[..., None])[..., 0] + ta


def _invert(R, t):
    Rt = np.swapaxes(R, -1, -2)
    return Rt, -(Rt @ t[..., None])[..., 0]


def trajectory(n_frames, rng, step=0.25):
    """a planar random walk with yaw drift and a little roll/pitch: (n, 12) f32 poses"""
    R = np.zeros((n_frames, 3, 3))
    t = np.zeros((n_frames, 3))
    yaw, pos = 0.0, np.zeros(3)
    for k in range(n_frames):
        yaw += rng.normal(0, 0.15)
        Rk = rot_axis_angle([0, 0, 1], yaw) @ rot_axis_angle(rng.normal(size=3), rng.normal(0, 0.02))
        pos = pos + Rk @ np.array([step, 0, 0]) + rng.normal(0, 0.05, 3)
        R[k], t[k] = Rk, pos
    return rows34(R, t).astype(np.float32)


def planted_world(n_true, n_outlier, n_alias, seed, n_frames=None, noise_t=0.02, noise_r=np.deg2rad(0.2), alias_shift=25.0, step=0.25):
    """n_true loops between frames of one trajectory (T = inv(B) A with noise_t / noise_r noise), n_outlier wrong ones of
    which the first n_alias are aliases: mutually consistent (one wrong place, alias_shift metres away) but not with the
    true ones.  A pair of true loops closes its cycle up to the two loops' noise: about sqrt(2) * (noise_t * sqrt(3) +
    noise_r * D) with D the distance between the two query frames (a rotation error acts over that lever arm), so a
    threshold has to be chosen for the extent of the session (step sets it).  -> dict of ids, poses (the store), frame_a, frame_b, rel_pose (n, 12), is_true (n,), is_alias (n,)"""
    rng = np.random.default_rng(seed)
    n = n_true + n_outlier
    n_frames = n_frames or max(2 * n, 64)
    poses = trajectory(n_frames, rng, step)
    ids = np.arange(n_frames, dtype=np.uint32)
    fa = rng.integers(n_frames // 2, n_frames, n).astype(np.uint32)
    fb = rng.integers(0, n_frames // 2, n).astype(np.uint32)
    Ra, ta = from_rows34(poses[fa])
    Rb, tb = from_rows34(poses[fb])
    Rbi, tbi = _invert(Rb, tb)
    G_R = rot_axis_angle([0, 0, 1], 0.3)
    G_t = np.array([alias_shift, -0.6 * alias_shift, 0.0])
    rel = np.zeros((n, 12))
    for i in range(n):
        if i < n_true:
            Rn = rot_axis_angle(rng.normal(size=3), rng.normal(0, noise_r))
            Rw, tw = _compose(Ra[i], ta[i], Rn, rng.normal(0, noise_t, 3))
        elif i < n_true + n_alias:
            Rw, tw = _compose(G_R, G_t, Ra[i], ta[i])
        else:
            Rw, tw = _compose(rot_axis_angle(rng.normal(size=3), rng.uniform(0.3, 3.0)), rng.uniform(-60, 60, 3), Ra[i], ta[i])
        Rr, tr = _compose(Rbi[i], tbi[i], Rw, tw)
        rel[i, :9], rel[i, 9:] = Rr.reshape(9), tr
    order = rng.permutation(n)
    kind = np.zeros(n, np.int8)
    kind[n_true:n_true + n_alias] = 1
    kind[n_true + n_alias:] = 2
    return {"ids": ids, "poses": poses, "frame_a": fa[order], "frame_b": fb[order], "rel_pose": rel[order],
            "is_true": kind[order] == 0, "is_alias": kind[order] == 1}
