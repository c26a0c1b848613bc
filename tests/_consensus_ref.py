"""numpy restatement of sgtd_pose_consensus' rule, written from the comment in include/sgtd_accel.h: f64 throughout, every
sum spelled out in the stated order.  inv / mul / greedy are _consistency_ref's, quat_of / unit / rot_of _relax_ref's.
Plus the planted batches the consensus tests and tools/consensus_bench.py share.

Inputs have the layouts of the C call: n_cand (nq,), cand_frame (nq, cn) int32, score (nq, cn) f64, rel_pose (nq, cn, 12)
f64 (rot row-major (9), t (3)); the store is what set_frame_poses holds ((m,) ids, (m, 12) f32 rows of [R | t])."""
import numpy as np

import _consistency_ref as cr
import _relax_ref as rr

KIND_TRUE, KIND_ALIAS, KIND_LONER, KIND_REJECTED, KIND_NO_POSE, KIND_NAN_POSE, KIND_PAST = range(7)


def candidates(store_ids, store_poses, n_cand, cand_frame, score, rel_pose):
    """one query -> (P, valid): P_k = mul(B_k, T_k) and the validity of the header"""
    cand_frame = np.asarray(cand_frame, np.int32).reshape(-1)
    cn = cand_frame.size
    score = np.asarray(score, np.float64).reshape(cn)
    rel = np.asarray(rel_pose, np.float64).reshape(cn, 12)
    store = {int(i): k for k, i in enumerate(np.asarray(store_ids).reshape(-1))}
    sp = np.asarray(store_poses, np.float32).reshape(-1, 12)
    rows = np.zeros((cn, 12), np.float32)
    valid = (np.arange(cn) < int(n_cand)) & (score >= 0.0)
    for k in range(cn):
        j = store.get(int(np.uint32(cand_frame[k])))       # (the library reads the id as u32)
        if j is None:
            valid[k] = False
        else:
            rows[k] = sp[j]
    valid &= np.isfinite(rows).all(1) & np.isfinite(rel).all(1)
    with np.errstate(all="ignore"):
        P = cr.mul(cr.from_rows34(rows), cr.from_rel(rel))
    return P, valid


def adjacency(P, valid, tt, min_trace):
    """-> (adj, gap_d2, gap_tr) as _consistency_ref.adjacency gives them, with Z = mul(inv(P_k), P_l) for k < l"""
    n = valid.size
    with np.errstate(all="ignore"):
        iP = cr.inv(P)
        Zr, Zt = cr.mul((iP[0][:, None], iP[1][:, None]), (P[0][None, :], P[1][None, :]))
        d2 = (Zt[..., 0] * Zt[..., 0] + Zt[..., 1] * Zt[..., 1]) + Zt[..., 2] * Zt[..., 2]
        tr = (Zr[..., 0, 0] + Zr[..., 1, 1]) + Zr[..., 2, 2]
        ok = (d2 <= tt) & (tr >= min_trace)
    pair = (np.arange(n)[:, None] < np.arange(n)[None, :]) & valid[:, None] & valid[None, :]
    adj = ok & pair
    adj |= adj.T
    return adj, np.where(pair, np.abs(d2 - tt), np.inf), np.where(pair, np.abs(tr - min_trace), np.inf)


def fuse(P, score, in_set, seed):
    """the fusion and the figures over the members in ascending index -> (pose12, support, spread_t2, spread_trace)"""
    members = np.flatnonzero(in_set)
    R, t = P
    q = rr.quat_of(R)
    ts = np.zeros(3)
    Q = np.zeros(4)
    support = 0.0
    for m in members:
        for c in range(3):
            ts[c] = ts[c] + t[m, c]
        s = ((q[m, 0] * q[seed, 0] + q[m, 1] * q[seed, 1]) + q[m, 2] * q[seed, 2]) + q[m, 3] * q[seed, 3]
        qm = -q[m] if s < 0.0 else q[m]
        for c in range(4):
            Q[c] = Q[c] + qm[c]
        support = support + score[m]
    that = ts / float(members.size)
    Rh = rr.rot_of(rr.unit(Q))
    spread_t2 = spread_tr = None
    for m in members:
        e = t[m] - that
        e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        r = [(Rh[i, 0] * R[m, i, 0] + Rh[i, 1] * R[m, i, 1]) + Rh[i, 2] * R[m, i, 2] for i in range(3)]
        tr = (r[0] + r[1]) + r[2]
        spread_t2 = e2 if spread_t2 is None else (e2 if e2 > spread_t2 else spread_t2)
        spread_tr = tr if spread_tr is None else (tr if tr < spread_tr else spread_tr)
    return np.concatenate([Rh, that[:, None]], axis=1).reshape(12), support, spread_t2, spread_tr


def consensus(store_ids, store_poses, n_cand, cand_frame, score, rel_pose, tt, min_trace, shortcut=False):
    """the whole rule for every query -> dict of pose [nq, 12], n_valid, n_set, seed [nq], mask [nq] (uint64),
    support_score, spread_t2, spread_trace [nq], rows [nq, cn] (uint64), degree, pick [nq, cn], adj [nq, cn, cn], valid
    [nq, cn], world (R [nq, cn, 3, 3], t [nq, cn, 3]: P) and the smallest gaps to the thresholds"""
    n_cand = np.asarray(n_cand, np.int32).reshape(-1)
    nq = n_cand.size
    score = np.asarray(score, np.float64)
    cn = score.shape[-1] if score.ndim == 2 else score.size // max(nq, 1)
    score = score.reshape(nq, cn)
    cand_frame = np.asarray(cand_frame, np.int32).reshape(nq, cn)
    rel_pose = np.asarray(rel_pose, np.float64).reshape(nq, cn, 12)
    out = {"pose": np.full((nq, 12), np.nan), "n_valid": np.zeros(nq, np.int32), "n_set": np.zeros(nq, np.int32),
           "seed": np.full(nq, -1, np.int32), "mask": np.zeros(nq, np.uint64), "support_score": np.zeros(nq),
           "spread_t2": np.full(nq, np.nan), "spread_trace": np.full(nq, np.nan), "rows": np.zeros((nq, cn), np.uint64),
           "degree": np.full((nq, cn), -1, np.int32), "pick": np.full((nq, cn), -1, np.int32),
           "adj": np.zeros((nq, cn, cn), bool), "valid": np.zeros((nq, cn), bool),
           "world": (np.zeros((nq, cn, 3, 3)), np.zeros((nq, cn, 3))), "min_gap_d2": np.inf, "min_gap_tr": np.inf}
    for q in range(nq):
        P, valid = candidates(store_ids, store_poses, n_cand[q], cand_frame[q], score[q], rel_pose[q])
        adj, g2, gt = adjacency(P, valid, tt, min_trace)
        in_set, degree, pick, n_set = cr.greedy(adj, valid, shortcut)
        out["valid"][q], out["adj"][q], out["degree"][q], out["pick"][q] = valid, adj, degree, pick
        out["world"][0][q], out["world"][1][q] = P
        out["rows"][q] = (adj.astype(np.uint64) << np.arange(cn, dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64)
        out["n_valid"][q], out["n_set"][q] = valid.sum(), n_set
        out["min_gap_d2"] = min(out["min_gap_d2"], float(g2.min()))
        out["min_gap_tr"] = min(out["min_gap_tr"], float(gt.min()))
        if n_set == 0:
            continue
        seed = int(np.flatnonzero(pick == 0)[0])
        out["seed"][q] = seed
        out["mask"][q] = (in_set.astype(np.uint64) << np.arange(cn, dtype=np.uint64)).sum(dtype=np.uint64)
        out["pose"][q], out["support_score"][q], out["spread_t2"][q], out["spread_trace"][q] = fuse(P, score[q], in_set, seed)
    return out


def clear_of_thresholds(ref, tt, min_trace, rel=1e-9):
    """no pair within rel * max(1, |threshold|) of either threshold"""
    return ref["min_gap_d2"] > rel * max(1.0, abs(tt)) and ref["min_gap_tr"] > rel * max(1.0, abs(min_trace))


def members_of(mask, cn):
    return np.array([k for k in range(cn) if (int(mask) >> k) & 1], np.int64)


def edge_pose(store_ids, store_poses, frame, fused12):
    """mul(inv(B), fused): sgtd_result_consensus_edges' rel_pose row (rot (9), t (3))"""
    k = int(np.flatnonzero(np.asarray(store_ids).reshape(-1) == frame)[0])
    B = cr.from_rows34(np.asarray(store_poses, np.float32).reshape(-1, 12)[k:k + 1])
    F = np.asarray(fused12, np.float64).reshape(1, 3, 4)
    R, t = cr.mul(cr.inv(B), (F[:, :, :3].copy(), F[:, :, 3].copy()))
    return np.concatenate([R.reshape(9), t.reshape(3)])


# ---- planted batches (inputs only: ordinary numpy is fine here) ----
def _rel_rows(R, t):
    return np.concatenate([R.reshape(-1, 9), t.reshape(-1, 3)], axis=1)


def planted_batch(nq, cn, seed, n_frames=96, noise_t=0.02, noise_r=np.deg2rad(0.2), alias_shift=25.0, alias_larger_every=5):
    """nq queries of cn candidate slots against a map of n_frames frames.  Per query: a group near the true pose (noise
    inside any sensible bounds), a smaller alias group alias_shift metres away (larger than the true group in every
    alias_larger_every-th query), loners, rejected candidates (score -1), frames without a pose (one id beyond the stored
    range among them) and frames whose stored pose holds a NaN; n_cand varies from 0 to cn, query 1 (if there is one) has
    candidates but none valid.  -> dict of ids, poses (the store), n_cand, cand_frame, score, rel_pose, kind (nq, cn),
    true_pose (R [nq, 3, 3], t [nq, 3])"""
    rng = np.random.default_rng(seed)
    poses = cr.trajectory(n_frames, rng)
    ids = np.arange(n_frames, dtype=np.uint32)
    no_pose = (ids % 7) == 3
    nan_pose = (ids % 11) == 5
    poses[nan_pose & ~no_pose, 7] = np.nan
    stored = ~no_pose
    good = np.flatnonzero(stored & ~nan_pose)
    bad_nan = np.flatnonzero(stored & nan_pose)
    bad_none = np.concatenate([np.flatnonzero(no_pose), [n_frames + 100]])
    B_R, B_t = cr.from_rows34(poses)
    G_R, G_t = cr.rot_axis_angle([0, 0, 1], 0.3), np.array([alias_shift, -0.6 * alias_shift, 0.0])
    n_cand = np.zeros(nq, np.int32)
    cand_frame = np.zeros((nq, cn), np.int32)
    score = np.full((nq, cn), -1.0)
    rel = np.zeros((nq, cn, 12))
    kind = np.full((nq, cn), KIND_PAST, np.int8)
    true_R, true_t = np.zeros((nq, 3, 3)), np.zeros((nq, 3))
    for q in range(nq):
        f0 = int(rng.choice(good))
        Wr = B_R[f0] @ cr.rot_axis_angle(rng.normal(size=3), rng.normal(0, 0.1))
        Wt = B_t[f0] + rng.normal(0, 1.0, 3)
        true_R[q], true_t[q] = Wr, Wt
        n = cn if q % 3 == 0 else int(rng.integers(0, cn + 1))
        if q == 2:
            n = 0
        n_cand[q] = n
        if q == 1:
            kinds = rng.choice([KIND_REJECTED, KIND_NO_POSE, KIND_NAN_POSE], n)
        else:
            larger = alias_larger_every and q % alias_larger_every == alias_larger_every - 1
            p = [0.2, 0.4, 0.15, 0.1, 0.08, 0.07] if larger else [0.4, 0.2, 0.15, 0.1, 0.08, 0.07]
            kinds = rng.choice(6, n, p=p)
        kind[q, :n] = kinds
        for k in range(cn):
            kd = kind[q, k]
            f = int(rng.choice(bad_none if kd == KIND_NO_POSE else bad_nan if kd == KIND_NAN_POSE else good))
            if kd == KIND_ALIAS:
                Xr, Xt = G_R @ Wr, G_R @ Wt + G_t
            elif kd == KIND_LONER:
                Xr, Xt = cr.rot_axis_angle(rng.normal(size=3), rng.uniform(0.3, 3.0)) @ Wr, Wt + rng.uniform(-60, 60, 3)
            else:
                Xr, Xt = Wr, Wt
            Xr = Xr @ cr.rot_axis_angle(rng.normal(size=3), rng.normal(0, noise_r))
            Xt = Xt + rng.normal(0, noise_t, 3)
            cand_frame[q, k] = f
            if f < n_frames and np.isfinite(poses[f]).all():
                Rb, tb = B_R[f], B_t[f]
            else:
                Rb, tb = np.eye(3), np.zeros(3)
            rel[q, k] = _rel_rows(Rb.T @ Xr, Rb.T @ (Xt - tb))[0]
            score[q, k] = -1.0 if kd == KIND_REJECTED else float(rng.integers(4, 40))      # (a slot past n_cand looks like a true one)
    return {"ids": ids[stored], "poses": poses[stored], "n_cand": n_cand, "cand_frame": cand_frame, "score": score,
            "rel_pose": rel, "kind": kind, "true_pose": (true_R, true_t)}


def line_batch(xs, cn=None, scores=None):
    """one query whose candidate k sits at the world position (xs[k], 0, 0) with the identity rotation, against a map of
    identity poses (frame k for candidate k): exact arithmetic for integer xs.  xs[k] = None: a rejected candidate"""
    n = len(xs)
    cn = n if cn is None else cn
    ids = np.arange(cn, dtype=np.uint32)
    poses = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (cn, 1))
    rel = np.zeros((1, cn, 12))
    rel[0, :, [0, 4, 8]] = 1.0
    score = np.full((1, cn), -1.0)
    for k, x in enumerate(xs):
        if x is not None:
            rel[0, k, 9] = x
            score[0, k] = 10.0 + k if scores is None else scores[k]
    return {"ids": ids, "poses": poses, "n_cand": np.array([n], np.int32), "cand_frame": np.arange(cn, dtype=np.int32)[None, :].copy(),
            "score": score, "rel_pose": rel}


def stack(batches):
    """several batches over one store (the first's) as one"""
    b0 = batches[0]
    return {"ids": b0["ids"], "poses": b0["poses"], "n_cand": np.concatenate([b["n_cand"] for b in batches]),
            "cand_frame": np.concatenate([b["cand_frame"] for b in batches]), "score": np.concatenate([b["score"] for b in batches]),
            "rel_pose": np.concatenate([b["rel_pose"] for b in batches])}
