"""Batches at the edges of sgtd_pose_consensus (consensus_kernels.hip.h) and a restatement of its rule with replaceable
parts.  Plain helper module of tests/test_consensus_edges.py (CPU: consensus_with(..., None) is _consensus_ref.consensus
bit for bit, every mutant below changes the expected result on the cases named for it, every case's precondition holds)
and tests/test_gpu_consensus_edges.py (GPU: every form of the call equals the rule on them, bit for bit).

A case is a batch in _consensus_ref's dict layout (ids, poses, n_cand, cand_frame, score, rel_pose) with the bounds it is
run under: cases()[name] = dict(batch, max_trans, max_rot, noisy).  The integer cases (identity store, integer
translations, signed permutation matrices) have exact arithmetic under any association, contraction or role order; the
noisy ones are kept clear of both thresholds; knife_runs() sit ON the translation bound: the pair's d2 is the exact
square of a double, so with max_trans = sqrt(d2) the library's tt is d2 itself and the pair agrees through <=, while a d2
one ulp larger (roles swapped, a sum re-associated, a product fused) does not.

The mutants (MUTANT_CASES names the cases that show each):
  pair rule   roles_swapped   the pair decided as (hi, lo)
              roles_by_lane   adj[k, l] decided as (k, l), adj[l, k] as (l, k): asymmetric rows
              sum_right       a + (b + c) in the dot products of the Z step
              contracted      each product after the first fused into the add that follows
              lt_bound        d2 < tt                      gt_trace   tr > min_trace
  validity    score_gt0, ncand_ignored, ncand_unclamped (a lane k >= cn below n_cand reads the next query's candidate
              and counts as valid), frame_signed (-1 indexes the store from its end), frame_le_n_ids (the id n_ids reads a
              pose of zeros), has_ignored (an id in range without a pose reads zeros), T_rot_only, T_trans_only,
              B_unchecked
  choice      tie_high, total_degree, seed_lowest_member
  fusion      no_flip, flip_vs_lowest, flip_le, sum_pick_order, mean_by_n_valid, quat_trace_only, quat_ge,
              spread_vs_seed, spread_from_zero (both spreads start from 0.0: the trace one shows it)
None of the listed mutants had to be dropped.  Two notes on what it takes to show them:
  flip_vs_lowest  negating against the lowest member instead of the seed negates Q as a whole whenever the signs of the
                  dot products are transitive, and UNIT(-Q), ROT(-q) give the rule's bits.  It shows only with a member X
                  whose dot products with the seed and with the lowest member have one sign while those two's has the
                  other: nearly 90 degrees of half angle from both, so the hemisphere cases run under max_rot = pi and hold a member turned
                  300 degrees about -z beside the ones at 115 .. 125.
  quat_ge         needs tr == 0 exactly, a z-branch quaternion with w < 0 and a seed with dot == 0 exactly (or the sign is
                  undone by the hemisphere rule): pairs of the cube's three-fold rotations, found by search.
max_rot = pi / 2: 1.0 + 2.0 * cos(pi / 2) is 1 + 1.2246e-16, which rounds to the double ABOVE 1.0 (half an ulp is
1.1102e-16), so a quarter turn with tr == 1 exactly does NOT agree there; the case asserts just that."""
import functools
import itertools

import numpy as np

import _consensus_ref as ref
import _consistency_ref as cr
from _consistency_edges import dot3_contracted, dot3_plain, dot3_sum_right, inv_with, mul_with

INT_KEYS = ("n_valid", "n_set", "seed", "mask")
DBL_KEYS = ("pose", "support_score", "spread_t2", "spread_trace")
KNIFE_ROT = np.deg2rad(5.0)
PLACEMENTS = ((0, 1), (0, 63), (62, 63), (31, 32), (5, 40))
ARITH_MUTANTS = ("roles_swapped", "sum_right", "contracted")
PAIR_MUTANTS = ARITH_MUTANTS + ("roles_by_lane", "lt_bound", "gt_trace")
MUTANT_CASES = {
    "roles_swapped": ("knife_pairs",), "roles_by_lane": ("knife_pairs",), "sum_right": ("knife_pairs",), "contracted": ("knife_pairs",),
    "lt_bound": ("knife_pairs", "on_bound", "descending"), "gt_trace": ("half_turns", "zero_rot"),
    "score_gt0": ("validity", "validity_rev"), "ncand_ignored": ("ncand", "ncand_cn3", "cn1", "stale_second"),
    "ncand_unclamped": ("ncand_cn3", "cn1"), "frame_signed": ("validity", "validity_rev"),
    "frame_le_n_ids": ("validity", "validity_rev"), "has_ignored": ("validity", "validity_rev"),
    "T_rot_only": ("validity", "validity_rev"), "T_trans_only": ("validity", "validity_rev"), "B_unchecked": ("validity", "validity_rev"),
    "tie_high": ("isolated", "tie"), "total_degree": ("remaining_degree", "remaining_degree_rev"),
    "seed_lowest_member": ("descending", "chain_low", "hemisphere_a", "hemisphere_b"),
    "no_flip": ("hemisphere_a", "hemisphere_b"), "flip_vs_lowest": ("hemisphere_a", "hemisphere_b"),
    "flip_le": ("half_turns", "three_cycles_a", "three_cycles_b"), "sum_pick_order": ("sum_order_a", "sum_order_b"),
    "mean_by_n_valid": ("tie", "descending", "sum_order_a"), "quat_trace_only": ("hemisphere_a", "hemisphere_b"),
    "quat_ge": ("three_cycles_a", "three_cycles_b"), "spread_vs_seed": ("tie", "sum_order_a", "hemisphere_a"),
    "spread_from_zero": ("tie", "sum_order_a", "descending"),
}
MUTANTS = tuple(MUTANT_CASES)
_DOT3 = {"sum_right": dot3_sum_right, "contracted": dot3_contracted}


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def differs(a, b):
    """the compared outputs of two results: the keys that differ"""
    out = [k for k in INT_KEYS if not np.array_equal(a[k], b[k])]
    out += [k for k in DBL_KEYS if not np.array_equal(bits(a[k]), bits(b[k]))]
    return out + [k for k in ("rows", "degree", "pick") if not np.array_equal(a[k], b[k])]


# ---- the restatement with replaceable parts ----
def quat_with(R, mutant=None):
    """QUAT of the header for one rotation -> (q (4,), branch 0 .. 3), with the branch conditions replaceable"""
    R = np.asarray(R, np.float64)
    with np.errstate(all="ignore"):
        tr = (R[0, 0] + R[1, 1]) + R[2, 2]
        first = tr >= 0.0 if mutant == "quat_ge" else tr > 0.0
        if mutant == "quat_trace_only" and tr > -1.0:
            first = True
        if first:
            s = np.sqrt(tr + 1.0) * 2.0
            q, branch = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s], 0
        elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
            s = np.sqrt(((1.0 + R[0, 0]) - R[1, 1]) - R[2, 2]) * 2.0
            q, branch = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s], 1
        elif R[1, 1] > R[2, 2]:
            s = np.sqrt(((1.0 + R[1, 1]) - R[0, 0]) - R[2, 2]) * 2.0
            q, branch = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s], 2
        else:
            s = np.sqrt(((1.0 + R[2, 2]) - R[0, 0]) - R[1, 1]) * 2.0
            q, branch = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s], 3
        q = np.array(q, np.float64)
        nn = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
        return q / np.sqrt(nn), branch


def _unit(q):
    nn = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]
    return q / np.sqrt(nn)


def _rot(q):
    w, x, y, z = q
    return np.array([[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]])


def _store_of(b):
    ids = np.asarray(b["ids"]).reshape(-1)
    sp = np.asarray(b["poses"], np.float32).reshape(-1, 12)
    return {int(i): sp[k] for k, i in enumerate(ids)}, (int(ids.max()) + 1 if ids.size else 0)


def _lane(b, store, n_ids, flat, mutant):
    """the candidate at the flat index -> (ok without the n_cand condition, its store row)"""
    score = np.asarray(b["score"], np.float64).reshape(-1)[flat]
    T = np.asarray(b["rel_pose"], np.float64).reshape(-1, 12)[flat]
    raw = int(np.asarray(b["cand_frame"], np.int32).reshape(-1)[flat])
    f = raw & 0xFFFFFFFF
    row = store.get(f)
    if mutant == "frame_signed" and raw < 0:
        row = store.get(n_ids + raw)
    if mutant == "frame_le_n_ids" and f == n_ids:
        row = np.zeros(12, np.float32)
    if mutant == "has_ignored" and f < n_ids and row is None:
        row = np.zeros(12, np.float32)
    ok = bool(score > 0.0) if mutant == "score_gt0" else bool(score >= 0.0)
    ok = ok and row is not None
    row = np.zeros(12, np.float32) if row is None else row
    checked = T[:9] if mutant == "T_rot_only" else T[9:] if mutant == "T_trans_only" else T
    ok = ok and bool(np.isfinite(checked).all()) and (mutant == "B_unchecked" or bool(np.isfinite(row).all()))
    return ok, row


def candidates_with(b, q, mutant=None):
    """one query -> (P, valid, extra): extra = the lanes beyond cn that a kernel without the clamp would count"""
    nq = np.asarray(b["n_cand"]).size
    cn = np.asarray(b["score"]).reshape(nq, -1).shape[1]
    store, n_ids = _store_of(b)
    n = int(np.asarray(b["n_cand"]).reshape(-1)[q])
    rows = np.zeros((cn, 12), np.float32)
    valid = np.zeros(cn, bool)
    for k in range(cn):
        ok, rows[k] = _lane(b, store, n_ids, q * cn + k, mutant)
        valid[k] = ok and (mutant == "ncand_ignored" or k < n)
    extra = 0
    if mutant == "ncand_unclamped":
        extra = sum(_lane(b, store, n_ids, q * cn + k, mutant)[0] for k in range(cn, min(n, 64)) if q * cn + k < nq * cn)
    rel = np.asarray(b["rel_pose"], np.float64).reshape(nq, cn, 12)[q]
    with np.errstate(all="ignore"):
        P = cr.mul(cr.from_rows34(rows), cr.from_rel(rel))
    return P, valid, extra


def z_values(P, lo, hi, dot3=dot3_plain):
    """(d2, tr) of Z = mul(inv(P_lo), P_hi) for index arrays lo, hi (any shape), the Z step and d2 taken by dot3"""
    with np.errstate(all="ignore"):
        iP = inv_with(P, dot3_plain)
        Zr, Zt = mul_with((iP[0][lo], iP[1][lo]), (P[0][hi], P[1][hi]), dot3)
        d2 = dot3(Zt[..., 0], Zt[..., 0], Zt[..., 1], Zt[..., 1], Zt[..., 2], Zt[..., 2])
        tr = (Zr[..., 0, 0] + Zr[..., 1, 1]) + Zr[..., 2, 2]
    return d2, tr


def adjacency_with(P, valid, tt, min_trace, mutant=None):
    """-> (adj, gap_d2, gap_tr); the gaps are those of the rule's ordered pairs k < l"""
    n = valid.size
    adj = np.zeros((n, n), bool)
    gap_d2 = np.full((n, n), np.inf)
    gap_tr = np.full((n, n), np.inf)
    v = np.flatnonzero(valid)
    if v.size == 0:
        return adj, gap_d2, gap_tr
    sub = (P[0][v], P[1][v])
    k, l = np.meshgrid(np.arange(v.size), np.arange(v.size), indexing="ij")
    d2, tr = z_values(sub, k, l, _DOT3.get(mutant, dot3_plain))          # [k, l]: k in the role of the lower index
    with np.errstate(invalid="ignore"):
        ok = (d2 < tt if mutant == "lt_bound" else d2 <= tt) & (tr > min_trace if mutant == "gt_trace" else tr >= min_trace)
    upper = k < l
    if mutant == "roles_by_lane":
        a = ok & (k != l)
    else:
        a = (ok.T if mutant == "roles_swapped" else ok) & upper
        a = a | a.T
    adj[np.ix_(v, v)] = a
    g2, gt = np.where(upper, np.abs(d2 - tt), np.inf), np.where(upper, np.abs(tr - min_trace), np.inf)
    gap_d2[np.ix_(v, v)] = g2
    gap_tr[np.ix_(v, v)] = gt
    return adj, gap_d2, gap_tr


def greedy_with(adj, valid, mutant=None, shortcut=False):
    """the choice -> (in_set, degree, pick, n_set); rows may be asymmetric (d(u) counts row u, P &= row v)"""
    n = valid.size
    in_set = np.zeros(n, np.int32)
    pick = np.full(n, -1, np.int32)
    deg0 = adj.sum(1)
    degree = np.where(valid, deg0, -1).astype(np.int32)
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
        key = deg0[idx] if (mutant == "total_degree" and n_set > 0) else d
        best = idx[key == key.max()]
        v = best[-1] if mutant == "tie_high" else best[0]
        pick[v] = n_set
        in_set[v] = 1
        n_set += 1
        P &= adj[v]
    return in_set, degree, pick, n_set


def fuse_with(P, score, in_set, seed, pick, n_valid, mutant=None):
    """the fusion and the figures -> (pose12, support, spread_t2, spread_trace, negated): negated = the members with
    s_m < 0 (under the mutant's rule), dots = their s_m"""
    members = np.flatnonzero(in_set)
    order = members[np.argsort(pick[members])] if mutant == "sum_pick_order" else members
    R, t = P
    with np.errstate(all="ignore"):
        q = {int(m): quat_with(R[m], mutant)[0] for m in members}
        q[int(seed)] = quat_with(R[seed], mutant)[0]
        against = q[int(members[0])] if mutant == "flip_vs_lowest" else q[int(seed)]
        ts = np.zeros(3)
        Q = np.zeros(4)
        support = 0.0
        negated, dots = [], {}
        for m in order:
            for c in range(3):
                ts[c] = ts[c] + t[m, c]
            qm = q[int(m)]
            s = ((qm[0] * against[0] + qm[1] * against[1]) + qm[2] * against[2]) + qm[3] * against[3]
            dots[int(m)] = s
            neg = False if mutant == "no_flip" else (s <= 0.0 if mutant == "flip_le" else s < 0.0)
            if neg:
                negated.append(int(m))
                qm = -qm
            for c in range(4):
                Q[c] = Q[c] + qm[c]
            support = support + score[m]
        that = ts / float(n_valid if mutant == "mean_by_n_valid" else members.size)
        Rh = _rot(_unit(Q))
        c_t, c_R = (t[seed], R[seed]) if mutant == "spread_vs_seed" else (that, Rh)
        spread_t2 = spread_tr = 0.0 if mutant == "spread_from_zero" else None
        for m in members:
            e = t[m] - c_t
            e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
            r = [(c_R[i, 0] * R[m, i, 0] + c_R[i, 1] * R[m, i, 1]) + c_R[i, 2] * R[m, i, 2] for i in range(3)]
            tr = (r[0] + r[1]) + r[2]
            spread_t2 = e2 if spread_t2 is None else (e2 if e2 > spread_t2 else spread_t2)
            spread_tr = tr if spread_tr is None else (tr if tr < spread_tr else spread_tr)
    return np.concatenate([Rh, that[:, None]], axis=1).reshape(12), support, spread_t2, spread_tr, negated, dots


def consensus_with(b, tt, min_trace, mutant=None, shortcut=False):
    """_consensus_ref.consensus' rule over the batch b with the part named by `mutant` replaced (None: the rule).  -> its
    dict, plus gap_d2 [nq, cn, cn], negated (per query: the members with s_m < 0), dots (per query: member -> s_m) and
    branch [nq, cn] (QUAT's branch of every valid candidate, else -1)"""
    assert mutant is None or mutant in MUTANTS, mutant
    n_cand = np.asarray(b["n_cand"], np.int32).reshape(-1)
    nq = n_cand.size
    score = np.asarray(b["score"], np.float64).reshape(nq, -1)
    cn = score.shape[1]
    out = {"pose": np.full((nq, 12), np.nan), "n_valid": np.zeros(nq, np.int32), "n_set": np.zeros(nq, np.int32),
           "seed": np.full(nq, -1, np.int32), "mask": np.zeros(nq, np.uint64), "support_score": np.zeros(nq),
           "spread_t2": np.full(nq, np.nan), "spread_trace": np.full(nq, np.nan), "rows": np.zeros((nq, cn), np.uint64),
           "degree": np.full((nq, cn), -1, np.int32), "pick": np.full((nq, cn), -1, np.int32),
           "adj": np.zeros((nq, cn, cn), bool), "valid": np.zeros((nq, cn), bool), "gap_d2": np.full((nq, cn, cn), np.inf),
           "world": (np.zeros((nq, cn, 3, 3)), np.zeros((nq, cn, 3))), "min_gap_d2": np.inf, "min_gap_tr": np.inf,
           "negated": [[] for _ in range(nq)], "dots": [{} for _ in range(nq)], "branch": np.full((nq, cn), -1, np.int8)}
    shifts = np.arange(cn, dtype=np.uint64)
    for q in range(nq):
        P, valid, extra = candidates_with(b, q, mutant)
        adj, g2, gt = adjacency_with(P, valid, tt, min_trace, mutant)
        in_set, degree, pick, n_set = greedy_with(adj, valid, mutant, shortcut)
        out["valid"][q], out["adj"][q], out["degree"][q], out["pick"][q], out["gap_d2"][q] = valid, adj, degree, pick, g2
        out["world"][0][q], out["world"][1][q] = P
        out["rows"][q] = (adj.astype(np.uint64) << shifts[None, :]).sum(1, dtype=np.uint64)
        out["n_valid"][q], out["n_set"][q] = int(valid.sum()) + extra, n_set
        out["min_gap_d2"] = min(out["min_gap_d2"], float(g2.min()))
        out["min_gap_tr"] = min(out["min_gap_tr"], float(gt.min()))
        for k in np.flatnonzero(valid):
            if np.isfinite(P[0][k]).all():
                out["branch"][q, k] = quat_with(P[0][k])[1]
        if n_set == 0:
            continue
        members = np.flatnonzero(in_set)
        seed = int(members[0]) if mutant == "seed_lowest_member" else int(np.flatnonzero(pick == 0)[0])
        out["seed"][q] = seed
        out["mask"][q] = (in_set.astype(np.uint64) << shifts).sum(dtype=np.uint64)
        fused = fuse_with(P, score[q], in_set, seed, pick, int(out["n_valid"][q]), mutant)
        out["pose"][q], out["support_score"][q], out["spread_t2"][q], out["spread_trace"][q] = fused[:4]
        out["negated"][q], out["dots"][q] = fused[4], fused[5]
    return out


def reference(b, tt, min_trace, shortcut=False):
    return ref.consensus(b["ids"], b["poses"], b["n_cand"], b["cand_frame"], b["score"], b["rel_pose"], tt, min_trace, shortcut)


# ---- builders ----
EYE12 = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
I3 = np.eye(3)
RZ90 = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
C3 = np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])
HX, HY, HZ = np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1])


def world_batch(cands, cn=None, scores=None):
    """one query against an identity store of cn frames (frame k for candidate k): cands[k] = (R, t), the world pose of
    candidate k, or None for a rejected one"""
    n = len(cands)
    cn = n if cn is None else cn
    b = ref.line_batch([None] * n, cn)
    for k, c in enumerate(cands):
        if c is not None:
            b["rel_pose"][0, k, :9] = np.asarray(c[0], np.float64).reshape(9)
            b["rel_pose"][0, k, 9:] = c[1]
            b["score"][0, k] = 10.0 + k if scores is None else scores[k]
    return b


def points_batch(pts, cn=None):
    return world_batch([None if p is None else (I3, np.asarray(p, np.float64)) for p in pts], cn)


def permuted(b, order):
    """the one-query batch b with candidate order[k] standing at lane k"""
    order = np.asarray(order)
    return dict(b, cand_frame=b["cand_frame"][:, order], score=b["score"][:, order], rel_pose=b["rel_pose"][:, order])


def with_n_cand(b, n):
    return dict(b, n_cand=np.array([n], np.int32))


@functools.lru_cache(None)
def cube_rotations():
    """the 24 signed permutation matrices of determinant +1"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for r in range(3):
                R[r, perm[r]] = signs[r]
            if round(np.linalg.det(R)) == 1:
                out.append(R)
    return out


@functools.lru_cache(None)
def zero_dot_pairs():
    """ordered pairs (S, M) of three-fold cube rotations (tr == 0 exactly, the all-equal diagonal: the z branch) whose
    quaternions have dot == 0 exactly and of which exactly one has w < 0: tr >= 0 -> branch 0 would turn that one's sign
    and, the dot being 0, the hemisphere rule would not turn it back"""
    three = [R for R in cube_rotations() if R[0, 0] + R[1, 1] + R[2, 2] == 0]
    assert len(three) == 8
    out = []
    for S in three:
        for M in three:
            qs, qm = quat_with(S)[0], quat_with(M)[0]
            if ((qs[0] * qm[0] + qs[1] * qm[1]) + qs[2] * qm[2]) + qs[3] * qm[3] == 0.0 and (qs[0] < 0) != (qm[0] < 0):
                out.append((S, M))
    return out


def _three_cycles(part):
    pairs = zero_dot_pairs()[part::2][:4]
    t = np.array([3.0, -2.0, 7.0])
    return ref.stack([world_batch([None, (S, t), None, None, None, (M, t), (M, t + 50.0), None]) for S, M in pairs])


def _half_turns():
    """I, Hx, Hy, Hz in four orders (each is the seed once), one place; bound -1: everything agrees"""
    mats = [I3, HX, HY, HZ]
    t = np.array([-4.0, 9.0, 1.0])
    return ref.stack([world_batch([(mats[(k + s) % 4], t) for k in range(4)] + [None, (I3, t + 30.0)], cn=8) for s in range(4)])


def _descending():
    """members at x = 1 .. 5 on lanes 10, 20, 30, 40, 63; extras e_i (i = 2 .. 5) at (i + 6, +-8, 0) / (i + 6, 0, +-8), 11.3
    apart from each other, see the members j >= i at d2 = dx^2 + 64 <= 100 (the nearest exactly ON the bound of 10).  Degrees:
    4 + (i - 1) for member i: 63 first, then 40, 30, 20, and 10 (degree 0 inside P, as e_2 on lane 12: the lower lane)"""
    pts = [None] * 64
    for i, lane in enumerate((10, 20, 30, 40, 63), start=1):
        pts[lane] = (i, 0, 0)
    for i, (lane, off) in enumerate(((12, (8, 0)), (50, (-8, 0)), (15, (0, 8)), (62, (0, -8))), start=2):
        pts[lane] = (i + 6, off[0], off[1])
    return points_batch(pts)


REMAINING_PTS = [(0, 0, 0), (5, 0, 0)] + [(2, 0, 0)] * 6 + [(10, 0, 0)] * 8 + [(-3, 0, 0)] * 5 + [(0, 5, 0), (0, -5, 0), (0, 0, 5), (0, 0, -5)]


def _full_wave():
    """sets of 64 and 63 through the shortcut over the full wave: all at one place; lane 17 rejected; lane 0 far away"""
    return ref.stack([points_batch([(7, 0, 0)] * 64), points_batch([(7, 0, 0)] * 17 + [None] + [(7, 0, 0)] * 46),
                      points_batch([(90, 0, 0)] + [(7, 0, 0)] * 63)])


def _validity(reverse):
    """cn = 64, a store of n_ids = 40 ids: 0 .. 11 hold a NaN or an inf in slot i, 20 has no pose, the rest the identity"""
    n_ids, dropped, cn = 40, 20, 64
    poses = np.tile(EYE12, (n_ids, 1))
    for i in range(12):
        poses[i, i] = (np.nan, np.inf, np.nan, -np.inf)[i % 4]
    keep = np.array([i for i in range(n_ids) if i != dropped])
    good = [i for i in range(12, n_ids) if i != dropped]
    queries = []
    for inf_member in (False, True):
        frame = np.array([good[k % len(good)] for k in range(cn)], np.int32)
        score = 5.0 + np.arange(cn)
        rel = np.zeros((cn, 12))
        rel[:, [0, 4, 8]] = 1.0
        for i in range(12):
            rel[i, i] = np.nan
            rel[12 + i, i] = np.inf if i % 2 == 0 else -np.inf
            frame[24 + i] = i
        score[36], score[37], score[38], score[39] = 0.0, -0.0, np.inf, np.nan
        if not inf_member:
            rel[38, 9] = 100.0
        frame[40], frame[41], frame[42], frame[43], frame[44] = -1, n_ids - 1, n_ids, 2 ** 31 - 1, dropped
        order = np.arange(cn)[::-1] if reverse else np.arange(cn)
        queries.append({"ids": keep.astype(np.uint32), "poses": poses[keep], "n_cand": np.array([cn], np.int32),
                        "cand_frame": frame[order][None], "score": score[order][None], "rel_pose": rel[order][None]})
    return ref.stack(queries)


def _ncand():
    a = with_n_cand(ref.line_batch([0, 1, 2, 50] + [1] * 60), 70)
    b = with_n_cand(ref.line_batch([0, 1, 2, 50] + [1] * 60), -1)
    c = ref.line_batch([0, 1, 2, 50] + [1] * 60)
    return ref.stack([a, b, c])


def _ncand_cn3():
    return ref.stack([with_n_cand(ref.line_batch([0, 1, 2]), 5), ref.line_batch([0, 1, 9]), with_n_cand(ref.line_batch([0, 1, 2]), 2)])


def _cn1():
    """cn = 1: n_cand 2 over a valid candidate, a valid one, a rejected one, none (the slot looks valid)"""
    return ref.stack([with_n_cand(ref.line_batch([4]), 2), ref.line_batch([4]), ref.line_batch([None]), with_n_cand(ref.line_batch([4]), 0)])


def _noisy_rot(rng, sigma):
    return cr.rot_axis_angle(rng.normal(size=3), rng.normal(0, sigma))


def hemisphere_batch(seed, nq=2, cn=32):
    """per query: eight members turned 115 .. 125 degrees about -z (four on either side of tr == 0) and X turned 300
    degrees, all 0.4 m on one side of the seed S (turned 123.5 degrees), six outers 0.4 m on the other side; bound 0.6 m,
    max_rot = pi.  S sees everything (the largest degree), the members do not see the outers.  The lowest member stands
    below S and lies before tr == 0 (branch 0, w > 0, z < 0), S behind it (z branch, w < 0)"""
    rng = np.random.default_rng(seed)
    queries = []
    for _ in range(nq):
        centre = rng.uniform(-20, 20, 3)
        lanes = rng.permutation(np.arange(2, cn))
        low, s_lane = int(lanes[:16].min()), None
        rest = [int(x) for x in lanes[:16] if x != low]
        s_lane = int(sorted(rest)[4])                                  # some members below the seed, most above
        rest.remove(s_lane)
        cands = [None] * cn
        angles = {low: 116.0}
        for lane, a in zip(rest, [117.5, 118.5, 119.2, 120.8, 122.0, 123.0, 124.5, 300.0] + [119.0, 121.0, 118.0, 122.5, 120.5, 121.5]):
            angles[lane] = a
        outers = set(rest[8:14])
        for lane, a in list(angles.items()) + [(s_lane, 123.5)]:
            R = cr.rot_axis_angle([0, 0, -1], np.deg2rad(a)) @ _noisy_rot(rng, np.deg2rad(0.2))
            side = 0.0 if lane == s_lane else (0.4 if lane in outers else -0.4)
            cands[lane] = (R, centre + np.array([side, 0, 0]) + rng.normal(0, 0.02, 3))
        b = world_batch(cands)
        b["role"] = {"low": low, "seed": s_lane, "x": rest[7], "members": [low] + rest[:8], "outers": sorted(outers)}
        queries.append(b)
    out = ref.stack(queries)
    out["roles"] = [b["role"] for b in queries]
    return out


def sum_order_batch(seed, cn=64):
    """one query: world positions near 1e5 m (the store's f32 translations, exact) with 0.1 m of noise, scores from 1 to
    1e15 (the two ends on lanes 5 and 40, which sit at the centre and so belong to the set), the agreement graph no clique (bound 0.3 m): the picks follow the degrees, not the lanes"""
    rng = np.random.default_rng(seed)
    ids = np.arange(cn, dtype=np.uint32)
    poses = np.tile(EYE12, (cn, 1))
    poses[:, 3], poses[:, 7], poses[:, 11] = 100000.0 + 3 * np.arange(cn), -200000.0 + np.arange(cn), 50000.0
    W = np.array([100050.0, -199970.0, 50002.0])
    rel = np.zeros((1, cn, 12))
    for k in range(cn):
        rel[0, k, :9] = _noisy_rot(rng, np.deg2rad(0.3)).reshape(9)
        rel[0, k, 9:] = (W - poses[k, [3, 7, 11]].astype(np.float64)) + rng.normal(0, 0.0 if k in (5, 40) else 0.1, 3)
    score = 10.0 ** rng.uniform(0, 15, (1, cn))
    score[0, 5], score[0, 40] = 1.0, 1e15
    return {"ids": ids, "poses": poses, "n_cand": np.array([cn], np.int32), "cand_frame": np.arange(cn, dtype=np.int32)[None].copy(),
            "score": score, "rel_pose": rel}


def _cluster(rng, n, cn, noise_t, centre):
    return world_batch([(_noisy_rot(rng, np.deg2rad(0.1)), centre + rng.normal(0, noise_t, 3)) for _ in range(n)], cn)


@functools.lru_cache(None)
def stale_pair():
    """two batches of nq = 5, cn = 64 (bound 0.5 m, 5 degrees).  The first: every candidate valid and agreeing, so every
    output word differs from what a query without candidates gets.  The second, at the same offsets: a query with no
    candidate, one with none valid, one with n_cand = 1, two ordinary ones"""
    rng = np.random.default_rng(31)
    first = ref.stack([_cluster(rng, 64, 64, 0.01, rng.uniform(-9, 9, 3)) for _ in range(5)])
    second = [_cluster(rng, 64, 64, 0.01, rng.uniform(-9, 9, 3)) for _ in range(5)]
    second[0] = with_n_cand(second[0], 0)
    second[1]["score"][:] = -1.0
    second[2] = with_n_cand(second[2], 1)
    second[3]["score"][0, ::3] = -1.0
    second[4] = with_n_cand(second[4], 40)
    return first, ref.stack(second)


HEMISPHERE_SEEDS = {"hemisphere_a": 11, "hemisphere_b": 12}
SUM_ORDER_SEEDS = {"sum_order_a": 21, "sum_order_b": 22}


@functools.lru_cache(None)
def cases():
    """name -> dict(batch, max_trans, max_rot, noisy)"""
    out = {}

    def add(name, batch, max_trans, max_rot, noisy=False):
        out[name] = dict(batch=batch, max_trans=max_trans, max_rot=max_rot, noisy=noisy)

    t = np.array([2.0, 0.0, -5.0])
    add("quarter_turn", world_batch([(I3, t), (RZ90, t), (C3, t), (RZ90.T, t)]), 1.0, np.pi / 2)
    add("half_turns", _half_turns(), 1.0, np.pi)
    add("three_cycles_a", _three_cycles(0), 1.0, np.pi)
    add("three_cycles_b", _three_cycles(1), 1.0, np.pi)
    add("on_bound", ref.line_batch([0, 1]), 1.0, 0.1)
    add("zero_rot", ref.line_batch([0, 1, 2, 9]), 2.0, 0.0)
    add("validity", _validity(False), 1.0, 0.1)
    add("validity_rev", _validity(True), 1.0, 0.1)
    add("ncand", _ncand(), 3.0, 0.1)
    add("ncand_cn3", _ncand_cn3(), 3.0, 0.1)
    add("cn1", _cn1(), 3.0, 0.1)
    add("isolated", ref.line_batch([0, 10, 20, 30, 40, 50, 60, 70]), 3.0, 0.1)
    add("tie", ref.line_batch([100, 0, 101, 1, 102, 2], cn=8), 3.0, 0.1)
    add("descending", _descending(), 10.0, 0.1)
    add("remaining_degree", points_batch(REMAINING_PTS, 32), 5.0, 0.1)
    add("remaining_degree_rev", points_batch(REMAINING_PTS[:1] + REMAINING_PTS[:0:-1], 32), 5.0, 0.1)
    add("full_wave", _full_wave(), 3.0, 0.1)
    add("chain_high", ref.line_batch([0] * 62 + [3, -3]), 5.0, 0.1)
    add("chain_low", ref.line_batch([3, -3] + [0] * 62), 5.0, 0.1)
    for name, seed in HEMISPHERE_SEEDS.items():
        add(name, hemisphere_batch(seed), 0.6, np.pi, noisy=True)
    for name, seed in SUM_ORDER_SEEDS.items():
        add(name, sum_order_batch(seed), 0.3, np.deg2rad(5.0), noisy=True)
    first, second = stale_pair()
    add("stale_first", first, 0.5, np.deg2rad(5.0), noisy=True)
    add("stale_second", second, 0.5, np.deg2rad(5.0), noisy=True)
    return out


CASE_GROUPS = {
    "thresholds": ("quarter_turn", "half_turns", "three_cycles_a", "three_cycles_b", "on_bound", "zero_rot"),
    "validity": ("validity", "validity_rev", "ncand", "ncand_cn3", "cn1"),
    "choice": ("isolated", "tie", "descending", "remaining_degree", "remaining_degree_rev", "full_wave", "chain_high", "chain_low"),
    "fusion": ("hemisphere_a", "hemisphere_b", "sum_order_a", "sum_order_b"),
}


# ---- knife pairs ----
KNIFE_SEED, KNIFE_NQ = 4242, 12


@functools.lru_cache(None)
def knife_source():
    return ref.planted_batch(KNIFE_NQ, 64, seed=KNIFE_SEED, noise_t=0.35)


def query_of(b, q):
    """query q of b as a batch of one"""
    return {"ids": b["ids"], "poses": b["poses"], "n_cand": b["n_cand"][q:q + 1].copy(), "cand_frame": b["cand_frame"][q:q + 1].copy(),
            "score": b["score"][q:q + 1].copy(), "rel_pose": b["rel_pose"][q:q + 1].copy()}


def place(b, lo, hi, i, j):
    """the one-query batch b with candidate lo standing at lane i and candidate hi at lane j (i < j: lo stays the lower)"""
    assert lo < hi and i < j
    order = list(range(b["score"].shape[1]))
    for src, dst in ((lo, i), (hi, j)):
        at = order.index(src)
        order[at], order[dst] = order[dst], order[at]
    assert order[i] == lo and order[j] == hi
    return permuted(b, order)


def _alone(b, i, j, d2, min_trace):
    """the pair (i, j) of the one-query batch sits on tt = d2, agrees, and no other pair lies within 1e-9 of either bound"""
    r = consensus_with(b, d2, min_trace)
    g = r["gap_d2"][0]
    return bool(g[i, j] == 0.0 and r["adj"][0, i, j] and np.count_nonzero(g <= 1e-9 * max(1.0, d2)) == 1
                and r["min_gap_tr"] > 1e-9 * max(1.0, abs(min_trace)))


@functools.lru_cache(None)
def knife_pairs(per_mutant=3, at_least=8, tries=60):
    """pairs (lo < hi) of one query (all 64 candidates counted: n_cand = 64) of knife_source() whose d2 is the square of a
    double, 0.01 < d2 < 4, well inside the trace bound, alone within 1e-9 of their d2 in every placement -> list of dicts
    q, lo, hi, d2, max_trans, flips (the arithmetic mutants under which the pair no longer agrees at tt = d2); chosen so
    that every one of those mutants flips at least per_mutant of them"""
    src = knife_source()
    min_trace = cr.thresholds(1.0, KNIFE_ROT)[1]
    found = []
    for q in np.flatnonzero(src["n_cand"] == 64):
        b = query_of(src, int(q))
        P, valid, _ = candidates_with(b, 0)
        v = np.flatnonzero(valid)
        lo, hi = np.triu_indices(v.size, 1)
        lo, hi = v[lo], v[hi]
        d2, tr = z_values(P, lo, hi)
        root = np.sqrt(d2)
        for k in np.flatnonzero((root * root == d2) & (d2 > 0.01) & (d2 < 4.0) & (tr > min_trace + 1e-6)):
            near = np.count_nonzero(np.abs(d2 - d2[k]) <= 1e-9 * max(1.0, d2[k]))
            if near == 1:
                found.append((int(q), int(lo[k]), int(hi[k]), float(d2[k]), float(root[k])))
    order = np.random.default_rng(9).permutation(len(found))[:tries]
    count = dict.fromkeys(ARITH_MUTANTS, 0)
    chosen = []
    spare = []
    for n in order:
        q, lo, hi, d2, root = found[n]
        b = query_of(src, q)
        if not all(_alone(place(b, lo, hi, i, j), i, j, d2, min_trace) for i, j in PLACEMENTS):
            continue
        P = candidates_with(b, 0)[0]
        flips = set()
        for m in ARITH_MUTANTS:
            a, c = ([hi], [lo]) if m == "roles_swapped" else ([lo], [hi])
            md2, mtr = z_values(P, np.array(a), np.array(c), _DOT3.get(m, dot3_plain))
            if not (md2[0] <= d2 and mtr[0] >= min_trace):
                flips.add(m)
        pair = dict(q=q, lo=lo, hi=hi, d2=d2, max_trans=root, flips=frozenset(flips))
        if any(count[m] < per_mutant for m in flips):
            chosen.append(pair)
            for m in flips:
                count[m] += 1
        else:
            spare.append(pair)
        if all(c >= per_mutant for c in count.values()) and len(chosen) + len(spare) >= at_least:
            break
    chosen += spare[:max(0, at_least - len(chosen))]
    return sorted(chosen, key=lambda p: (p["q"], p["lo"], p["hi"]))


@functools.lru_cache(None)
def knife_runs():
    """[(name, batch, pair, (i, j), q)]: every knife pair at every placement, once as the only query of its call (q = 0)
    and once as the last of five (q = 4; the four before it: other queries of the source); the run's max_trans is
    pair["max_trans"], its max_rot KNIFE_ROT"""
    src = knife_source()
    out = []
    for p in knife_pairs():
        fill = [query_of(src, (p["q"] + 1 + k) % KNIFE_NQ) for k in range(4)]
        for i, j in PLACEMENTS:
            b = place(query_of(src, p["q"]), p["lo"], p["hi"], i, j)
            name = "knife_q%d_%d_%d@%d_%d" % (p["q"], p["lo"], p["hi"], i, j)
            out.append((name, b, p, (i, j), 0))
            out.append((name + "_last", ref.stack(fill + [b]), p, (i, j), 4))
    return out
