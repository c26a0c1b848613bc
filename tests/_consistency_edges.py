"""Worlds at the edges of sgtd_consistent_loops (consistency_kernels.hip.h) and a restatement of its rule with replaceable
parts.  Plain helper module of tests/test_consistency_edges.py (CPU: every mutant below changes the expected result on the
world named for it, the fast reference helpers equal the plain ones, every world's precondition holds) and
tests/test_gpu_consistency_edges.py (GPU: every form of the call equals the rule on them, bit for bit).

Two kinds of edge:
  * sizes.  cons_count_kernel's word loop and grid stride take a second step, and cons_select_kernel's block scan leaves
    wave 0, only beyond 4096 edges: N_BIG = max(4096, 16 * n_cus) + 65 edges (4161 on 256 CUs: 66 row words, the last
    holding one bit; more rows than the count pass has waves).  The big worlds are integer translations, whose arithmetic
    is exact and whose answer is analytic, and one noisy world judged by sampled rows.
  * the bitwise rule.  knife_pairs() are pairs of a noisy world whose d2 is the exact square of a double: with
    max_trans = sqrt(d2) the library's tt = max_trans * max_trans is d2 itself, so the pair sits ON the bound and is
    consistent through <=; a d2 one ulp larger (roles swapped, a sum re-associated, a product fused) is not.

The mutants (test_consistency_edges.py asserts each on the worlds named here):
  roles_swapped   the pair decided as (hi, lo)                                   knife_pairs
  sum_right       a + (b + c) in the dot products                                knife_pairs
  contracted      each product after the first fused into the add that follows   knife_pairs
                  (exact fused multiply-add through fractions.Fraction)
  tie_high        the highest index among equal degrees                          tie_far, tie_split, groups_big
  total_degree    round 0's degree used in later rounds                          remaining_degree
  words_64        d(u) counted over the first 64 row words only                  groups_big, noisy_big
  stride_once     rows u >= n_waves never counted                                tie_far, tie_split
  no_wave_prefix  the shortcut's positions without the waves before              groups_big
  wave0_total     the new |P| from wave 0's words only                           chain_big, hub_then_clique_big
hub_then_clique_big cannot show no_wave_prefix: its shortcut's P lies in words >= 64 alone, which one wave owns at N_BIG,
and the waves before it hold nothing, so the prefix is 0 by right.  groups_big is the world for it."""
import functools
from fractions import Fraction

import numpy as np

import _consistency_ref as cr

N_CUS_MI355X = 256
SMALL_CHAINS = (17, 18, 49, 50, 113, 114)          # 16, 17, 48, 49, 112, 113 rounds: on and one past the host's groups
MAX_EDGES = 32768                                  # SGTD_MAX_LOOP_EDGES
KNIFE_ROT = np.deg2rad(5.0)
PLACEMENTS = ((5, 9), (5, 70), (60, 130), (63, 64), (127, 128), (3, 199))
PAIR_MUTANTS = ("roles_swapped", "sum_right", "contracted")
MUTANT_WORLDS = {
    "roles_swapped": ("knife_pairs",), "sum_right": ("knife_pairs",), "contracted": ("knife_pairs",),
    "tie_high": ("tie_far", "tie_split", "groups_big"), "total_degree": ("remaining_degree",),
    "words_64": ("groups_big", "noisy_big"), "stride_once": ("tie_far", "tie_split"),
    "no_wave_prefix": ("groups_big",), "wave0_total": ("chain_big", "hub_then_clique_big"),
}
BIG_ONLY_MUTANTS = ("words_64", "stride_once", "no_wave_prefix", "wave0_total")


def n_big(n_cus=N_CUS_MI355X):
    return max(4096, 16 * n_cus) + 65


def n_waves(n, n_cus=N_CUS_MI355X):
    """the waves of cons_count_kernel's launch: 4 per workgroup, min(ceil(n / 4), 4 * n_cus) workgroups"""
    return 4 * min((n + 3) // 4, 4 * n_cus)


def greedy_parts(mutant, n, n_cus=N_CUS_MI355X):
    """cr.greedy_fast's `parts` for a mutant of the choice, for n edges on a device of n_cus CUs"""
    return {"tie_high": dict(tie_high=True), "total_degree": dict(total_degree=True), "words_64": dict(col_limit=cr.WAVE_BITS),
            "stride_once": dict(row_limit=n_waves(n, n_cus)), "no_wave_prefix": dict(no_wave_prefix=True),
            "wave0_total": dict(psize_limit=cr.WAVE_BITS)}[mutant]


# ---- the pair rule with a replaceable dot product ----
def dot3_plain(a0, b0, a1, b1, a2, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def dot3_sum_right(a0, b0, a1, b1, a2, b2):
    return a0 * b0 + (a1 * b1 + a2 * b2)


_fma = np.frompyfunc(lambda a, b, c: float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))), 3, 1)


def fma(a, b, c):
    """a * b + c rounded once (finite inputs), elementwise"""
    return np.asarray(_fma(a, b, c), dtype=np.float64)


def dot3_contracted(a0, b0, a1, b1, a2, b2):
    return fma(a2, b2, fma(a1, b1, a0 * b0))


def inv_with(X, dot3):
    R, t = X
    Ri = np.swapaxes(R, -1, -2).copy()
    ti = np.empty_like(t)
    for r in range(3):
        ti[..., r] = -dot3(Ri[..., r, 0], t[..., 0], Ri[..., r, 1], t[..., 1], Ri[..., r, 2], t[..., 2])
    return Ri, ti


def mul_with(X, Y, dot3):
    Xr, Xt = X
    Yr, Yt = Y
    shape = np.broadcast(Xr, Yr).shape
    R = np.empty(shape, np.float64)
    t = np.empty(shape[:-1], np.float64)
    for r in range(3):
        for c in range(3):
            R[..., r, c] = dot3(Xr[..., r, 0], Yr[..., 0, c], Xr[..., r, 1], Yr[..., 1, c], Xr[..., r, 2], Yr[..., 2, c])
        t[..., r] = dot3(Xr[..., r, 0], Yt[..., 0], Xr[..., r, 1], Yt[..., 1], Xr[..., r, 2], Yt[..., 2]) + Xt[..., r]
    return R, t


def _take(X, idx):
    return X[0][idx], X[1][idx]


def pair_values(w, first, second, dot3=dot3_plain):
    """(d2, tr) of the pairs (first[k], second[k]) of world w, `first` in the role of the lower index, with every dot
    product of the rule (P = mul(B, T) and the inverses included) taken by dot3.  Every frame of w has a pose."""
    first, second = np.asarray(first, np.int64), np.asarray(second, np.int64)
    B, A, T = cr.from_rows34(w["poses"][w["frame_b"]]), cr.from_rows34(w["poses"][w["frame_a"]]), cr.from_rel(w["rel_pose"])
    used = np.unique(np.concatenate([first, second]))
    at = np.full(len(w["frame_b"]), -1)
    at[used] = np.arange(used.size)
    A = _take(A, used)
    P = mul_with(_take(B, used), _take(T, used), dot3)
    iP, iA = inv_with(P, dot3), inv_with(A, dot3)
    lo, hi = at[first], at[second]
    U = mul_with(_take(iP, lo), _take(P, hi), dot3)
    V = mul_with(_take(iA, hi), _take(A, lo), dot3)
    Zr, Zt = mul_with(U, V, dot3)
    d2 = dot3(Zt[..., 0], Zt[..., 0], Zt[..., 1], Zt[..., 1], Zt[..., 2], Zt[..., 2])
    tr = (Zr[..., 0, 0] + Zr[..., 1, 1]) + Zr[..., 2, 2]
    return d2, tr


def pair_mutant_values(w, lo, hi, mutant):
    if mutant == "roles_swapped":
        return pair_values(w, hi, lo)
    return pair_values(w, lo, hi, {"sum_right": dot3_sum_right, "contracted": dot3_contracted}[mutant])


# ---- knife pairs ----
@functools.lru_cache(None)
def knife_world():
    """200 edges, parity_world's recipe: 140 true loops with 0.35 m of noise, 60 wrong ones, 12 of them aliases"""
    return cr.planted_world(140, 60, 12, seed=1200, n_frames=400, noise_t=0.35)


@functools.lru_cache(None)
def knife_pairs(n_candidates=400, per_mutant=3, at_least=8):
    """pairs (lo < hi) of knife_world() whose d2 is the square of a double, 0.01 < d2 < 4, well inside the trace bound and
    alone within 1e-9 of their d2 -> list of dicts lo, hi, d2, max_trans, flips (the pair mutants under which the pair is
    no longer consistent at tt = d2); chosen so that every pair mutant flips at least per_mutant of them"""
    w = knife_world()
    n = len(w["frame_b"])
    lo, hi = np.triu_indices(n, 1)
    d2, tr = pair_values(w, lo, hi)
    min_trace = cr.thresholds(1.0, KNIFE_ROT)[1]
    with np.errstate(invalid="ignore"):
        root = np.sqrt(d2)
    cand = np.flatnonzero((root * root == d2) & (d2 > 0.01) & (d2 < 4.0) & (tr > min_trace + 1e-6))
    order = np.sort(d2)
    alone = np.array([np.searchsorted(order, d2[k] + 1e-9 * max(1.0, d2[k]), "right") - np.searchsorted(order, d2[k] - 1e-9 * max(1.0, d2[k]), "left") == 1
                      for k in cand], bool)
    cand = np.random.default_rng(9).permutation(cand[alone])[:n_candidates]        # (pairs of many different edges)
    flips = [set() for _ in cand]
    for m in PAIR_MUTANTS:
        md2, mtr = pair_mutant_values(w, lo[cand], hi[cand], m)
        for k in np.flatnonzero(~((md2 <= d2[cand]) & (mtr >= min_trace))):
            flips[k].add(m)
    count = dict.fromkeys(PAIR_MUTANTS, 0)
    chosen = []
    for k in range(cand.size):
        if any(count[m] < per_mutant for m in flips[k]):
            chosen.append(k)
            for m in flips[k]:
                count[m] += 1
    for k in range(cand.size):
        if len(chosen) >= at_least:
            break
        if k not in chosen:
            chosen.append(k)
    return [dict(lo=int(lo[cand[k]]), hi=int(hi[cand[k]]), d2=float(d2[cand[k]]), max_trans=float(root[cand[k]]), flips=frozenset(flips[k]))
            for k in sorted(chosen)]


def place(w, lo, hi, i, j):
    """w with its edges permuted so that edge lo stands at index i and edge hi at index j (i < j: lo stays the lower)"""
    assert lo < hi and i < j
    order = list(range(len(w["frame_b"])))
    for src, dst in ((lo, i), (hi, j)):
        at = order.index(src)
        order[at], order[dst] = order[dst], order[at]
    assert order[i] == lo and order[j] == hi
    order = np.array(order)
    return dict(w, frame_a=w["frame_a"][order], frame_b=w["frame_b"][order], rel_pose=w["rel_pose"][order])


def knife_runs():
    """[(name, world, pair, (i, j))]: every knife pair at every placement; the run's max_trans is pair["max_trans"]"""
    return [("knife_%d_%d@%d_%d" % (p["lo"], p["hi"], i, j), place(knife_world(), p["lo"], p["hi"], i, j), p, (i, j))
            for p in knife_pairs() for i, j in PLACEMENTS]


# ---- integer translations: exact arithmetic, analytic answers ----
def shift_world(g_shift, seed=3, n_frames=None, name=None, max_trans=5.0, max_rot=0.1):
    """edge i: frame_a = i % F at a, frame_b = F + i % F at b (integer positions, identity rotations, F = n_frames or n)
    and a loop that puts the query at a + g_shift[i]: the pair (i, j) closes its cycle up to g_shift[j] - g_shift[i], exactly"""
    g_shift = np.asarray(g_shift, np.float64).reshape(-1, 3)
    n = g_shift.shape[0]
    F = n_frames or n
    rng = np.random.default_rng(seed)
    a = rng.integers(-500, 500, (F, 3)).astype(np.float64)
    b = rng.integers(-500, 500, (F, 3)).astype(np.float64)
    eye = np.broadcast_to(np.eye(3), (2 * F, 3, 3))
    poses = cr.rows34(eye, np.concatenate([a, b])).astype(np.float32)
    k = np.arange(n) % F
    rel = np.zeros((n, 12))
    rel[:, [0, 4, 8]] = 1.0
    rel[:, 9:] = a[k] - b[k] + g_shift
    return {"name": name, "ids": np.arange(2 * F, dtype=np.uint32), "poses": poses, "frame_a": k.astype(np.uint32),
            "frame_b": (F + k).astype(np.uint32), "rel_pose": rel, "shift": g_shift.astype(np.int64), "max_trans": max_trans, "max_rot": max_rot}


def shift_adjacency(w):
    """the analytic adjacency of a shift world (all edges valid): |shift_j - shift_i|^2 <= max_trans^2"""
    s = w["shift"]
    d2 = np.zeros((s.shape[0], s.shape[0]), np.int64)
    for k in range(3):
        d = s[:, k, None] - s[None, :, k]
        d2 += d * d
    adj = d2 <= int(round(w["max_trans"] * w["max_trans"]))
    np.fill_diagonal(adj, False)
    return adj


def _far(n, start=1000):
    """n isolated places, 10 apart along x from `start` on"""
    s = np.zeros((n, 3))
    s[:, 0] = start + 10 * np.arange(n)
    return s


@functools.lru_cache(None)
def chain(n, low=False):
    """a clique minus one edge, bound 5: the edge between the two highest indices (low=False: n - 1 rounds, picks 0, 1, 2,
    ...; the last index is left out) or between 0 and 1 (low=True: picks 2, 3, ..., n - 1, then 0; 1 is left out)"""
    s = np.zeros((n, 3))
    u, v = (0, 1) if low else (n - 2, n - 1)
    s[u, 0], s[v, 0] = 3.0, -3.0
    return shift_world(s, name="chain_%d_%s" % (n, "low" if low else "high"))


def chain_expect(n, low):
    """-> (in_set, degree, pick, n_set, rounds), written down"""
    in_set = np.ones(n, np.int32)
    degree = np.full(n, n - 1, np.int32)
    if low:
        degree[[0, 1]] = n - 2
        pick = np.arange(n, dtype=np.int32) - 2
        pick[0], pick[1], in_set[1] = n - 2, -1, 0
    else:
        degree[[n - 2, n - 1]] = n - 2
        pick = np.arange(n, dtype=np.int32)
        pick[n - 1], in_set[n - 1] = -1, 0
    return in_set, degree, pick, n - 1, n - 1


@functools.lru_cache(None)
def groups_big(n_cus=N_CUS_MI355X):
    """three groups of equal size, 100 apart, bound 1: by i % 3, but the last index (alone in the last row word) belongs to
    0's group in exchange for n - 3.  After the pick of 0 the shortcut takes 3, 6, ..., n - 1 from every row word"""
    n = n_big(n_cus)
    assert n % 3 == 0
    group = np.arange(n) % 3
    group[n - 1], group[n - 3] = 0, 2
    s = np.zeros((n, 3))
    s[:, 0] = 100 * group
    w = shift_world(s, name="groups_big", max_trans=1.0)
    w["group"] = group
    return w


@functools.lru_cache(None)
def hub_then_clique_big(n_cus=N_CUS_MI355X):
    """bound 5.  Hub 0 at x = 4 sees the crowd (30 edges at x = 8, indices 1 .. 30) and the clique K (the last 65 indices,
    all in row words >= 64, at x = 0); crowd and K do not see each other, the rest is isolated.  Picks: 0 (degree 95),
    then K's lowest index (d = 64 against the crowd's 29), then the shortcut over the rest of K"""
    n = n_big(n_cus)
    s = _far(n)
    s[0] = (4, 0, 0)
    s[1:31] = (8, 0, 0)
    s[n - 65:] = (0, 0, 0)
    assert n - 65 >= cr.WAVE_BITS
    return shift_world(s, name="hub_then_clique_big")


def _tie_world(n, u1, u2, name, m=20):
    """bound 5.  u1 and u2 each sit between two crowds of m that do not see each other (x = -4 and x = +4 of the hub): degree
    2 m for the two hubs, m for the crowds (indices 1 .. 4 m), 0 for the rest"""
    s = _far(n, start=10000)
    for k, u in enumerate((u1, u2)):
        x = 1000 * (k + 1)
        s[u] = (x, 0, 0)
        s[1 + 2 * m * k:1 + 2 * m * k + m] = (x - 4, 0, 0)
        s[1 + 2 * m * k + m:1 + 2 * m * (k + 1)] = (x + 4, 0, 0)
    assert 4 * m < min(u1, u2)
    w = shift_world(s, name=name)
    w["tie"] = (u1, u2)
    return w


@functools.lru_cache(None)
def tie_far(n_cus=N_CUS_MI355X):
    """the largest degree shared by two rows of the count pass's second grid-stride step, counted by different waves"""
    n = n_big(n_cus)
    nw = n_waves(n, n_cus)
    assert nw + 40 < n
    return _tie_world(n, nw + 3, nw + 40, "tie_far")


@functools.lru_cache(None)
def tie_split(n_cus=N_CUS_MI355X):
    """... by one row of the first step and one of the second"""
    n = n_big(n_cus)
    nw = n_waves(n, n_cus)
    return _tie_world(n, nw - 30, nw + 7, "tie_split")


@functools.lru_cache(None)
def chain_big(low=False, n_cus=N_CUS_MI355X):
    w = dict(chain(n_big(n_cus), low))
    w["name"] = "chain_big_%s" % ("low" if low else "high")
    return w


BIG_ANALYTIC = {"groups_big": groups_big, "hub_then_clique_big": hub_then_clique_big, "tie_far": tie_far, "tie_split": tie_split,
                "chain_big_high": lambda n_cus=N_CUS_MI355X: chain_big(False, n_cus), "chain_big_low": lambda n_cus=N_CUS_MI355X: chain_big(True, n_cus)}


@functools.lru_cache(None)
def remaining_degree():
    """25 edges, bound 5.  0 at the origin has the largest degree (16).  Of its neighbours, x (index 1, at (5, 0, 0)) has
    the largest degree (15: 0, G1 and eight more at (10, 0, 0) that 0 does not see) but only 6 inside P = adj(0); a member
    of G1 (six at (2, 0, 0)) has 12 in all and 11 inside P (G1, x, and G2: five at (-3, 0, 0)).  The rule goes on with G1's
    lowest index and ends with {0} + G1 + G2; with round 0's degrees it goes on with x and ends with {0, x} + G1"""
    pts = [(0, 0, 0), (5, 0, 0)] + [(2, 0, 0)] * 6 + [(10, 0, 0)] * 8 + [(-3, 0, 0)] * 5 + [(0, 5, 0), (0, -5, 0), (0, 0, 5), (0, 0, -5)]
    return shift_world(np.array(pts, np.float64), name="remaining_degree")


# ---- a noisy world at N_BIG ----
def parity_recipe(n, seed=None):
    """parity_world of tests/test_gpu_consistency.py: about 70 % true loops with 0.35 m of noise, the rest wrong"""
    n_out = (3 * n) // 10
    return cr.planted_world(n - n_out, n_out, n_out // 5, seed=1000 + n if seed is None else seed, n_frames=max(2 * n, 64), noise_t=0.35)


@functools.lru_cache(None)
def noisy_big(n_cus=N_CUS_MI355X):
    """parity_world's recipe at N_BIG with about 1 % of the edges invalid on the b side or in rel_pose (so that the frame_a
    and the pose_a form agree on them): w["invalid"] = {index: kind}"""
    n = n_big(n_cus)
    w = parity_recipe(n)
    ids, poses = w["ids"], w["poses"]
    fb, rel = w["frame_b"].copy(), w["rel_pose"].copy()
    hole, inf_frame, top = len(ids) + 5, len(ids) + 9, len(ids) + 12       # the stored range ends at `top`
    inf_pose = poses[0].copy()
    inf_pose[7] = np.inf
    ids = np.concatenate([ids, [inf_frame, top]]).astype(np.uint32)
    poses = np.concatenate([poses, inf_pose[None], poses[:1]])
    rng = np.random.default_rng(77)
    where = np.unique(np.concatenate([rng.choice(n - 1, 36, replace=False), [0, 63, 64, cr.WAVE_BITS - 1, cr.WAVE_BITS, cr.WAVE_BITS + 1, n - 2 - 17, n - 1]]))
    kinds = ("no_pose", "beyond_store", "beyond_u32", "nan_rel", "inf_pose", "nan_rot")
    invalid = {}
    for k, i in enumerate(where):
        kind = kinds[k % len(kinds)]
        invalid[int(i)] = kind
        if kind == "no_pose":
            fb[i] = hole
        elif kind == "beyond_store":
            fb[i] = top + 1 + k
        elif kind == "beyond_u32":
            fb[i] = 0xFFFFFFFF - k
        elif kind == "nan_rel":
            rel[i, 9 + k % 3] = np.nan
        elif kind == "inf_pose":
            fb[i] = inf_frame
        else:
            rel[i, k % 9] = np.nan
    return dict(w, name="noisy_big", ids=ids, poses=poses, frame_b=fb, rel_pose=rel, invalid=invalid, max_trans=1.0, max_rot=np.deg2rad(5.0))


def sample_rows(n, nw):
    """one row of every 64-row block, at an offset that moves through the block (every wave of the pair pass, several of
    its row steps), plus the rows at the edges of the blocks, of the count pass's grid and of the matrix"""
    rows = [min(64 * k + (7 * k + 3) % 64, n - 1) for k in range((n + 63) // 64)]
    rows += [0, 63, 64, 127, 128, nw - 1, nw, n - 2, n - 1]
    return np.unique([r for r in rows if 0 <= r < n])


def spread_rows(n, count=64):
    """`count` rows spread over the matrix the same way"""
    blocks = np.linspace(0, (n + 63) // 64 - 1, count - 4).astype(int)
    rows = [min(64 * int(k) + (7 * i + 3) % 64, n - 1) for i, k in enumerate(blocks)] + [0, 63, n - 2, n - 1]
    return np.unique(rows)


# ---- the limit ----
@functools.lru_cache(None)
def max_edges():
    """SGTD_MAX_LOOP_EDGES edges in four groups by i % 8 (1 2 3 5 | 0 4 | 6 | 7), 100 apart, bound 1, over 4096 frame
    pairs used eight times each: pick 1, then the shortcut over the rest of the first group, in every one of the 512 row
    words.  w["group"]: the group of every edge"""
    n = MAX_EDGES
    group = np.array([1, 0, 0, 0, 1, 0, 2, 3])[np.arange(n) % 8]
    s = np.zeros((n, 3))
    s[:, 0] = 100 * group
    w = shift_world(s, n_frames=4096, name="max_edges", max_trans=1.0)
    w["group"] = group
    return w


def group_rows(group):
    """the packed adjacency of edges that agree inside their group and not across: every row is its group's mask with its
    own bit cleared"""
    n = group.size
    words = (n + 63) // 64
    masks = np.zeros((int(group.max()) + 1, words * 64), np.uint8)
    masks[group, np.arange(n)] = 1
    masks = np.packbits(masks, axis=1, bitorder="little").view("<u8").astype(np.uint64)
    rows = masks[group]
    i = np.arange(n)
    rows[i, i >> 6] &= ~(np.uint64(1) << (i & 63).astype(np.uint64))
    return rows


def group_greedy(group):
    """-> (in_set, degree, pick, n_set, rounds) of such a graph, written down: the largest group, the one with the lowest
    index among equals, joins in ascending order (rounds: the pick of its first member, then the shortcut)"""
    size = np.bincount(group)
    first = np.array([np.flatnonzero(group == k)[0] for k in range(size.size)])
    best = min(range(size.size), key=lambda k: (-size[k], first[k]))
    in_set = (group == best).astype(np.int32)
    pick = np.full(group.size, -1, np.int32)
    pick[group == best] = np.arange(size[best])
    return in_set, (size[group] - 1).astype(np.int32), pick, int(size[best]), 1 if size.size == 1 else 2


# ---- the cached pose store ----
@functools.lru_cache(None)
def store_world():
    """150 noisy edges; edge 20's frame_b lies beyond the stored range until the third of store_steps() gives it a pose"""
    w = parity_recipe(150)
    fb = w["frame_b"].copy()
    fb[20] = len(w["ids"]) + 40
    return dict(w, name="store_updates", frame_b=fb, max_trans=1.0, max_rot=np.deg2rad(5.0))


def store_steps():
    """[(what, ids, poses or None)] applied in turn with set_frame_poses(ids, poses): a pose replaced, a pose forgotten,
    a pose added beyond the stored range.  The frames are b sides, so the pose_a form sees every change"""
    w = store_world()
    moved, gone, new = int(w["frame_b"][3]), int(w["frame_b"][70]), int(w["frame_b"][20])
    assert len({moved, gone, new}) == 3
    shifted = w["poses"][moved].copy()
    shifted[[3, 7]] += np.float32(0.5)
    return [("replaced", np.array([moved]), shifted[None]), ("forgotten", np.array([gone]), None),
            ("grown", np.array([new]), w["poses"][int(w["frame_b"][21])][None])]


def store_after(steps):
    """(ids, poses) of store_world()'s store after the first `steps` of store_steps()"""
    w = store_world()
    store = {int(i): p for i, p in zip(w["ids"], w["poses"])}
    for _, ids, poses in store_steps()[:steps]:
        for k, i in enumerate(ids):
            if poses is None:
                store.pop(int(i))
            else:
                store[int(i)] = poses[k]
    ids = np.array(sorted(store), np.uint32)
    return ids, np.stack([store[int(i)] for i in ids]).astype(np.float32)


def small_worlds():
    """every world below 4096 edges with its bounds: [(name, world, max_trans, max_rot)]"""
    out = [(c["name"], c, c["max_trans"], c["max_rot"]) for c in (chain(n, low) for n in SMALL_CHAINS for low in (False, True))]
    out.append(("remaining_degree", remaining_degree(), 5.0, 0.1))
    out.append(("store_updates", store_world(), 1.0, np.deg2rad(5.0)))
    name, w, p, _ = knife_runs()[0]
    out.append((name, w, p["max_trans"], KNIFE_ROT))
    return out
