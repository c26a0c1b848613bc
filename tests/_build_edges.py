"""Workloads at the edges of BuildSingleScanSTD (STDesc.cpp:174-315) and a plain restatement of it.  Plain helper module
of tests/test_build_edges.py (CPU: the restatement equals the oracle bit for bit, the workloads reach the edges, mutants
of the restatement are caught) and tests/test_gpu_build_edges.py (GPU: every form that reaches build_frames_kernel
equals the oracle on them).  No GPU and no torch here.

A family is a list of (cfg, frames): cfg the manager settings (keyword arguments of STDescManager and OracleManager),
frames a list of (xyz f32 [n, 3], label u32 [n]).  A frame the library must refuse is listed in REFUSED by its size.
"""
import itertools

import numpy as np

F32 = np.float32
BUILD_THREADS = 1024                 # SGTD_BUILD_THREADS of build_kernel.hip.h
LDS_LIMIT = 160 * 1024               # lds_limit of launch_build
SHIPPED = dict(descriptor_near_num=10, descriptor_min_len=2.0, descriptor_max_len=50.0, std_side_resolution=1.0)


def cfg_of(K=10, min_len=2.0, max_len=50.0, res=1.0):
    return dict(descriptor_near_num=K, descriptor_min_len=min_len, descriptor_max_len=max_len, std_side_resolution=res)


def tpi_of(K):
    """triplets per keypoint: the (m, n) pairs 1 <= m < n <= K - 1 (:193-194)"""
    return (K - 1) * (K - 2) // 2


def parts_of(K):
    """threads that share a keypoint in the kernel's k-NN stage"""
    return 4 if 3 * K <= tpi_of(K) else 1


def f32_step(x, k=1):
    """the f32 value k steps above (k < 0: below) x"""
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf))
    return x


# ---- the launch's size rules (build_lds_bytes / launch_build) ------------------------------------------------------
def lds_bytes(n, K, lds_dedup):
    tpi = tpi_of(K)
    max_t = n * tpi
    words = (max_t + 31) // 32
    slots = 64
    while slots < max_t + 1:
        slots *= 2
    up = (lambda v: (v + 15) & ~15)
    b = n * 16 + up(n * K * 2) + up(tpi * 2) + up(words * 4) + up((words + 1) * 4)
    return b + (max_t * 8 + slots * 4 if lds_dedup else 0)


def lds_switch(K):
    """the largest n whose dedup tables live in LDS"""
    n = K
    while lds_bytes(n + 1, K, True) <= LDS_LIMIT:
        n += 1
    return n


def largest_n(K):
    """the largest n the global form accepts"""
    n = lds_switch(K)
    while lds_bytes(n + 1, K, False) <= LDS_LIMIT:
        n += 1
    return n


# ---- the restatement ---------------------------------------------------------------------------------------------
SIDE_ENDS = ((0, 1), (0, 2), (1, 2))   # a = |p1 p2|, b = |p1 p3|, c = |p3 p2| (:198-203) as vertex pairs of (p1, p2, p3)


def knn(x, K, ties_high=False, self_first=False):
    """the K nearest of every point, itself included (:191): f32 ((dx*dx) + dy*dy) + dz*dz, ascending, equal distances
    in index order.  -> (idx [n, K], d2 [n, K + 1]: one more distance than neighbours, for the bookkeeping)"""
    n = len(x)
    idx = np.zeros((n, K), np.int64)
    d2k = np.full((n, K + 1), np.inf, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i0 in range(0, n, 256):
            d = x[i0:i0 + 256, None, :] - x[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            if ties_high:
                o = (n - 1) - np.argsort(d2[:, ::-1], axis=1, kind="stable")
            else:
                o = np.argsort(d2, axis=1, kind="stable")
            kk = min(K + 1, n)
            d2k[i0:i0 + len(o), :kk] = np.take_along_axis(d2, o[:, :kk], axis=1)
            o = o[:, :K]
            if self_first:
                for r in range(len(o)):
                    row = [i0 + r] + [j for j in o[r].tolist() if j != i0 + r]
                    o[r] = row[:K]
            idx[i0:i0 + len(o)] = o
    return idx, d2k


class RefBuild:
    """the descriptors of one frame and how every triplet was decided"""
    FIELDS = ("side", "angle", "center", "vertex", "label", "frame", "node_id")


def ref_build(xyz, label, cfg, frame_id=0, mutant=None):
    """BuildSingleScanSTD (STDesc.cpp:174-315) of one frame.  mutant: one named deviation (MUTANTS), for the
    sensitivity tests."""
    K, min_len, max_len = cfg["descriptor_near_num"], cfg["descriptor_min_len"], cfg["descriptor_max_len"]
    scale = 1.0 / cfg["std_side_resolution"]                                      # :178
    x = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    lab = np.ascontiguousarray(label, np.uint32)
    n = len(x)
    out = RefBuild()
    out.n_kp, out.K = n, K
    # per triplet t = i * tpi + r: raw sides (a, b, c), 0 dropped by the filter / 1 loses its key / 2 emitted
    out.raw, out.state, out.key, out.claims = [], [], [], {}
    pairs = [(m, q) for m in range(1, K - 1) for q in range(m + 1, K)]            # :193-194
    emitted = []                                                                  # (t, a, b, c, iA, iB, iC, i, m, q)
    if n >= K:                                                                    # (fewer than K points: no descriptors)
        nn, out.d2 = knn(x, K, ties_high=mutant == "ties_high", self_first=mutant == "self_first")
        out.nn = nn
        # every side among a point's neighbours at once: f32 differences, squared and summed in f64 (:198-203)
        d = (x[nn][:, :, None, :] - x[nn][:, None, :, :]).astype(np.float64)
        sides = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).tolist()
        ge = mutant == "filter_ge"
        t = -1
        for i in range(n):
            S = sides[i]
            for m, q in pairs:
                t += 1
                v = (i, int(nn[i, m]), int(nn[i, q]))                            # p1, p2, p3 (:195-197)
                a, b, c = S[0][m], S[0][q], S[q][m]                              # |p1 p2|, |p1 p3|, |p3 p2|
                out.raw.append((a, b, c))
                if ge:
                    drop = any(s >= max_len for s in (a, b, c)) or any(s <= min_len for s in (a, b, c))
                else:
                    drop = a > max_len or b > max_len or c > max_len or a < min_len or b < min_len or c < min_len   # :204
                if drop:
                    out.state.append(0)
                    out.key.append(None)
                    continue
                # the three swaps (:218-241) on (length, the side's two vertices)
                s = [(a, SIDE_ENDS[0]), (b, SIDE_ENDS[1]), (c, SIDE_ENDS[2])]
                for step, (lo, hi) in enumerate(((0, 1), (1, 2), (0, 1))):
                    if s[lo][0] > s[hi][0] or (mutant == "swap%d_ge" % (step + 1) and s[lo][0] == s[hi][0]):
                        s[lo], s[hi] = s[hi], s[lo]
                a, b, c = s[0][0], s[1][0], s[2][0]
                if mutant == "key_f64":
                    key = (int(a * 1000), int(b * 1000), int(c * 1000))
                else:                                                             # through a float (:244-248)
                    key = (int(F32(a * 1000)), int(F32(b * 1000)), int(F32(c * 1000)))
                out.key.append(key)
                out.claims.setdefault(key, []).append(t)
                if len(out.claims[key]) > 1 and mutant != "last_wins":            # :249-251
                    out.state.append(1)
                    continue
                out.state.append(2)
                # A: the vertex shared by the shortest and the middle side, B: shortest and longest, C: middle and
                # longest (:253-291)
                common = (lambda u, w: v[(set(u[1]) & set(w[1])).pop()])
                row = (t, a, b, c, common(s[0], s[1]), common(s[0], s[2]), common(s[1], s[2]), i, m, q)
                if mutant == "last_wins" and len(out.claims[key]) > 1:
                    old = out.claims[key][-2]
                    out.state[old] = 1
                    emitted = [e for e in emitted if e[0] != old]
                emitted.append(row)
    out.state = np.array(out.state, np.int8)
    out.t = np.array([e[0] for e in emitted], np.int64)
    E = len(emitted)
    a, b, c = (np.array([e[k] for e in emitted], np.float64) for k in (1, 2, 3))
    iA, iB, iC = (np.array([e[k] for e in emitted], np.int64) for k in (4, 5, 6))
    out.n = E
    out.side = np.stack([scale * a, scale * b, scale * c], 1).reshape(E, 3)        # :298
    with np.errstate(all="ignore"):
        if mutant == "assoc":
            ang = [np.abs(((b * b - a * a) + c * c) / (2 * b * c)), np.abs(((c * c - b * b) + a * a) / (2 * a * c)),
                   np.abs(((a * a - c * c) + b * b) / (2 * a * b))]
        else:                                                                     # :299-301
            ang = [np.abs((b * b + c * c - a * a) / (2 * b * c)), np.abs((a * a + c * c - b * b) / (2 * a * c)),
                   np.abs((a * a + b * b - c * c) / (2 * a * b))]
    out.angle = np.stack(ang, 1).reshape(E, 3)
    xd = x.astype(np.float64)
    A, B, C = xd[iA].reshape(E, 3), xd[iB].reshape(E, 3), xd[iC].reshape(E, 3)
    out.center = (A + (B + C)) / 3 if mutant == "assoc" else (A + B + C) / 3      # :296
    out.vertex = np.concatenate([A, B, C], 1).reshape(E, 9)
    # vertex_attached_ holds the u32 label as a double (:256); (int) of it is what the table uses (:158-160)
    out.label = np.stack([lab[iA], lab[iB], lab[iC]], 1).astype(np.float64).astype(np.int32).reshape(E, 3)
    out.frame = np.full(E, frame_id, np.uint32)                                   # :305
    out.node_id = np.array([e[7:10] for e in emitted], np.int32).reshape(E, 3)    # :302
    return out


# mutant -> the family that must catch it.  "self_first" (a keypoint forced to rank 0 of its own neighbours) is kept as
# a mutant that CANNOT be caught: copies of a point have the same neighbour list, so every triangle of a higher copy is
# found first, with the same key, by the lowest copy, whose own index is at rank 0 anyway.
EQUIVALENT_MUTANTS = ("self_first",)
MUTANTS = {
    "filter_ge": "limits", "swap1_ge": "equal_sides", "swap2_ge": "equal_sides", "swap3_ge": "equal_sides",
    "key_f64": "milli", "last_wins": "milli", "ties_high": "ties", "assoc": "extras",
}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def field_bits_equal(a, b):
    """every element the same bits; the one exception: two NaNs are equal whatever their sign and payload.  Arrays of
    different float widths (vertex: f32 on the device, f64 in the reference) are compared as f64: the widening is exact
    and keeps the sign of a zero."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype != b.dtype:
        if a.dtype.kind != "f" or b.dtype.kind != "f":
            return a.dtype.kind in "iu" and b.dtype.kind in "iu" and bool(np.array_equal(a.astype(np.int64), b.astype(np.int64)))
        a, b = a.astype(np.float64), b.astype(np.float64)
    same = _bits(a) == _bits(b)
    if a.dtype.kind == "f":
        same = same | (np.isnan(a) & np.isnan(b))
    return bool(np.all(same))


def desc_bits_equal(a, b, fields=RefBuild.FIELDS):
    """'' if the two descriptor sets are bit-identical, else what differs"""
    if a.n != b.n:
        return "n: %d != %d" % (a.n, b.n)
    for f in fields:
        x, y = np.asarray(getattr(a, f))[:a.n], np.asarray(getattr(b, f))[:b.n]
        if not field_bits_equal(x, y):
            bad = np.nonzero(np.any(np.atleast_2d((x.astype(np.float64) != y.astype(np.float64)).reshape(a.n, -1)), axis=1))[0]
            return "%s differs (first rows %s of %d)" % (f, bad[:5].tolist(), a.n)
    return ""


# ---- workloads ---------------------------------------------------------------------------------------------------
def _frame(pts, labels=None):
    pts = np.asarray(pts, F32).reshape(-1, 3)
    if labels is None:
        labels = 3 + np.arange(len(pts)) % 9
    return pts, np.asarray(labels, np.uint32)


def _tri_frames(tris, labels=(3, 7, 11)):
    """three points per frame in all six index orders"""
    out = []
    for tri in tris:
        tri = np.asarray(tri, F32).reshape(3, 3)
        for perm in itertools.permutations(range(3)):
            out.append(_frame(tri[list(perm)], [labels[k] for k in perm]))
    return out


def _along(ax, v, w, u=(0.0, 0.0)):
    """a triangle with one side of length v along axis ax from the origin plane, the third point w = (along, across);
    u shifts all three points in the other two axes (differences stay exact)"""
    p = np.zeros((3, 3), F32)
    o = [k for k in range(3) if k != ax]
    p[1, ax] = v
    p[2, ax], p[2, o[0]] = w
    p[:, o[0]] += F32(u[0])
    p[:, o[1]] += F32(u[1])
    return p


def limits():
    """K = 3, three points per frame: one triangle per frame with a side at a limit or one f32 step of a coordinate
    inside / outside it"""
    out = []
    shifts = ((0.0, 0.0), (1.0, 2.0), (3.0, 1.0), (2.0, 3.0))
    for min_len, max_len, third_min, third_max in ((2.0, 50.0, (1.0, 3.0), (25.0, 30.0)),
                                                   (1.1, 30.3, (0.5, 2.0), (15.0, 17.0)),
                                                   (5.0, 2097.125, (2.0, 6.0), (1000.0, 1500.0))):
        frames = []
        for lim, third in ((min_len, third_min), (max_len, third_max)):
            for k in (-1, 0, 1):
                for ax in range(3):
                    for u in shifts:
                        frames.append(_frame(_along(ax, f32_step(lim, k), third, u), (3, 7, 11)))
        out.append((cfg_of(3, min_len, max_len), frames))
    # right triangles whose hypotenuse is the limit: 3-4-5 at min_len 5, 25-60-65 at max_len 65, 30-40-50 at 50
    for min_len, max_len, legs, which in ((5.0, 65.0, (3.0, 4.0), "min"), (5.0, 65.0, (25.0, 60.0), "max"), (2.0, 50.0, (30.0, 40.0), "max")):
        frames = []
        for k in (-1, 0, 1):
            for ax in range(3):
                for u in shifts[:3]:
                    o = [j for j in range(3) if j != ax]
                    p = np.zeros((3, 3), F32)
                    p[1, ax] = legs[0]
                    p[2, o[0]] = f32_step(legs[1], k)
                    p[:, o[1]] += F32(u[0])
                    frames.append(_frame(p, (3, 7, 11)))
        out.append((cfg_of(3, min_len, max_len), frames))
    # two sides at max_len from one point: the limit is then also |p1 p2|, the nearer neighbour's side
    out.append((cfg_of(3, 2.0, 50.0), _tri_frames([[[0, 0, 0], [50, 0, 0], [30, 40, 0]], [[1, 2, 0], [1, 2, 50], [1, 32, 40]]])))
    out.append((cfg_of(3, 5.0, 65.0), _tri_frames([[[0, 0, 0], [65, 0, 0], [39, 52, 0]], [[0, 3, 0], [0, 3, 65], [52, 3, 39]]])))
    return out


def _near_tie_triangles():
    """isosceles triangles a hair from equilateral, whose base and legs have the same f32 squared length: the k-NN
    order is the index order, so the longer side can come first and the first swap (:218) fires"""
    out = []
    for i in range(400):
        s = F32(1.5 + i / 64.0)
        h = F32(np.sqrt(3.0) * float(s))
        base2 = F32(F32(2 * s) * F32(2 * s))
        leg2 = F32(F32(s * s) + F32(h * h))
        base, leg = 2.0 * float(s), float(np.sqrt(float(s) ** 2 + float(h) ** 2))
        if base2 == leg2 and base != leg:
            out.append(np.array([[-s, 0, 0], [s, 0, 0], [0, h, 0]], F32))
    return out


KINDS = ("equilateral", "two_short_equal", "two_long_equal", "right_isosceles")


def kind_of(a, b, c):
    """of sorted sides"""
    if a == b == c:
        return "equilateral"
    if a == b:
        return "right_isosceles" if abs(a * a + b * b - c * c) < 1e-9 * c * c else "two_short_equal"
    return "two_long_equal" if b == c else None


def equal_sides():
    """K = 3, three points per frame, every index order, a label per vertex"""
    tris = []
    for s in (2.0, 3.0, 5.5):
        tet = np.array([[0, 0, 0], [s, s, 0], [s, 0, s], [0, s, s]], F32)
        for pick in itertools.combinations(range(4), 3):
            tris.append(tet[list(pick)])                                          # equilateral, side s * sqrt(2)
        tris.append([[-4 * s / 2, 0, 0], [4 * s / 2, 0, 0], [0, 1.5 * s, 0]])   # legs 2.5 s, base 4 s
        tris.append([[-0.75 * s, 0, 0], [0.75 * s, 0, 0], [0, 0, 2 * s]])       # base 1.5 s, the two long sides equal
        tris.append([[0, 0, 0], [s, 0, 0], [0, s, 0]])                           # right isosceles
        tris.append([[1, 1, 0], [1, 1, s], [1, 1 + s, 0]])
    return [(cfg_of(3, 0.5, 50.0), _tri_frames(tris)),
            (cfg_of(3, 0.5, 50.0), _tri_frames(_near_tie_triangles()[:12]))]


def flipping_sides(lo=4001, hi=8000):
    """f32 values s with int(f32(s * 1000)) != int(s * 1000): the millimetre count N they round up to"""
    out = []
    for N in range(lo, hi):
        s = F32(N / 1000.0)
        if float(s) * 1000 >= N:
            s = f32_step(s, -1)
        if int(F32(float(s) * 1000)) == N and int(float(s) * 1000) == N - 1:
            out.append((N, s))
    return out


def _milli_key(s):
    return int(F32(float(s) * 1000))


def milli():
    """K = 3; two right triangles (legs along x and y) per frame, the second 50 m up the z axis and at the higher
    indices.  Legs and hypotenuses are chosen so that the pair shares a key (the first wins), lies less than 1 mm apart
    across a key boundary (both kept), or is decided differently by an f64 truncation of the key."""
    frames = []

    def pair(l1, l2):
        p = np.zeros((6, 3), F32)
        p[1, 0], p[2, 1] = l1
        p[3:, 2] = 50.0
        p[4, 0], p[5, 1] = l2
        return _frame(p, (3, 4, 5, 6, 7, 8))

    def hyp_key(l):
        return _milli_key(np.sqrt(float(F32(l[0])) ** 2 + float(F32(l[1])) ** 2))
    for base in range(3, 15):
        x, y = float(base) + 0.0001, float(base) + 1.0002
        for dx, dy in ((0.0004, 0.0003), (0.0002, 0.0005)):                       # same millimetres, other triangle
            frames.append(pair((x, y), (x + dx, y + dy)))
        for dx, dy in ((-0.0004, 0.0), (0.0, -0.0005)):                           # across a millimetre boundary
            frames.append(pair((x, y), (x + dx, y + dy)))
    n_flip = 0
    for N, s in flipping_sides():
        if n_flip >= 24:
            break
        y = 9.3337
        above, below = N / 1000.0 + 0.0002, N / 1000.0 - 0.0003
        if not (hyp_key((s, y)) == hyp_key((above, y)) == hyp_key((below, y))):
            continue
        frames.append(pair((s, y), (above, y)))                                   # one key as f32, two as f64
        frames.append(pair((s, y), (below, y)))                                   # two keys as f32, one as f64
        n_flip += 1
    return [(cfg_of(3, 0.5, 50.0), frames)]


def _lattice(shape, spacing=2.0, perm_seed=None):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, len(shape))
    pts = np.zeros((len(g), 3), F32)
    pts[:, :len(shape)] = g * np.asarray(spacing)
    if perm_seed is not None:
        pts = pts[np.random.default_rng(perm_seed).permutation(len(pts))]
    return _frame(pts)


def loop_frame(n, seed):
    """n points on a circle with jittered gaps: every point's two nearest are its neighbours on the circle, so with
    K = 3 the n triangles are n different ones"""
    rng = np.random.default_rng(seed)
    gaps = 1.0 + 0.8 * rng.random(n)
    ang = np.cumsum(gaps) / gaps.sum() * 2 * np.pi
    r = gaps.sum() / (2 * np.pi)
    pts = np.stack([r * np.cos(ang), r * np.sin(ang), 0.4 * rng.random(n)], 1)       # (z: a third number in every key)
    return _frame(pts[rng.permutation(n)])


FULL_TABLES = ((3, 63), (3, 127), (3, 1023), (4, 21), (4, 85), (4, 341), (7, 17), (7, 273), (8, 195), (16, 39))


def contention():
    out = [(cfg_of(10, 2.0, 50.0), [_lattice((8, 8)), _lattice((16, 16)), _lattice((32, 31)), _lattice((5, 5, 5)),
                                    _lattice((10, 10, 10)), _lattice((10, 10, 10), perm_seed=5)])]
    for K, n in FULL_TABLES:          # T = n * tpi = 2^k - 1: the dedup table has T + 1 slots
        if K == 3:
            fr = loop_frame(n, 100 + n)
        else:
            rng = np.random.default_rng(1000 * K + n)
            fr = _frame(30.0 * rng.random((n, 3)))
        out.append((cfg_of(K, 0.0, 2000.0), [fr]))
    return out


def quarter_of(j, n):
    return max(q for q in range(4) if n * q // 4 <= j)


def ties():
    out = []
    for K in (8, 9, 10, 12, 16):
        frames = [_lattice((12, 12), perm_seed=K), _lattice((6, 6, 6), perm_seed=K + 1), _lattice((17, 16), perm_seed=K + 2)]
        if K == 10:
            frames.append(_lattice((20, 15), perm_seed=3))                       # 300 keypoints: two k-NN passes, global dedup
            rng = np.random.default_rng(77)
            for copies in (2, K, K + 3):
                for low in (True, False):
                    pts = (20.0 * rng.random((60, 3))).astype(F32)
                    at = np.arange(copies) * 2 if low else 59 - np.arange(copies) * 3
                    pts[at] = pts[30]
                    frames.append(_frame(pts))
        out.append((cfg_of(K, 0.5, 50.0), frames))
    return out


def random_frame(n, seed, K=10):
    """n uniform points, about K of them within 8 m of any; redrawn (seed + 1000, ...) until free of k-NN ties"""
    from sgtd_amd import synth
    side = 8.0 * max(n / max(K, 1), 1.0) ** (1.0 / 3.0)
    while True:
        rng = np.random.default_rng(seed)
        pts = (side * rng.random((n, 3))).astype(F32)
        if n < 2 or not synth.has_knn_ties(pts, min(K, n - 1)):
            return _frame(pts, rng.integers(3, 12, n))
        seed += 1000


SHAPE_KS = (3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 16)
SWITCH_KS = (10, 12, 16)
REFUSED = {K: largest_n(K) + 1 for K in SWITCH_KS}


def shape_sizes(K):
    ns = [K - 1, K, K + 1] + ([256, 257, 513] if parts_of(K) == 4 else [1024, 1025])
    if K in SWITCH_KS:
        s = lds_switch(K)
        ns += [s - 1, s, s + 1, largest_n(K)]
    return ns


def shapes(largest=True):
    """tie-free random frames at every network size, pass boundary and dedup form (largest=False: without the largest
    accepted frames, which cost the restatement seconds each)"""
    out = []
    for K in SHAPE_KS:
        ns = [n for n in shape_sizes(K) if largest or K not in SWITCH_KS or n != largest_n(K)]
        out.append((cfg_of(K, 0.5, 50.0), [random_frame(n, 10000 * K + n, K) for n in ns]))
    return out


def refused_frame(K):
    return random_frame(REFUSED[K], 7, K)


def batch_of(frames):
    """frames -> (xyz [total, 3], label [total], kp_off [F + 1])"""
    off = np.concatenate([[0], np.cumsum([len(f[0]) for f in frames])]).astype(np.int64)
    xyz = np.concatenate([f[0] for f in frames] + [np.zeros((0, 3), F32)]).astype(F32)
    lab = np.concatenate([f[1] for f in frames] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return xyz, lab, off


MIXED_K = 10


def mixed_batches():
    """ragged batches (one launch each): empty frames, n < K, n = K, about 200, one past the LDS switch; every frame
    its own points.  The second and third have more frames than any grid the launch chooses."""
    K, big = MIXED_K, lds_switch(MIXED_K) + 1
    small = (0, 3, K - 1, K, K + 1, 12, 25, 40)
    b1 = [0, 5, K, 200, big, 9, K, 11, 0, 150, big - 2, K + 1, 64, 0, 257, 33, K, 199, 3, 201]
    b2 = [small[(7 * i) % len(small)] for i in range(1100)]
    for i in range(50, 1100, 100):
        b2[i] = 190 + i // 100
    b2[555] = big
    b3 = [small[(5 * i) % len(small)] for i in range(600)]
    for i in range(30, 600, 60):
        b3[i] = 180 + i // 60
    out = []
    for b, sizes in enumerate((b1, b2, b3)):
        out.append((cfg_of(K, 0.5, 50.0), [random_frame(n, 500000 * (b + 1) + 7 * i, K) for i, n in enumerate(sizes)]))
    return out


def degenerate():
    """descriptor_min_len = 0: duplicate points (zero sides, NaN angles), collinear points and right angles (cosines of
    exactly 1 and 0)"""
    out = []
    for K in (4, 10):
        frames = []
        for seed in range(3):
            fr = _lattice((6, 6) if K == 4 else (7, 7), (3.0, 4.0), perm_seed=seed)     # 3-4-5: cosines of exactly 0
            pts = fr[0].copy()
            pts[[1, 7, 9]] = pts[3]                                               # four copies
            pts[12] = pts[5]
            frames.append(_frame(pts))
        frames.append(_frame([[k * 1.5, 0, 0] for k in range(K + 4)]))           # collinear
        if K == 4:                         # right triangles with whole sides, 200 m apart: a cosine of 0 per key
            legs = ((3, 4), (6, 8), (5, 12), (8, 15), (9, 12), (7, 24), (20, 21), (12, 16), (15, 20), (10, 24))
            frames.append(_frame([p for k, (u, w) in enumerate(legs) for p in ([0, 0, 200 * k], [u, 0, 200 * k], [0, w, 200 * k], [0, 0, 200 * k + 1])]))
        frames.append(_frame([[0, 0, 0]] * (K + 2)))                             # one point, K + 2 times
        out.append((cfg_of(K, 0.0, 50.0), frames))
    return out


def extras():
    """labels up to 2^31 - 1 (beyond: outside the contract, include/sgtd_accel.h); coordinates whose f32 squared
    distance overflows (descriptor_min_len > 0: the kernel's empty k-NN slots only make triangles that the filter drops
    or that lose their key to the real one)"""
    rng = np.random.default_rng(9)
    pts = (12.0 * rng.random((40, 3))).astype(F32)
    lab = np.array([0, 1, 15, 16, 17, 255, 256, 4095, 65535, 65536, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 31 - 2, 2 ** 30] * 3, np.uint32)[:40]
    far = (10.0 * rng.random((16, 3))).astype(F32)
    far[12:] += F32(3e19)
    few = (6.0 * rng.random((14, 3))).astype(F32)
    few[5:] *= F32(1e19)
    few[5:] += F32(2e19)
    return [(cfg_of(10, 0.5, 50.0), [_frame(pts, lab), _frame(far), _frame(few)])]


FAMILIES = {"limits": limits, "equal_sides": equal_sides, "milli": milli, "contention": contention, "ties": ties,
            "shapes": shapes, "mixed_batches": mixed_batches, "degenerate": degenerate, "extras": extras}
_CACHE = {}


def family(name):
    if name not in _CACHE:
        _CACHE[name] = FAMILIES[name]()
    return _CACHE[name]
