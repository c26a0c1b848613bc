"""Workloads at the edges of the keypoint passes (sgtd_overlap: overlap_kernel; sgtd_align_keypoints: align_kernel over
the shared overlap_walk; sgtd_amd/csrc/overlap_kernels.hip.h, align_kernels.hip.h): the `<=` comparisons at r2 == rr, ties
within an unroll group and across tiles, NaN and inf frame coordinates, frames and queries of 0 to 65535 keypoints, the
inactive lanes of the last round, labels as 32-bit words, the summation order and the stop rule.  Plain helper module of
tests/test_keypoint_edges.py (CPU: every workload keeps its promises on the oracle's poses, and mutants of the rule are
caught) and tests/test_gpu_keypoint_edges.py (GPU: every form of the calls equals the restatements tests/_overlap_ref.py
and tests/_align_ref.py on them).

The pose of a candidate cannot be set, but it is read back to the bit, and the frame's keypoints are a setting.  So a
workload is a function of one candidate's start pose (R, t) and a seed: the builder transforms its query keypoints with
_overlap_ref.transform (x_i, the device's own f64 arithmetic) and plants the frame's f32 keypoints relative to the x_i.
Whatever depends on the start pose alone is then exact however near a threshold it sits; decisions after the first fit
depend on the device's SVD, and every planted one keeps 1e-3 m^2 (MARGIN) from its threshold.

A Workload holds the query and the frame keypoints, its runs (radius, iterations) and `promise(res)`: assertions on
res[run] = dict(before, after (dicts of _overlap_ref.KEYS), assign, n_fits, n_corr, stop) — the restatement's output or
the device's, in the same shape."""
import numpy as np

import _align_ref as al
import _overlap_ref as ov
import _refine_ref as rf

W = 256              # threads: query keypoints of one round, accumulators
TILE = 1024          # SGTD_OVERLAP_TILE
CAP = 1024           # SGTD_ALIGN_CAP
MAX_KP = 65535       # the store's and the calls' bound
MARGIN = 1e-3        # m^2: what a decision after the first fit keeps from its threshold
LABELS = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x00010001, 0x00000001, 0x3F800000, 0x00000100], np.uint32)
D = np.array([0.3, -0.2, 0.1])       # the rigid planted offset: |D| = 0.374 m, far below half the lattice spacing


def overlap_lds_bytes(max_kp):
    """overlap_kernels.hip.h: the head, the tile, the hit bytes"""
    return 1152 + min(max(max_kp, 1), TILE) * 16 + ((max(max_kp, 1) + 15) & ~15)


def align_lds_bytes(max_kp):
    """align_kernels.hip.h: the head, the tile, the hit bytes, the assignment of CAP keypoints"""
    return 9728 + min(max(max_kp, 1), TILE) * 16 + ((max(max_kp, 1) + 15) & ~15) + CAP * 4


class Workload:
    def __init__(self, name, q_xyz, q_lab, f_xyz, f_lab, runs, promise, large=False, **info):
        self.name = name
        self.q_xyz = np.ascontiguousarray(q_xyz, np.float32).reshape(-1, 3)
        self.q_lab = np.ascontiguousarray(q_lab, np.uint32).reshape(-1)
        self.f_xyz = np.ascontiguousarray(f_xyz, np.float32).reshape(-1, 3)
        self.f_lab = np.ascontiguousarray(f_lab, np.uint32).reshape(-1)
        assert len(self.q_xyz) == len(self.q_lab) <= MAX_KP and len(self.f_xyz) == len(self.f_lab) <= MAX_KP, name
        self.runs = [(float(r), int(i)) for r, i in runs]
        self.promise = promise
        self.large = large          # a 65535-keypoint side: run in one form and the sharded one
        self.info = info


# ---- planting --------------------------------------------------------------------------------------------------------
def lattice(rng, n, spacing=12.0):
    """n query keypoints on a cubic lattice of 12 m with 1 m of jitter (every pair at least 10 m apart), in random order"""
    side = max(int(np.ceil(n ** (1.0 / 3.0))), 1)
    while side ** 3 < n:
        side += 1
    cell = rng.permutation(side ** 3)[:n]
    ijk = np.stack([cell % side, (cell // side) % side, cell // (side * side)], axis=1).astype(np.float64)
    return ((ijk - (side - 1) / 2.0) * spacing + rng.uniform(-1.0, 1.0, (n, 3))).astype(np.float32)


def near(x, d):
    return (np.asarray(x, np.float64) + np.asarray(d, np.float64)).astype(np.float32)


def fillers(x, n):
    """n distinct frame keypoints 1000 m and more from every x_i"""
    far = np.float64(np.abs(x).max() if len(x) else 0.0) + 1000.0
    i = np.arange(n)
    return np.stack([far + 2.0 * (i % W), far + 2.0 * (i // W), np.zeros(n)], axis=1).astype(np.float32)


def ulp_pair(m):
    """radii one ulp apart with r0 * r0 < m <= r1 * r1"""
    r0 = np.sqrt(np.float64(m))
    while r0 * r0 >= m:
        r0 = np.nextafter(r0, 0.0)
    while np.nextafter(r0, np.inf) ** 2 < m:
        r0 = np.nextafter(r0, np.inf)
    r1 = np.nextafter(r0, np.inf)
    assert r0 * r0 < m <= r1 * r1
    return r0, r1


def exact_radius(R, t, q_xyz, q_lab, f_xyz, f_lab, i, j):
    """move frame keypoint j over the f32 grid (a coordinate in turn, upwards) until m = r2(i, j) has sqrt(m) ** 2 == m -> m"""
    for k in range(6000):
        m = ov.r2_matrix(R, t, q_xyz[i:i + 1], q_lab[i:i + 1], f_xyz[j:j + 1], f_lab[j:j + 1])[0][0, 0]
        s = np.sqrt(m)
        if s * s == m:
            return m
        f_xyz[j, k % 3] = np.nextafter(f_xyz[j, k % 3], np.float32(np.inf))
    raise AssertionError("no f32 position with an exactly representable distance within 2000 ulps a coordinate")


def _counts(e, which="before"):
    return e[which]["n_hit_query"], e[which]["n_hit_frame"]


# ---- threshold -------------------------------------------------------------------------------------------------------
def threshold(kind):
    """one planted pair (i, j) at about 0.7 m; three radii: r0 * r0 < m <= r1 * r1 one ulp apart, and radius * radius == m"""
    def build(R, t, seed):
        rng = np.random.default_rng(seed)
        q = lattice(rng, 8)
        ql = np.ones(8, np.uint32)
        if kind == "shared":                                  # two query keypoints 1 m apart share one frame keypoint
            q[1] = near(q[0], [1.0, 0.0, 0.0])
        x = ov.transform(R, t, q)
        f = fillers(x, 5)
        if kind == "query":                                   # (a) the query's only hit
            f[0], (i, j) = near(x[0], [0.7, 0, 0]), (0, 0)
        elif kind == "frame":                                 # (b) keypoint 0's nearest is frame keypoint 0; keypoint 1 at the threshold
            f[0], f[1], (i, j) = near(x[0], [0.2, 0, 0]), near(x[0], [0, 0.7, 0]), (0, 1)
        elif kind == "shared":                                # (c) 0.3 m from x_0 towards x_1: 0.7 m from x_1
            f[0], (i, j) = near(x[0], 0.3 * (x[1] - x[0]) / np.linalg.norm(x[1] - x[0])), (1, 0)
        else:                                                 # (d) "asg3": two assigned for sure, the third at the threshold
            f[0], f[1], f[2], (i, j) = near(x[0], [0.3, 0, 0]), near(x[1], [0, 0.3, 0]), near(x[2], [0, 0, 0.7]), (2, 2)
        fl = np.ones(5, np.uint32)
        m = exact_radius(R, t, q, ql, f, fl, i, j)
        r0, r1 = ulp_pair(m)
        radii = sorted({float(r0), float(r1), float(np.sqrt(m))})
        assert float(np.sqrt(m)) ** 2 == m and len(radii) >= 2

        def promise(res):
            seen = set()
            for r in radii:
                e, inside = res[(r, 1)], bool(m <= np.float64(r) * np.float64(r))
                seen.add(inside)
                if kind == "query":
                    assert _counts(e) == (int(inside), int(inside)) and e["assign"][0] == (0 if inside else -1)
                    assert ov.same_value(e["before"]["overlap"], np.float64(int(inside)) / np.float64(8))
                elif kind == "frame":
                    assert _counts(e) == (1, 1 + int(inside)) and e["assign"][0] == 0
                elif kind == "shared":
                    assert _counts(e) == (1 + int(inside), 1) and e["assign"][1] == (0 if inside else -1) and e["assign"][0] == 0
                else:
                    assert e["before"]["n_hit_query"] == 2 + int(inside)
                    assert (e["n_fits"], e["n_corr"], e["stop"]) == ((1, 3, 0) if inside else (0, 0, 1))
                if kind != "asg3":
                    assert (e["n_fits"], e["stop"]) == (0, 1)
            assert seen == {False, True}
        return Workload("threshold/" + kind, q, ql, f, fl, [(r, 1) for r in radii], promise, m=m, radii=radii, exact=float(np.sqrt(m)))
    return build


def zero_radius(R, t, seed):
    """radius 0: f32(x_0) is x_0 only by chance, f32(t) is the image of a keypoint at the origin only if t is
    representable; a hit needs r2 == 0 exactly"""
    rng = np.random.default_rng(seed)
    q = lattice(rng, 8)
    q[1] = 0.0
    ql = np.ones(8, np.uint32)
    x = ov.transform(R, t, q)
    f = fillers(x, 4)
    f[0], f[1] = near(x[0], 0.0), near(x[1], 0.0)
    fl = np.ones(4, np.uint32)
    m = ov.minima(R, t, q, ql, f, fl)
    zeros = int(np.count_nonzero(m == 0.0))

    def promise(res):
        e = res[(0.0, 1)]
        assert (m[2:] > 25.0).all() and (m[:2] < 1e-6).all()
        assert _counts(e) == (zeros, zeros) and (e["n_fits"], e["stop"]) == (0, 1)
        assert np.array_equal(e["assign"] >= 0, m == 0.0)
    return Workload("threshold/zero", q, ql, f, fl, [(0.0, 1)], promise, zeros=zeros)


# ---- ties, NaN, inf --------------------------------------------------------------------------------------------------
def _free(nf, taken, n):
    """n frame indices from the middle of the frame on, none of them taken"""
    out, k = [], nf // 2
    while len(out) < n:
        if k % nf not in taken and k % nf not in out:
            out.append(k % nf)
        k += 1
    return out


def ties(nf, i, j, tag=None):
    """twin frame keypoints (the same bits, the same label) at i < j, three more pairs for a fit: the lowest index is assigned"""
    def build(R, t, seed):
        rng = np.random.default_rng(seed)
        q = lattice(rng, 8)
        x = ov.transform(R, t, q)
        f = fillers(x, nf)
        f[i] = f[j] = near(x[0], D)
        others = _free(nf, (i, j), 3)
        for k, o in enumerate(others):
            f[o] = near(x[k + 1], D)

        def promise(res):
            e = res[(1.0, 3)]
            assert e["assign"][:4].tolist() == [i] + others and (e["assign"][4:] == -1).all()
            assert _counts(e) == (4, 5) and _counts(e, "after") == (4, 5)            # both twins are reached
            assert (e["n_fits"], e["n_corr"], e["stop"]) == (1, 4, 2)
        return Workload(tag or "ties/%d_%d" % (i, j), q, np.ones(8, np.uint32), f, np.ones(nf, np.uint32), [(1.0, 3)], promise, lowest=i)
    return build


def decoy(kind):
    """what stands at index 0 ahead of the real nearest keypoint (index 3): a twin of another label, a same-label keypoint
    with a NaN or a +inf coordinate; "dead": query keypoint 4's label has only NaN and inf keypoints in the frame"""
    def build(R, t, seed):
        rng = np.random.default_rng(seed)
        q = lattice(rng, 8)
        ql = np.ones(8, np.uint32)
        x = ov.transform(R, t, q)
        f = fillers(x, 9)
        fl = np.ones(9, np.uint32)
        f[3] = near(x[0], D)
        f[0] = f[3]
        n_asg = 4
        if kind == "label":
            fl[0] = 2
        elif kind == "nan":
            f[0, 0] = np.nan
        elif kind == "inf":
            f[0, 0] = np.inf
        else:
            ql[4] = 7
            f[0], f[1], f[2] = [np.inf, 0, 0], [np.nan, 0, 0], [1.0, -np.inf, 2.0]
            fl[:3] = 7
        others = [6, 7, 8]
        for k, o in enumerate(others):
            f[o] = near(x[k + 1], D)

        def promise(res):
            e = res[(1.0, 3)]
            assert e["assign"][:4].tolist() == [3] + others and (e["assign"][4:] == -1).all()
            assert _counts(e) == (n_asg, 4) and (e["n_fits"], e["n_corr"], e["stop"]) == (1, 4, 2)
        return Workload("ties/decoy_" + kind, q, ql, f, fl, [(1.0, 3)], promise)
    return build


# ---- sizes -----------------------------------------------------------------------------------------------------------
FRAME_SIZES = [1, 2, 3, 4, 5, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 3, MAX_KP]
QUERY_SIZES = [0, 1, 2, 3, 4, 255, 256, 257, CAP - 1, CAP, CAP + 1, 4097, MAX_KP]


def frame_size(nf, where):
    """a frame of nf keypoints whose deciding keypoint (query keypoint 0's) is the last one, or the first of the last tile;
    up to three more pairs elsewhere; everything else 1000 m away"""
    d = nf - 1 if where == "last" else ((nf - 1) // TILE) * TILE

    def build(R, t, seed):
        rng = np.random.default_rng(seed)
        q = lattice(rng, 8)
        x = ov.transform(R, t, q)
        f = fillers(x, nf)
        f[d] = near(x[0], D)
        extra = [k for k in [0, nf // 2, 1, 2, 3] if k != d and k < nf]
        extra = list(dict.fromkeys(extra))[:3]
        for k, o in enumerate(extra):
            f[o] = near(x[k + 1], D)
        n = 1 + len(extra)

        def promise(res):
            e = res[(1.0, 3)]
            assert e["assign"][:n].tolist() == [d] + extra and (e["assign"][n:] == -1).all()
            assert e["before"]["n_frame_kp"] == nf and _counts(e) == (n, n) and _counts(e, "after") == (n, n)
            assert (e["n_fits"], e["n_corr"], e["stop"]) == ((1, n, 2) if n >= 3 else (0, 0, 1))
        return Workload("sizes/frame%d/%s" % (nf, where), q, np.ones(8, np.uint32), f, np.ones(nf, np.uint32), [(1.0, 3)], promise,
                        large=nf == MAX_KP, deciding=d)
    return build


def query_size(nq):
    """a query of nq keypoints whose last one decides, against a frame of 5 (frame keypoint 4 is its partner)"""
    def build(R, t, seed):
        rng = np.random.default_rng(seed)
        q = lattice(rng, nq)
        x = ov.transform(R, t, q)
        f = fillers(x, 5)
        pairs = {}
        if nq:
            pairs[nq - 1] = 4
        if nq >= 4:
            pairs.update({0: 0, 1: 1, 2: 2})
        for i, j in pairs.items():
            f[j] = near(x[i], D)
        want = np.full(nq, -1, np.int32)
        for i, j in pairs.items():
            want[i] = j
        n = len(pairs)

        def promise(res):
            e = res[(1.0, 3)]
            assert e["assign"].shape == (nq,) and np.array_equal(e["assign"], want)
            assert e["before"]["n_query_kp"] == nq and _counts(e) == (n, n) and _counts(e, "after") == (n, n)
            assert (e["n_fits"], e["n_corr"], e["stop"]) == ((1, n, 2) if n >= 3 else (0, 0, 1))
            assert np.isnan(e["before"]["overlap"]) if nq == 0 else ov.same_value(e["before"]["overlap"], np.float64(n) / np.float64(nq))
        return Workload("sizes/query%d" % nq, q, np.ones(nq, np.uint32), f, np.ones(5, np.uint32), [(1.0, 3)], promise, large=nq == MAX_KP)
    return build


# ---- origin ----------------------------------------------------------------------------------------------------------
ORIGIN_SIZES = [0, 1, 255, 257, CAP + 1]


def origin(nq, with0):
    """a label-0 frame keypoint at (0, 0, 0): where the inactive lanes of the last round stand (x = 0, label 0).  with0: the
    query has label-0 keypoints, all of them 20 m and more from the origin under the start pose"""
    def build(R, t, seed):
        rng = np.random.default_rng(seed)
        q = lattice(rng, nq)
        x = ov.transform(R, t, q)
        ql = np.ones(nq, np.uint32)
        if with0:
            ql[(np.linalg.norm(x, axis=1) >= 20.0) & (np.arange(nq) % 3 == 0)] = 0
        f = fillers(x, 6)
        fl = np.array([1, 1, 0, 1, 0, 1], np.uint32)
        f[2] = 0.0
        pairs = dict(zip(range(min(3, nq)), (0, 1, 3)))
        for i, j in pairs.items():
            f[j], fl[j] = near(x[i], D), ql[i]
        n = len(pairs)
        want = np.full(nq, -1, np.int32)
        want[:n] = [pairs[i] for i in range(n)]

        def promise(res):
            e = res[(1.0, 3)]
            assert not f[2].any() and fl[2] == 0
            if with0 and nq >= 255:
                assert np.count_nonzero(ql == 0) >= 10
            assert _counts(e) == (n, n) and _counts(e, "after") == (n, n)          # the origin keypoint is not counted
            assert np.array_equal(e["assign"], want)
        return Workload("origin/%d/%s" % (nq, "label0_far" if with0 else "no_label0"), q, ql, f, fl, [(1.0, 3)], promise)
    return build


# ---- labels ----------------------------------------------------------------------------------------------------------
def labels(R, t, seed):
    """nine coincident frame keypoints per query keypoint, one of every label, in an order that turns with the keypoint:
    only the equality of the 32-bit labels separates a hit from a miss"""
    rng = np.random.default_rng(seed)
    n, nl = 2 * len(LABELS), len(LABELS)
    q = lattice(rng, n)
    ql = LABELS[np.arange(n) % nl]
    x = ov.transform(R, t, q)
    f = np.repeat(near(x, D), nl, axis=0)
    fl = np.concatenate([np.roll(LABELS, i) for i in range(n)])
    want = np.array([nl * i + int(np.flatnonzero(np.roll(LABELS, i) == ql[i])[0]) for i in range(n)], np.int32)
    twice = int(np.count_nonzero(ql == 1))      # (1 and 0x00000001 are one label: two of the nine reach it, the lower is assigned)

    def promise(res):
        e = res[(1.0, 3)]
        assert np.array_equal(e["assign"], want)
        assert _counts(e) == (n, n + twice) and (e["n_fits"], e["n_corr"], e["stop"]) == (1, n, 2)
    return Workload("labels/coincident", q, ql, f, fl, [(1.0, 3)], promise)


# ---- order -----------------------------------------------------------------------------------------------------------
def order_take(kind, n=4 * W):
    i = np.arange(n)
    if kind == "alternate":
        return i % 2 == 0                      # every second accumulator stays empty
    if kind == "only255":
        return i % W == W - 1                  # accumulator 255 alone
    return (i < W) | (i >= 2 * W)              # "midround": the whole second round misses


def order(kind):
    """1024 query keypoints, each with a partner at 1e-7 m to 1.5 m (the minima spread over many decades, half of them
    between 0.09 and 2.25 m^2), the non-hits' partners 5 m away; radius 2"""
    def build(R, t, seed):
        n = 4 * W
        take = order_take(kind, n)
        for sub in range(64):                          # the first sub-seed whose sum shows the order: the three other orders give other bits
            rng = np.random.default_rng([seed, sub])
            q = lattice(rng, n)
            x = ov.transform(R, t, q)
            u = rng.normal(size=(n, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            dist = np.where(rng.random(n) < 0.5, 10.0 ** rng.uniform(-7.0, 0.17, n), rng.uniform(0.3, 1.5, n))    # (half of them of one magnitude)
            f = near(x, u * np.where(take, dist, 5.0)[:, None])
            e = x - f.astype(np.float64)
            own = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]          # r2(i, i)
            s = ov.ordered_sum(own, take)
            if kind == "only255" or all(v.view(np.uint64) != s.view(np.uint64) for v in other_sums(own, take).values()):
                break
        else:
            raise AssertionError("no sub-seed of 64 separates the summation orders")
        m = ov.minima(R, t, q, np.ones(n, np.uint32), f, np.ones(n, np.uint32))
        assert np.array_equal(m, own)                  # every keypoint's nearest is its own partner
        hits = m[m <= 4.0]
        decades = float(np.log10(hits.max() / hits[hits > 0].min()))

        def promise(res):
            e = res[(2.0, 1)]
            assert np.array_equal(m <= 4.0, take) and (decades >= 9.0 or kind == "only255"), decades     # (only255 has four hits)
            assert _counts(e) == (int(take.sum()),) * 2 and (e["n_fits"], e["stop"]) == (1, 0)
        return Workload("order/" + kind, q, np.ones(n, np.uint32), f, np.ones(n, np.uint32), [(2.0, 1)], promise, m=m, take=take, decades=decades)
    return build


def other_sums(values, take):
    """the same terms in three other orders -> {name: sum}"""
    v = np.asarray(values, np.float64)[np.asarray(take, bool)]
    out = {}
    s = np.float64(0.0)
    for a in v:
        s = s + a
    out["sequential"] = s
    idx = np.flatnonzero(take)
    n = len(take)
    per = -(-n // W)
    acc = np.zeros(W)
    for i in idx:                                   # accumulator l <- the contiguous block l
        acc[i // per] = acc[i // per] + np.float64(values[i])
    k = W // 2
    while k >= 1:
        acc[:k] = acc[:k] + acc[k:2 * k]
        k //= 2
    out["blocks"] = np.float64(acc[0])
    w = list(v)
    while len(w) > 1:                               # adjacent pairs
        w = [w[i] + w[i + 1] if i + 1 < len(w) else w[i] for i in range(0, len(w), 2)]
    out["pairs"] = np.float64(w[0])
    return out


# ---- stop ------------------------------------------------------------------------------------------------------------
def stop_rigid(R, t, seed):
    """(a) every keypoint's partner at the same offset D: one fit, then the same assignment"""
    rng = np.random.default_rng(seed)
    n = 40
    q = lattice(rng, n)
    x = ov.transform(R, t, q)
    f = near(x, D)

    def promise(res):
        e3, e1 = res[(1.0, 3)], res[(1.0, 1)]
        assert (e3["n_fits"], e3["n_corr"], e3["stop"]) == (1, n, 2) and (e1["n_fits"], e1["n_corr"], e1["stop"]) == (1, n, 0)
        assert np.array_equal(e3["assign"], np.arange(n)) and np.array_equal(e1["assign"], np.arange(n))
        assert e3["after"]["rms"] < 1e-4 < e3["before"]["rms"]
    return Workload("stop/rigid", q, np.ones(n, np.uint32), f, np.ones(n, np.uint32), [(1.0, 3), (1.0, 1)], promise)


def stop_flip(nqk):
    """(b, c) 30 partners shifted by 0.4 m in x; the last query keypoint stands between frame keypoints 30 (0.15 m behind
    it) and 31 (0.55 m ahead): nearer to 30 by 0.28 m^2 under the start pose, nearer to 31 by 0.2 m^2 after the first fit.
    A_2 differs from A_1 in that one element, of the same count; a third walk finds A_3 = A_2"""
    def build(R, t, seed):
        rng = np.random.default_rng(seed)
        q = lattice(rng, nqk)
        x = ov.transform(R, t, q)
        L = nqk - 1
        f = np.concatenate([near(x[:30], [0.4, 0, 0]), near(x[L], [-0.15, 0, 0])[None], near(x[L], [0.55, 0, 0])[None]])
        a1, m1, _ = al.assignment(R, t, q, np.ones(nqk, np.uint32), f, np.ones(32, np.uint32), 1.0)
        want = np.full(nqk, -1, np.int32)
        want[:30] = np.arange(30)
        want[L] = 31

        def promise(res):
            assert a1[L] == 30 and np.count_nonzero(a1 >= 0) == 31 and np.array_equal(np.delete(a1, L), np.delete(want, L))
            for it, fits, stop in ((5, 2, 2), (2, 2, 0), (1, 1, 0)):        # (c): out of iterations exactly where it would converge
                e = res[(1.0, it)]
                assert (e["n_fits"], e["n_corr"], e["stop"]) == (fits, 31, stop), (it, e["n_fits"], e["stop"])
                assert np.array_equal(e["assign"], want) and _counts(e, "after") == (31, 32)
        return Workload("stop/flip%d" % nqk, q, np.ones(nqk, np.uint32), f, np.ones(32, np.uint32), [(1.0, 5), (1.0, 2), (1.0, 1)], promise,
                        owner=(L % W, L // W))
    return build


def stop_leave3(R, t, seed):
    """(d) exactly three assigned under the start pose: an isosceles triangle whose partners stretch its height (the apex
    0.95 m outwards, the base 0.6 m the other way; by symmetry the fit is a translation of -0.083 m along the height).
    The fit leaves the apex 1.033 m from its partner, out of reach: stop 1 after one fit, and the fitted pose stands"""
    rng = np.random.default_rng(seed)
    q = np.concatenate([np.array([[0, 20, 0], [-10, 0, 0], [10, 0, 0]], np.float32), lattice(rng, 5) + np.float32([0, 0, 200])])
    x = ov.transform(R, t, q)
    up = np.asarray(R, np.float64).reshape(3, 3) @ np.array([0.0, 1.0, 0.0])
    f = fillers(x, 4)
    f[0], f[1], f[2] = near(x[0], 0.95 * up), near(x[1], -0.6 * up), near(x[2], -0.6 * up)

    def promise(res):
        e = res[(1.0, 5)]
        assert _counts(e) == (3, 3) and (e["n_fits"], e["n_corr"], e["stop"]) == (1, 3, 1)
        assert _counts(e, "after")[0] == 2 and e["assign"][0] == -1 and e["assign"][1:3].tolist() == [1, 2]
    return Workload("stop/leave3", q, np.ones(8, np.uint32), f, np.ones(4, np.uint32), [(1.0, 5)], promise)


# ---- the suite -------------------------------------------------------------------------------------------------------
def builders():
    """[(name, builder)]: one candidate each"""
    out = [("threshold/" + k, threshold(k)) for k in ("query", "frame", "shared", "asg3")] + [("threshold/zero", zero_radius)]
    out += [("ties/%d_%d" % (i, j), ties(nf, i, j)) for nf, i, j in ((9, 0, 1), (9, 2, 3), (9, 3, 4), (TILE - 1, TILE - 4, TILE - 2),
                                                                      (TILE + 6, TILE - 1, TILE), (2 * TILE + 52, TILE + 5, 2 * TILE + 5),
                                                                      (3 * TILE + 3, 0, 3 * TILE + 2))]
    out += [("ties/decoy_" + k, decoy(k)) for k in ("label", "nan", "inf", "dead")]
    for nf in FRAME_SIZES:
        out.append(("sizes/frame%d/last" % nf, frame_size(nf, "last")))
        if nf > 1:
            out.append(("sizes/frame%d/tile0" % nf, frame_size(nf, "tile0")))
    out += [("sizes/query%d" % n, query_size(n)) for n in QUERY_SIZES]
    out += [("origin/%d/%s" % (n, "label0_far" if w else "no_label0"), origin(n, w)) for n in ORIGIN_SIZES for w in (False, True)]
    out += [("labels/coincident", labels)]
    out += [("order/" + k, order(k)) for k in ("alternate", "only255", "midround")]
    out += [("stop/rigid", stop_rigid), ("stop/flip1025", stop_flip(CAP + 1)), ("stop/flip1000", stop_flip(1000)), ("stop/leave3", stop_leave3)]
    return out


def own_keypoints(R, t, seed, q_xyz, q_lab):
    """around a batch's own query keypoints (no explicit ones): every keypoint's partner at a tenth of D, a twin of
    keypoint 0's partner at the end, a label-0 keypoint at the origin and a keypoint of a foreign label on top of keypoint
    1's partner at index 0"""
    n = len(q_lab)
    x = ov.transform(R, t, q_xyz)
    base = near(x, 0.1 * D)
    f = np.concatenate([base[1:2], base, base[0:1], np.zeros((1, 3), np.float32)])
    fl = np.concatenate([[0x00010000 | int(q_lab[1])], q_lab, q_lab[0:1], [0]]).astype(np.uint32)
    hit_origin = bool(((np.asarray(q_lab) == 0) & ((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2] <= 0.25)).any())

    def promise(res):
        e = res[(0.5, 3)]
        assert np.array_equal(e["assign"], 1 + np.arange(n)) and (e["n_fits"], e["n_corr"], e["stop"]) == (1, n, 2)
        assert _counts(e) == (n, n + 1 + int(hit_origin))
    return Workload("own/rigid", q_xyz, q_lab, f, fl, [(0.5, 3)], promise)


# ---- the restatement on a workload -----------------------------------------------------------------------------------
def margin(R, t, wl, radius):
    """the smallest distance (m^2) of a decision from its threshold under (R, t): an m_i from radius^2, a best from a
    second-best r2 of an assigned keypoint (copies of the best keypoint aside)"""
    rr = np.float64(radius) * np.float64(radius)
    r2, same = ov.r2_matrix(R, t, wl.q_xyz, wl.q_lab, wl.f_xyz, wl.f_lab)
    if r2.shape[0] == 0 or r2.shape[1] == 0:
        return np.inf
    with np.errstate(invalid="ignore"):
        masked = np.where(same & ~np.isnan(r2), r2, np.inf)
        j = np.argmin(masked, axis=1)
        m = masked[np.arange(len(j)), j]
        fin = np.isfinite(m)
        out = np.abs(m[fin] - rr).min() if fin.any() else np.inf
        w = wl.f_xyz.view(np.uint32)
        twin = (w[None, :, :] == w[j][:, None, :]).all(axis=2)
        gap = np.where(twin, np.inf, masked).min(axis=1) - m
        gap = gap[fin & np.isfinite(gap) & (m <= rr)]          # (out of reach, the nearest keypoint's index decides nothing)
    return float(min(out, gap.min() if gap.size else np.inf))


def reference(wl, R, t, radius, iterations):
    """_align_ref.align from (R, t), plus `late_margin`: the smallest margin of the walks after the first fit (inf: none)"""
    e = al.align(R, t, wl.q_xyz, wl.q_lab, wl.f_xyz, wl.f_lab, radius, iterations)
    Rk, tk = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    late, prev = np.inf, None
    for it in range(1, iterations + 1):
        a, _, _ = al.assignment(Rk, tk, wl.q_xyz, wl.q_lab, wl.f_xyz, wl.f_lab, radius)
        if np.count_nonzero(a >= 0) < 3 or (it >= 2 and np.array_equal(a, prev)):
            break
        cp, cw, H = al.fit(wl.q_xyz, wl.f_xyz, a)
        Rk = rf.kabsch(H)
        tk = rf.translation(Rk, cp, cw)
        prev = a
        late = min(late, margin(Rk, tk, wl, radius))
    assert np.array_equal(Rk, e["rot"]) and np.array_equal(tk, e["t"])
    e["late_margin"] = late
    return e


def signature(e):
    """everything of a result that does not come out of an SVD, as comparable values"""
    f = lambda d: tuple(int(d[k]) for k in ov.KEYS[:4]) + tuple(np.float64(d[k]).view(np.uint64) if not np.isnan(d[k]) else -1 for k in ov.KEYS[4:])
    return f(e["before"]), f(e["after"]), int(e["n_fits"]), int(e["n_corr"]), int(e["stop"]), tuple(np.asarray(e["assign"]).tolist())


# ---- mutants of the rule ---------------------------------------------------------------------------------------------
MUTANTS = {
    "lt": ["threshold/query", "threshold/shared"],                     # m < rr
    "high_tie": ["ties/0_1", "ties/2_3", "ties/3_4", "ties/1023_1024"],  # the highest j wins a tie
    "tile_reset": ["ties/1029_2053", "ties/0_3074", "sizes/frame2049/tile0"],   # the best index is reset per tile
    "nearest_only": ["threshold/frame"],                               # the frame hit comes from the nearest keypoint only
    "low16": ["labels/coincident"],                                    # labels are compared in their low 16 bits
    "no_gate": ["ties/decoy_label", "labels/coincident"],              # the label gate is missing on the frame hit
    "stop_le3": ["threshold/asg3", "stop/leave3", "sizes/frame3/last"],  # stop at <= 3 assigned
    "conv_by_count": ["stop/flip1000", "stop/flip1025"],               # convergence judged on the assigned count
    "seq_sum": ["order/alternate", "order/midround"],                  # the sum runs sequentially
    "skip_tail": ["sizes/frame1/last", "sizes/frame5/last", "ties/1020_1022", "sizes/frame2049/last"],   # a tile's nt % 4 tail is skipped
    "inactive": ["origin/1/no_label0", "origin/255/no_label0", "origin/257/label0_far", "origin/1025/no_label0"],   # inactive lanes are included
    "conv_when_out": ["stop/rigid", "stop/flip1000"],                  # convergence is reported when the iterations run out
}


def _mwalk(mut, R, t, wl, radius):
    """one walk of the rule, tile by tile as the kernel goes, with one mutation -> (a, figures)"""
    rr = np.float64(radius) * np.float64(radius)
    n = len(wl.q_lab)
    pad = (W - n % W) % W if mut == "inactive" else 0
    r2, same = ov.r2_matrix(R, t, wl.q_xyz, wl.q_lab, wl.f_xyz, wl.f_lab)
    if pad:                                            # lanes past the query's end: x = (0, 0, 0), label 0
        w = wl.f_xyz.astype(np.float64)
        r0 = ((0.0 - w[:, 0]) ** 2 + (0.0 - w[:, 1]) ** 2) + (0.0 - w[:, 2]) ** 2
        r2 = np.concatenate([r2, np.repeat(r0[None], pad, axis=0)])
        same = np.concatenate([same, np.repeat((wl.f_lab == 0)[None], pad, axis=0)])
    if mut == "low16":
        same = (wl.q_lab[:, None] & 0xFFFF) == (wl.f_lab[None, :] & 0xFFFF)
    nn, nf = r2.shape
    m, bj, hit_f = np.full(nn, np.inf), np.full(nn, -1, np.int64), np.zeros(nf, bool)
    with np.errstate(invalid="ignore"):
        for t0 in range(0, nf, TILE):
            nt = min(TILE, nf - t0)
            use = nt - nt % 4 if mut == "skip_tail" else nt
            if mut == "tile_reset":
                bj[:] = -1
            if use == 0 or nn == 0:
                continue
            b2, bs = r2[:, t0:t0 + use], same[:, t0:t0 + use]
            cand = bs & ~np.isnan(b2)
            masked = np.where(cand, b2, np.inf)
            has = cand.any(axis=1)
            tmin = masked.min(axis=1)
            eq = cand & (masked == tmin[:, None])
            if mut == "high_tie":
                upd, pick = has & (tmin <= m), use - 1 - np.argmax(eq[:, ::-1], axis=1)
            else:
                upd, pick = has & ((tmin < m) | ((bj < 0) & (tmin <= m))), np.argmax(eq, axis=1)
            m, bj = np.where(upd, tmin, m), np.where(upd, t0 + pick, bj)
            gate = np.ones_like(bs) if mut == "no_gate" else bs
            hit_f[t0:t0 + use] |= (gate & (b2 <= rr)).any(axis=0)
        m, bj = m[:n], bj[:n]
        hit_q = (m < rr) if mut == "lt" else (m <= rr)
    a = np.where(hit_q & (bj >= 0), bj, -1).astype(np.int32)
    if mut == "nearest_only":
        hit_f[:] = False
        hit_f[a[a >= 0]] = True
    nhq, nhf = int(hit_q.sum()), int(hit_f.sum())
    s = other_sums(m, hit_q)["sequential"] if mut == "seq_sum" and nhq else ov.ordered_sum(m, hit_q)
    nan = np.float64("nan")
    fig = dict(n_query_kp=n, n_frame_kp=nf, n_hit_query=nhq, n_hit_frame=nhf, overlap=np.float64(nhq) / np.float64(n) if n else nan,
               rms=np.sqrt(s / np.float64(nhq)) if nhq else nan)
    return a, fig


def mutant_align(mut, wl, R0, t0, radius, iterations):
    """the rule with one mutation (None: the rule itself), in _align_ref.align's result shape"""
    R, t = np.asarray(R0, np.float64).reshape(3, 3), np.asarray(t0, np.float64).reshape(3)
    a, before = _mwalk(mut, R, t, wl, radius)
    after, prev, stop, n_fits, n_corr = before, None, 0, 0, 0
    for it in range(1, iterations + 1):
        na = int(np.count_nonzero(a >= 0))
        if na < (4 if mut == "stop_le3" else 3):
            stop = 1
            break
        if it >= 2 and (na == int(np.count_nonzero(prev >= 0)) if mut == "conv_by_count" else np.array_equal(a, prev)):
            stop = 2
            break
        cp, cw, H = al.fit(wl.q_xyz, wl.f_xyz, a)
        R = rf.kabsch(H)
        t = rf.translation(R, cp, cw)
        n_fits, n_corr, prev = n_fits + 1, na, a
        a, after = _mwalk(mut, R, t, wl, radius)
    if mut == "conv_when_out" and stop == 0 and prev is not None and np.array_equal(a, prev):
        stop = 2
    return dict(before=before, after=after, assign=a, n_fits=n_fits, n_corr=n_corr, stop=stop)


# ---- placing the workloads on a verified batch -----------------------------------------------------------------------
def place(n, verified, per_query=1):
    """workload i goes to query i // per_query, on its first verified candidate whose frame no earlier workload has taken;
    verified(q) -> [(candidate, frame)] -> [(q, candidate, frame)].  The device's query keypoints are a query's, so the GPU
    half places one workload per query; the CPU half needs the poses only and places several"""
    used, out, cands = set(), [], {}
    for i in range(n):
        q = i // per_query
        if q not in cands:
            cands[q] = list(verified(q))
        k, f = next((k, f) for k, f in cands[q] if f not in used)
        used.add(f)
        out.append((q, k, f))
    return out
