"""Frames at the edges of build_frames_kernel's neighbour selection, and a numpy restatement of that selection.  Plain
helper module of tests/test_knn_edges.py (CPU: the restatement and the oracle agree on every frame, the frames hold the
ties they are named after) and tests/test_gpu_knn_edges.py (GPU: the library equals the oracle on them, bit for bit).
No GPU and no torch here.

The kernel selects a keypoint's K nearest (itself included) in batches of K candidates per thread, by sorting networks
on keys (f32 distance bits, index), four threads per keypoint where 3 K <= C(K-1, 2): thread `part` takes the candidates
n * part / 4 .. n * (part + 1) / 4.  Sizes: n = K, K + 1, 2K - 1, 2K, 2K + 1, 4K + 3, 41 and 200 — batch tails of every
length class and quarter boundaries that do not divide — plus a frame of K - 1 keypoints (no descriptors).  Kinds:
  random      no tie at all (the baseline of every size)
  lattice     points of an integer lattice with spacing 1, in a random order: most distances tie
  collinear   equally spaced points on a line, in a random order: every distance ties left against right
  duplicates  a point copied to the lowest, the highest and some middle indices; a second pair
  kth_tie     one keypoint with K - 1 nearer points at different distances and two at the same distance after them:
              the lower index alone belongs to its list
A batch is one launch.  One whose largest frame is past lds_switch(K) runs every frame of it in the kernel's global
dedup form, so each K has a batch of the frames up to that size (LDS form) and a batch of all frames with a frame
past it (global form): both hold frames far smaller than the batch's largest.
"""
import numpy as np

import _build_edges as be

F32 = np.float32
KS = (4, 8, 10, 12, 16)            # descriptor_near_num, one per network size of the kernel
KINDS = ("random", "lattice", "collinear", "duplicates", "kth_tie")
LARGE = 200                        # at this size: random, lattice and duplicates only (the restatement's time)


def cfg_of(K):
    return be.cfg_of(K, 0.5, 50.0)


def sizes(K):
    out = []
    for n in (K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, 4 * K + 3, 41, LARGE):
        if n not in out:
            out.append(n)
    return out


def knn_ref(xyz, K):
    """the K nearest of every point, itself included: f32 ((dx*dx) + dy*dy) + dz*dz, every operation rounded to f32, a
    stable argsort (equal distances: the lower index first).  -> (idx [n, K], the K + 1 smallest distances [n, K + 1],
    inf where there are fewer)"""
    x = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    n = len(x)
    with np.errstate(over="ignore", invalid="ignore"):
        d = x[:, None, :] - x[None, :, :]
        d2 = d[..., 0] * d[..., 0]
        d2 = d2 + d[..., 1] * d[..., 1]
        d2 = d2 + d[..., 2] * d[..., 2]
    assert d2.dtype == F32
    order = np.argsort(d2, axis=1, kind="stable")
    near = np.full((n, K + 1), np.inf, F32)
    kk = min(K + 1, n)
    near[:, :kk] = np.take_along_axis(d2, order[:, :kk], axis=1)
    return order[:, :K], near


def tie_stats(xyz, K):
    """(keypoints with a tie among their K + 1 nearest, keypoints whose K-th and (K + 1)-th distances tie)"""
    _, near = knn_ref(xyz, K)
    inside = np.any(near[:, 1:] == near[:, :-1], axis=1)
    return int(np.sum(inside)), int(np.sum(near[:, K - 1] == near[:, K]))


def _lattice(n, seed):
    s = 1
    while s ** 3 < n:
        s += 1
    g = np.stack(np.meshgrid(*[np.arange(s)] * 3, indexing="ij"), -1).reshape(-1, 3)
    return g[np.random.default_rng(seed).permutation(len(g))[:n]].astype(F32)


def _collinear(n, seed):
    t = np.random.default_rng(seed).permutation(n).astype(F32)
    return np.stack([t, 2 * t, 2 * t], 1) * F32(0.5)          # spacing 1.5, every coordinate exact


def _duplicates(n, seed, K):
    pts = be.random_frame(n, seed, K)[0].copy()
    src = n // 2
    at = sorted({0, n - 1, src} | ({n // 4, (3 * n) // 4} if n >= 12 else set()))
    pts[at] = pts[src]
    if n >= 8:
        pts[n // 3] = pts[n // 3 + 1]
    return pts


def _kth_tie(n, seed, K):
    """n >= K + 1.  Around the origin: K - 2 points on the x axis at 1, 2, ..., K - 2, then (0, R, 0) and (0, 0, R); the
    rest far off in -x.  In a random order."""
    rng = np.random.default_rng(seed)
    R = F32(K - 1.5)
    core = [[0, 0, 0]] + [[k, 0, 0] for k in range(1, K - 1)] + [[0, R, 0], [0, 0, R]]
    rest = np.zeros((n - len(core), 3))
    rest[:, 0] = -40.0 - 6.0 * rng.random(len(rest))
    rest[:, 1:] = 6.0 * rng.random((len(rest), 2))
    pts = np.concatenate([np.asarray(core, np.float64), rest]).astype(F32)
    return pts[rng.permutation(n)]


def frame(K, n, kind, seed):
    if kind == "random":
        return be.random_frame(n, seed, K)
    pts = {"lattice": lambda: _lattice(n, seed), "collinear": lambda: _collinear(n, seed),
           "duplicates": lambda: _duplicates(n, seed, K), "kth_tie": lambda: _kth_tie(n, seed, K)}[kind]()
    return be._frame(pts)


def cases(K):
    """[(n, kind, (xyz, label))]: every size in every kind that exists at it, then the frame below K"""
    out = []
    for n in sizes(K):
        for k, kind in enumerate(KINDS):
            if (kind == "kth_tie" and n < K + 1) or (n == LARGE and kind in ("collinear", "kth_tie")):
                continue
            out.append((n, kind, frame(K, n, kind, 7000 * K + 10 * n + k)))
    out.append((K - 1, "random", be.random_frame(K - 1, 99 + K, K)))
    return out


def batches(K):
    """{"lds": cases, "global": cases}: one launch each; "global" ends with a frame past the LDS form's largest"""
    all_cases = cases(K)
    switch = be.lds_switch(K)
    lds = [c for c in all_cases if c[0] <= switch]
    glob = list(all_cases)
    if max(c[0] for c in glob) <= switch:
        glob.append((switch + 1, "random", be.random_frame(switch + 1, 31 * K, K)))
    assert max(c[0] for c in lds) <= switch < max(c[0] for c in glob)
    return {"lds": lds, "global": glob}


_CACHE = {}


def all_batches():
    """{(K, form): cases}, generated once"""
    if not _CACHE:
        for K in KS:
            for form, cs in batches(K).items():
                _CACHE[(K, form)] = cs
    return _CACHE
