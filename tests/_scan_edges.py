"""Planted worlds for sgtd_scan_keypoints' structural edges, mutants of the restatement (tests/_scan_ref.py) and a
synchronous model of the device's hook + jump rounds.  tests/test_scan_edges.py shows on the CPU that every world
reaches the edge it is named for and that every mutant changes the world listed with it; tests/test_gpu_scan_edges.py
runs every form of the call on the worlds and compares exactly.

The edges (scan_kernels.hip.h, scan_device in sgtd_accel.hip):
  big-*          scan_sum_block_kernel (clusters of SGTD_SCAN_BIG = 4096 points or more) and the hand-over from
                 scan_sum_wave_kernel at 4095 / 4096 / 4097
  small-sums     the wave kernel at 1, 63, 64, 65 and 255 points
  block27        a voxel with all 26 neighbours occupied (SGTD_SCAN_NBR)
  last-azimuth   the azimuth cell width - 1, whose clamped x + 1 names one neighbour twice, and the wrap of x - 1 at cell 0
  zigzag, percolation   components that need a hook after a jump
  all-dropped, one-live   n_vox == 0, K == 0 and K == 1
  257-scans      a second block of scan_offsets_kernel, K > 256

rounds_model counts hook + jump rounds as a synchronous machine would run them.  The device reads its neighbours' parents
live and may need fewer, so the GPU file asserts results only.  Every round at least halves the number of roots on a path,
and the largest count the model has shown on planted and random scenes is 5: the second group of eight rounds in
scan_device (kGroup) is not reached by any world here."""
import functools

import numpy as np

import _scan_ref as ref

R0, R1, R2 = 19.85, 20.17, 20.5      # ring k, k + 1, k + 2 of a class whose minPolar is 5.0 (bounds 19.6716, 20.004, 20.336, 20.6676)
BIG = 4096                           # SGTD_SCAN_BIG
MAX_SCANS = 4096                     # SGTD_SCAN_MAX_SCANS
UNSUPPORTED = -6                     # SGTD_ERR_UNSUPPORTED


def cell(azi, pit, r, n=1, cls=15, inst=0, jitter=0.0, seed=0):
    """n points in the voxel (azimuth cell azi, pitch cell pit) at range r: at its centre, or within `jitter` metres of it"""
    az, pt = np.deg2rad(azi * 1.2), np.deg2rad(pit * 1.2)
    c = np.array([r * np.cos(pt) * np.cos(az), r * np.cos(pt) * np.sin(az), r * np.sin(pt)])
    p = np.tile(c, (n, 1))
    if jitter:
        p = p + np.random.default_rng(seed).uniform(-jitter, jitter, (n, 3))
    return p.astype(np.float32), np.full(n, cls | (inst << 16), np.uint32)


def scene(*parts):
    return np.concatenate([p for p, _ in parts]), np.concatenate([l for _, l in parts])


def cancelling(part, seed):
    """the part with its z replaced: a third of the points at +a, a third at -a (a within 0.02 m, the same f32), the rest at
    1e-13 m, shuffled.  x and y of a jittered cell lie in one binade and 4096 of them add exactly in f64 in any order; the
    exact sum of these z is that of the tiny ones, what an f64 sum gives depends on the order of its additions by about
    1e-5 of it, and so do the bits of the f32 centre.  The pitch span stays within a tenth of a cell of 0."""
    p, l = part
    n = len(l)
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.005, 0.02, n // 3).astype(np.float32)
    z = np.concatenate([a, -a, rng.uniform(1e-13, 2e-13, n - 2 * (n // 3)).astype(np.float32)])
    rng.shuffle(z)
    p = p.copy()
    p[:, 2] = z
    return p, l


def edge_cfg():
    cfg = ref.default_cfg()
    cfg["min_seg"] = cfg["min_seg"].copy()
    cfg["min_seg"][16] = 5
    return cfg


def seg_cfg(min_seg):
    cfg = ref.default_cfg()
    cfg["min_seg"] = np.full(32, min_seg, np.int64)
    return cfg


def lib_cfg(cfg):
    return None if cfg is None else {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in cfg.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- the comparison of the GPU files ----
def restate(points, labels, off, cfg=None):
    """the restatement of one batch, every scan clear of the rule's rounding boundaries: (res, xyz, label, kp_off, n_points)"""
    off = np.asarray(off, np.int64)
    for s in range(len(off) - 1):
        assert ref.clear_of_boundaries(points[off[s]:off[s + 1]], labels[off[s]:off[s + 1]], cfg), "scan %d sits on a rounding boundary" % s
    return ref.batch_rule(points, labels, off, cfg)


def same_as(h, got, want):
    """the results of the last scan call on handle h (got: what it returned) against the restatement's"""
    res, xyz, lab, kp_off, npts = want
    gx, gl, go, gn = got
    assert np.array_equal(go, kp_off), (go, kp_off)
    assert np.array_equal(gl, lab) and np.array_equal(gn, npts)
    assert np.array_equal(bits(gx), bits(xyz))
    for s, r in enumerate(res):
        assert np.array_equal(h.scan_point_clusters(s), r["cluster"]), s
        grid, rng = h.scan_grids(s)
        assert np.array_equal(grid, r["grid"]), (s, grid[10:19], r["grid"][10:19])
        assert np.array_equal(bits(rng[:, 2:]), bits(r["range"][:, 2:])), s
        assert np.all(np.abs(rng[:, :2] - r["range"][:, :2]) <= 1e-12), s


def run(h, points, labels, off, cfg=None, dev=False):
    """one call on handle h: host arrays, or device tensors"""
    off = np.asarray(off, np.int64)
    if dev:
        import torch
        dp, dl = torch.from_numpy(np.ascontiguousarray(points)).cuda(), torch.from_numpy(labels.view(np.int32)).cuda()
        return h.scan_keypoints(dp, dl, off, lib_cfg(cfg))
    return h.scan_keypoints(points, labels, off, lib_cfg(cfg))


def with_stride(points, stride):
    """the (n, 3) points at stride 3, or at stride 4 with a fourth column the rule does not read"""
    points = np.ascontiguousarray(points[:, :3], np.float32)
    if stride == 3:
        return points
    return np.ascontiguousarray(np.concatenate([points, np.full((len(points), 1), 0.5, np.float32)], axis=1))


# ---- the rounds model ----
def voxel_links(vox, dims, no_wrap=False, cap=None):
    """the occupied voxels of vox (n, 3) pit, pol, azi in key order (the device's voxel indices), the voxel of every point,
    and per voxel the list of its occupied neighbours as scan_links_kernel keeps it (repeats included, itself not)"""
    pn, width, height = dims
    keys = [tuple(int(c) for c in v) for v in vox]
    order = sorted(set(keys))
    index = {k: i for i, k in enumerate(order)}
    links = []
    for k in order:
        nb = ref.neighbours(k[1], k[0], k[2], pn, width, height)
        if no_wrap:
            xs = (k[2] - 1, k[2], k[2] + 1) * (len(nb) // 3)      # the x each entry was made from
            nb = [t for t, x in zip(nb, xs) if x >= 0]
        l = [index[t] for t in nb if t in index and t != k]
        links.append(l if cap is None else l[:cap])
    return order, np.array([index[k] for k in keys], np.int64), links


def hook_rounds(links, limit=None):
    """synchronous hook + jump rounds over the voxels' links: (rounds run, the last one hooking nothing unless `limit`
    ended them first; the root of every voxel)"""
    parent = list(range(len(links)))
    rounds = 0
    while limit is None or rounds < limit:
        rounds += 1
        snap = list(parent)
        hooked = False
        for v, l in enumerate(links):
            for u in l:
                pu, pv = snap[u], snap[v]
                if pu != pv:
                    hi, lo = max(pu, pv), min(pu, pv)
                    parent[hi] = min(parent[hi], lo)
                    hooked = True
        if not hooked:
            break
        for v in range(len(parent)):
            p = parent[v]
            while parent[p] != p:
                p = parent[p]
            parent[v] = p
    return rounds, np.array(parent, np.int64)


def rounds_model(vox, dims):
    """the number of synchronous rounds (one hook, one jump) up to and including the first that hooks nothing"""
    return hook_rounds(voxel_links(vox, dims)[2])[0]


def world_rounds(points, labels, cfg, cls=15):
    """rounds_model of one scan's voxel-mode class"""
    _, vox, dims = ref.voxel_mode_points(points, labels, cls, cfg)
    return rounds_model(vox, dims)


# ---- mutants of the restatement ----
MUTANTS = ("plain_sum", "block_fold", "inst15", "no_wrap", "hook_once", "min_order_by_voxel", "nbr25")


def _block_fold(v):
    """fixed_sum's additions for n >= BIG in another order: the four accumulators l, l + 64, l + 128, l + 192 first"""
    v = np.asarray(v, np.float64)
    acc = np.zeros(256, np.float64)
    for k0 in range(0, v.size, 256):
        part = v[k0:k0 + 256]
        acc[:part.size] = acc[:part.size] + part
    acc = ((acc[0:64] + acc[64:128]) + acc[128:192]) + acc[192:256]
    w = 32
    while w >= 1:
        acc[:w] = acc[:w] + acc[w:2 * w]
        w //= 2
    return acc[0]


def _sum(v, mutant):
    if mutant == "plain_sum":
        return np.float64(np.sum(np.asarray(v, np.float64)))
    if mutant == "block_fold" and len(v) >= BIG:
        return _block_fold(v)
    return ref.fixed_sum(v)


def _components(vox, dims, mutant):
    if mutant not in ("no_wrap", "hook_once", "nbr25"):
        return ref.components(vox, *dims)
    _, of_point, links = voxel_links(vox, dims, no_wrap=mutant == "no_wrap", cap=25 if mutant == "nbr25" else None)
    return hook_rounds(links, limit=1 if mutant == "hook_once" else None)[1][of_point]


def scan_rule(points, labels, cfg=None, mutant=None):
    """_scan_ref.scan_rule with one named change (None: none, and then equal to it)"""
    assert mutant is None or mutant in MUTANTS
    cfg = cfg or ref.default_cfg()
    points = np.asarray(points, np.float32).reshape(-1, points.shape[-1] if points.ndim > 1 else 3)
    labels = np.asarray(labels, np.uint32)
    n = points.shape[0]
    sem, inst = (labels & 0xFFFF).astype(np.int64), (labels >> 16).astype(np.int64)
    if mutant == "inst15":
        inst = inst & 0x7FFF
    kept = ref.kept_mask(points, labels, cfg)
    r, pitch, azimuth = ref.polar(points)
    grid, rng = np.zeros((ref.N_CLASSES, 4), np.int32), np.zeros((ref.N_CLASSES, 4), np.float64)
    cluster = np.full(n, -1, np.int32)
    xyz, lab, cnt = [], [], []
    for s in range(ref.N_CLASSES):
        idx = np.nonzero(kept & (sem == s))[0]
        if idx.size == 0:
            continue
        groups = []
        if np.any(inst[idx] != 0):
            grid[s, 0] = 1
            for v in np.unique(inst[idx]):
                m = idx[inst[idx] == v]
                if m.size > cfg["min_instance_points"]:
                    groups.append((int(v), m))
        else:
            grid[s, 0] = 2
            m = idx[ref.in_range(r[idx], cfg)]
            g4, width, height, bounds = ref.class_grid(r[m], pitch[m], cfg)
            grid[s, 1:] = (len(bounds), width, height)
            rng[s] = g4
            if m.size:
                pol, pit, azi = ref.voxel_indices(r[m], pitch[m], azimuth[m], g4, bounds, cfg)
                vox = np.stack([pit, pol, azi], axis=1)
                comp = _components(vox, (len(bounds), width, height), mutant)
                for c in np.unique(comp):
                    sel = comp == c
                    mm = m[sel]
                    if mm.size >= cfg["min_seg"][s]:
                        first = min(tuple(int(x) for x in v) for v in vox[sel]) if mutant == "min_order_by_voxel" else int(mm[0])
                        groups.append((first, mm))
        for _, m in sorted(groups, key=lambda g: g[0]):
            cluster[m] = len(xyz)
            p64 = points[m, :3].astype(np.float64)
            xyz.append([np.float32(_sum(p64[:, k], mutant) / np.float64(m.size)) for k in range(3)])
            lab.append(int(cfg["node_label"][s]))
            cnt.append(m.size)
    return dict(xyz=np.array(xyz, np.float32).reshape(-1, 3), label=np.array(lab, np.uint32), n_points=np.array(cnt, np.int32),
                cluster=cluster, grid=grid, range=rng)


def same_result(a, b):
    """two results of the rule, compared as the GPU file compares (centres bit for bit)"""
    return (np.array_equal(a["n_points"], b["n_points"]) and np.array_equal(a["label"], b["label"]) and np.array_equal(a["cluster"], b["cluster"])
            and np.array_equal(bits(a["xyz"]), bits(b["xyz"])) and np.array_equal(a["grid"], b["grid"]))


# ---- the worlds: name -> (points (n, 3), labels, pt_off, cfg) ----
PERCOLATION_SEED = 0      # (chosen on the CPU: see test_scan_edges.test_percolation)
PERC_ROWS, PERC_COLS, PERC_P = 12, 280, 0.42


def _one(points, labels, cfg):
    return points, labels, np.array([0, len(labels)], np.int64), cfg


def _big(n):
    return _one(*scene(cancelling(cell(10, 0, R0, n, jitter=0.02, seed=n), n), cancelling(cell(50, 0, R0, 300, jitter=0.02, seed=7), 7)), edge_cfg())


def _big_two():
    # a small cluster ahead of the first big one: the big ones are keypoints 1 and 41 of 42
    parts = [cell(4, 0, R0, 5, jitter=0.02, seed=100), cancelling(cell(10, 0, R0, 4096, jitter=0.02, seed=101), 101)]
    parts += [cell(20 + 3 * k, 0, R0, 5 + k % 4, jitter=0.02, seed=110 + k) for k in range(39)]
    parts += [cancelling(cell(200, 0, R0, 5000, jitter=0.02, seed=102), 102)]
    return _one(*scene(*parts), edge_cfg())


def _big_instance():
    # ids 0xFFFF (kept), 1 (21 points: kept), 2 and 0x7FFF (20 points: dropped); an id cut to 15 bits merges 0x7FFF and 0xFFFF
    return _one(*scene(cancelling(cell(10, 0, R0, 4096, cls=10, inst=0xFFFF, jitter=0.02, seed=120), 120), cell(60, 0, R0, 20, cls=10, inst=2, jitter=0.02, seed=121),
                       cell(90, 0, R0, 20, cls=10, inst=0x7FFF, jitter=0.02, seed=122), cell(120, 0, R0, 21, cls=10, inst=1, jitter=0.02, seed=123)),
                edge_cfg())


SMALL_SUMS = (1, 63, 64, 65, 255)


def _small_sums():
    return _one(*scene(*[cancelling(cell(10 + 10 * k, 0, R0, n, jitter=0.02, seed=130 + k), 130 + k) for k, n in enumerate(SMALL_SUMS)]), seg_cfg(1))


def _block27():
    # (the point at pitch cell 2.7 keeps the pitch span off a whole number of cells, as top_layer's 3.7 does; alone, it is dropped)
    parts = [cell(10 + a, b, r) for b in range(3) for r in (R0, R1, R2) for a in range(3)]
    return _one(*scene(*parts, cell(200, 2.7, R0)), edge_cfg())


def _last_azimuth():
    parts = [cell(a, b, R0) for b in (0, 1) for a in (299, 300, 0.25)]
    return _one(*scene(*parts, cell(150, 1.7, R0)), edge_cfg())


def _zigzag():
    return _one(*scene(*[cell(10 + a, a % 2, R0) for a in range(64)], cell(200, 1.7, R0)), edge_cfg())


def percolation(seed):
    rng = np.random.default_rng(seed)
    occ = rng.random((PERC_ROWS, PERC_COLS)) < PERC_P
    where = [(a, b) for b in range(PERC_ROWS) for a in range(PERC_COLS) if occ[b, a]]
    parts = [cell(10 + a, b, R0) for a, b in (where[k] for k in rng.permutation(len(where)))]      # (point order is not voxel order)
    return _one(*scene(*parts, cell(295, PERC_ROWS - 1 + 0.7, R0)), seg_cfg(2))


def _all_dropped():
    p0, l0 = cell(10, 0, R0, 40, cls=5, jitter=0.02, seed=140)            # a class whose node_label is 0
    p1, l1 = cell(20, 0, R0, 30, cls=40, jitter=0.02, seed=141)           # sem >= 32 ...
    l1[::2] = 15 | (1 << 15)                                              # ... and sem with a high bit
    p2, l2 = cell(30, 0, R0, 50, cls=15, jitter=0.02, seed=142)           # a coordinate that is not finite
    p2[0::3, 0], p2[1::3, 1], p2[2::3, 2] = np.nan, np.inf, -np.inf
    p, l = scene((p0, l0), (p1, l1), (p2, l2))
    return p, l, np.array([0, 40, 70, 120], np.int64), seg_cfg(2)


def _one_live():
    p, l, off, _ = _all_dropped()
    q, m = cell(40, 0, R0)
    return np.concatenate([p, q]), np.concatenate([l, m]), np.array([0, 40, 70, 121], np.int64), seg_cfg(1)


def _scans_257():
    rng = np.random.default_rng(150)
    parts, off = [], [0]
    for s in range(257):
        if s % 16 != 15:
            n = int(rng.integers(4, 10))
            a = 10 + (7 * s) % 280
            if s % 4 == 1:      # two cells
                parts += [cell(a, 0, R0, n // 2, jitter=0.02, seed=1000 + s), cell(a + 3, 0, R1, n - n // 2, jitter=0.02, seed=2000 + s)]
            else:
                parts += [cell(a, 0, R0, n, jitter=0.02, seed=1000 + s)]
            off.append(off[-1] + n)
        else:
            off.append(off[-1])
    p, l = scene(*parts)
    return p, l, np.array(off, np.int64), seg_cfg(2)


WORLDS = {
    "big-4095": lambda: _big(4095), "big-4096": lambda: _big(4096), "big-4097": lambda: _big(4097), "big-two": _big_two,
    "big-instance": _big_instance, "small-sums": _small_sums, "block27": _block27, "last-azimuth": _last_azimuth, "zigzag": _zigzag,
    "percolation": lambda: percolation(PERCOLATION_SEED), "all-dropped": _all_dropped, "one-live": _one_live, "257-scans": _scans_257,
}
FIVE = ("big-4096", "big-two", "percolation", "257-scans", "all-dropped")      # the worlds that run in every form


@functools.lru_cache(maxsize=None)
def world(name):
    return WORLDS[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement of a world, computed once (read, never written)"""
    p, l, off, cfg = world(name)
    return restate(p, l, off, cfg)


@functools.lru_cache(maxsize=None)
def concatenated():
    """FIVE in one batch under min_seg 2: points, labels, pt_off, cfg"""
    ws = [world(k) for k in FIVE]
    off = [np.zeros(1, np.int64)]
    for _, l, o, _ in ws:
        off.append(o[1:] + off[-1][-1])
    return np.concatenate([w[0] for w in ws]), np.concatenate([w[1] for w in ws]), np.concatenate(off), seg_cfg(2)


@functools.lru_cache(maxsize=None)
def expected_concatenated():
    return restate(*concatenated())


def too_many_scans():
    """MAX_SCANS + 1 scans of one point"""
    p, l = cell(10, 0, R0, MAX_SCANS + 1)
    return p, l, np.arange(MAX_SCANS + 2, dtype=np.int64)
