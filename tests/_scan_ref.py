"""numpy restatement of sgtd_scan_keypoints' rule (include/sgtd_accel.h), a literal restatement of the reference's
sweep (src/sgtd/include/cluster_manager.hpp:148-421), and the boundary check every exact comparison asserts first."""
import numpy as np

N_CLASSES = 32
MARGIN = 1e-9


def default_cfg():
    node_label = np.zeros(N_CLASSES, np.int64)
    node_label[10:19] = np.arange(3, 12)
    min_seg = np.full(N_CLASSES, 300, np.int64)
    min_seg[[15, 17, 18]] = 5
    return dict(node_label=node_label, min_seg=min_seg, min_instance_points=20, start_r=0.35, delta_r=0.0004, delta_p=1.2,
                delta_a=1.2, min_range=0.5, max_range=120.0)


def c_round(v):
    """C's round: halves away from zero"""
    v = np.asarray(v, np.float64)
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)


def polar(xyz):
    """r, pitch, azimuth in f64, one rounding per operation (cluster_manager.hpp:178-196)"""
    x, y, z = (xyz[:, k].astype(np.float64) for k in range(3))
    r = np.sqrt((x * x + y * y) + z * z)
    with np.errstate(invalid="ignore", divide="ignore"):
        pitch = (np.arcsin(z / r) * 180.0) / np.pi
    a = np.arctan2(y, x)
    azimuth = (np.where(a > 0.0, a, a + 2.0 * np.pi) * 180.0) / np.pi
    return r, pitch, azimuth


def kept_mask(xyz, labels, cfg):
    sem = labels & 0xFFFF
    ok = sem < N_CLASSES
    ok &= np.asarray(cfg["node_label"])[np.minimum(sem, N_CLASSES - 1)] != 0
    ok &= np.isfinite(xyz[:, :3].astype(np.float64)).all(axis=1)
    return ok


def in_range(r, cfg):
    return ~(r >= cfg["max_range"]) & ~(r <= cfg["min_range"])


def class_grid(r, pitch, cfg):
    """of the in-range points of one voxel-mode class: (minPitch, maxPitch, minPolar, maxPolar), width, height, bounds"""
    min_pitch = min(0.0, float(pitch.min())) if pitch.size else 0.0
    max_pitch = max(0.0, float(pitch.max())) if pitch.size else 0.0
    min_polar = min(5.0, float(r.min())) if r.size else 5.0
    max_polar = max(5.0, float(r.max())) if r.size else 5.0
    width = int(c_round(360.0 / cfg["delta_a"]) + 1.0)
    height = int((max_pitch - min_pitch) / cfg["delta_p"])
    bounds, rg, step = [], min_polar, 1
    while rg <= max_polar:
        rg = rg + (cfg["start_r"] - step * cfg["delta_r"])
        bounds.append(rg)
        step += 1
    return (min_pitch + 0.0, max_pitch + 0.0, min_polar, max_polar), width, height, np.array(bounds, np.float64)


def voxel_indices(r, pitch, azimuth, rng, bounds, cfg):
    pn = len(bounds)
    pol = np.searchsorted(bounds, r, side="right")      # the first k with r < bounds[k]
    pol = np.where(pol < pn, pol, pn - 1)
    pit = c_round((pitch - rng[0]) / cfg["delta_p"]).astype(np.int64)
    azi = c_round(azimuth / cfg["delta_a"]).astype(np.int64)
    return pol.astype(np.int64), pit, azi


def neighbours(pol, pit, azi, pn, width, height):
    """searchKNN's list (:365-385), in its order, the 300 read as width - 1: (z, y, ax) triples"""
    out = []
    for z in range(pit - 1, pit + 2):
        if z < 0 or z > height:
            continue
        for y in range(pol - 1, pol + 2):
            if y < 0 or y > pn:
                continue
            for x in range(azi - 1, azi + 2):
                ax = x
                if ax < 0:
                    ax = width - 1
                if ax > width - 1:
                    ax = width - 1
                out.append((z, y, ax))
    return out


def components(vox, pn, width, height):
    """connected components of the symmetrised voxel graph: per point the smallest voxel key's ... a label per point
    (equal labels = one component); vox: (n, 3) pit, pol, azi"""
    keys = [tuple(int(c) for c in v) for v in vox]
    occupied = {}
    for k in keys:
        occupied.setdefault(k, len(occupied))
    parent = list(range(len(occupied)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for k, i in occupied.items():
        for nb in neighbours(k[1], k[0], k[2], pn, width, height):
            j = occupied.get(nb)
            if j is not None and j != i:
                ra, rb = find(i), find(j)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(occupied[k]) for k in keys], np.int64)


def fixed_sum(v):
    """256 accumulators from +0.0, rank k to accumulator k mod 256 in ascending k, then the fold w = 128 .. 1"""
    v = np.asarray(v, np.float64)
    acc = np.zeros(256, np.float64)
    for k0 in range(0, v.size, 256):
        part = v[k0:k0 + 256]
        acc[:part.size] = acc[:part.size] + part
    w = 128
    while w >= 1:
        acc[:w] = acc[:w] + acc[w:2 * w]
        w //= 2
    return acc[0]


def scan_rule(points, labels, cfg=None):
    """one scan: dict of xyz (K, 3) f32, label (K,) u32, n_points (K,) i32, cluster (n,) i32, grid (32, 4) i32,
    range (32, 4) f64"""
    cfg = cfg or default_cfg()
    points = np.asarray(points, np.float32).reshape(-1, points.shape[-1] if points.ndim > 1 else 3)
    labels = np.asarray(labels, np.uint32)
    n = points.shape[0]
    sem, inst = (labels & 0xFFFF).astype(np.int64), (labels >> 16).astype(np.int64)
    kept = kept_mask(points, labels, cfg)
    r, pitch, azimuth = polar(points)
    grid, rng = np.zeros((N_CLASSES, 4), np.int32), np.zeros((N_CLASSES, 4), np.float64)
    cluster = np.full(n, -1, np.int32)
    xyz, lab, cnt = [], [], []
    for s in range(N_CLASSES):
        idx = np.nonzero(kept & (sem == s))[0]
        if idx.size == 0:
            continue
        groups = []      # (order, member indices ascending)
        if np.any(inst[idx] != 0):
            grid[s, 0] = 1
            for v in np.unique(inst[idx]):
                m = idx[inst[idx] == v]
                if m.size > cfg["min_instance_points"]:
                    groups.append((int(v), m))
        else:
            grid[s, 0] = 2
            m = idx[in_range(r[idx], cfg)]
            g4, width, height, bounds = class_grid(r[m], pitch[m], cfg)
            grid[s, 1:] = (len(bounds), width, height)
            rng[s] = g4
            if m.size:
                pol, pit, azi = voxel_indices(r[m], pitch[m], azimuth[m], g4, bounds, cfg)
                comp = components(np.stack([pit, pol, azi], axis=1), len(bounds), width, height)
                for c in np.unique(comp):
                    mm = m[comp == c]
                    if mm.size >= cfg["min_seg"][s]:
                        groups.append((int(mm[0]), mm))
        for _, m in sorted(groups, key=lambda g: g[0]):
            cluster[m] = len(xyz)
            p64 = points[m, :3].astype(np.float64)
            xyz.append([np.float32(fixed_sum(p64[:, k]) / np.float64(m.size)) for k in range(3)])
            lab.append(int(cfg["node_label"][s]))
            cnt.append(m.size)
    return dict(xyz=np.array(xyz, np.float32).reshape(-1, 3), label=np.array(lab, np.uint32), n_points=np.array(cnt, np.int32),
                cluster=cluster, grid=grid, range=rng)


def batch_rule(points, labels, pt_off, cfg=None):
    """a batch: the scans' results and the concatenated keypoints (xyz, label, kp_off, n_points)"""
    res = [scan_rule(points[pt_off[s]:pt_off[s + 1]], labels[pt_off[s]:pt_off[s + 1]], cfg) for s in range(len(pt_off) - 1)]
    kp_off = np.concatenate([[0], np.cumsum([len(r["label"]) for r in res])]).astype(np.int64)
    cat = lambda k, shape, dt: (np.concatenate([r[k] for r in res]) if res else np.zeros(shape, dt))
    return res, cat("xyz", (0, 3), np.float32), cat("label", 0, np.uint32), kp_off, cat("n_points", 0, np.int32)


def voxel_mode_points(points, labels, cls, cfg=None):
    """of one scan: the in-range kept points of class cls (indices), their voxels (pit, pol, azi) and (pn, width, height)"""
    cfg = cfg or default_cfg()
    points = np.asarray(points, np.float32)
    labels = np.asarray(labels, np.uint32)
    r, pitch, azimuth = polar(points)
    m = np.nonzero(kept_mask(points, labels, cfg) & ((labels & 0xFFFF) == cls) & in_range(r, cfg))[0]
    g4, width, height, bounds = class_grid(r[m], pitch[m], cfg)
    pol, pit, azi = voxel_indices(r[m], pitch[m], azimuth[m], g4, bounds, cfg)
    return m, np.stack([pit, pol, azi], axis=1), (len(bounds), width, height)


def sweep(vox, dims):
    """DCVC() as the reference runs it (cluster_manager.hpp:224-355) over points whose voxels are vox (n, 3) pit, pol,
    azi, in their order: createHashTable's lists in point order, searchKNN's neighbour order, the relabelling sweep.
    Returns a label per point (> 0)."""
    pn, width, height = dims
    n = len(vox)
    vmap = {}
    keys = [tuple(int(c) for c in v) for v in vox]
    for i, k in enumerate(keys):
        vmap.setdefault(k, []).append(i)
    label = np.full(n, -1, np.int64)
    count = 0
    for i in range(n):
        if label[i] != -1:
            continue
        pit, pol, azi = keys[i]
        nbrs = []
        for nb in neighbours(pol, pit, azi, pn, width, height):
            nbrs.extend(vmap.get(nb, ()))
        for j in nbrs:
            cur, nei = label[i], label[j]
            if cur != -1 and nei != -1 and cur != nei:
                label[label == cur] = nei
            elif nei != -1:
                label[i] = nei
            elif cur != -1:
                label[j] = cur
        if label[i] == -1:
            count += 1
            label[i] = count
            for j in nbrs:
                label[j] = count
    return label


def _half_margin(v):
    """distance of v from the nearest half-integer"""
    f = v - np.floor(v)
    return np.abs(f - 0.5)


def clear_of_boundaries(points, labels, cfg=None, margin=MARGIN):
    """true when every in-range point of every voxel-mode class keeps `margin` from a rounding boundary: (pitch -
    minPitch) / delta_p and azimuth / delta_a from a half-integer, r from every ring bound and both range gates, and
    (maxPitch - minPitch) / delta_p from an integer"""
    cfg = cfg or default_cfg()
    points = np.asarray(points, np.float32)
    labels = np.asarray(labels, np.uint32)
    if points.shape[0] == 0:
        return True
    sem, inst = labels & 0xFFFF, labels >> 16
    kept = kept_mask(points, labels, cfg)
    r, pitch, azimuth = polar(points)
    for s in range(N_CLASSES):
        idx = np.nonzero(kept & (sem == s))[0]
        if idx.size == 0 or np.any(inst[idx] != 0):
            continue
        if np.any(np.abs(r[idx] - cfg["max_range"]) < margin) or np.any(np.abs(r[idx] - cfg["min_range"]) < margin):
            return False
        m = idx[in_range(r[idx], cfg)]
        g4, _, _, bounds = class_grid(r[m], pitch[m], cfg)
        h = (g4[1] - g4[0]) / cfg["delta_p"]
        if abs(h - np.round(h)) < margin and h > margin:
            return False
        if m.size == 0:
            continue
        if np.any(_half_margin((pitch[m] - g4[0]) / cfg["delta_p"]) < margin) or np.any(_half_margin(azimuth[m] / cfg["delta_a"]) < margin):
            return False
        if np.any(np.abs(r[m][:, None] - bounds[None, :]) < margin):
            return False
    return True
