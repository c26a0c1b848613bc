"""Planted worlds for sgtd_local_map_keypoints' structural edges and mutants of the restatement
(tests/_local_map_ref.py).  tests/test_local_map_edges.py shows on the CPU that every world reaches the edge it is named
for and that every mutant changes the world listed with it; tests/test_gpu_local_map_edges.py runs every form of the
call on the worlds and compares exactly.

The member rule depends on poses only, so the worlds keep the clustering trivial and exact: every point is of class 10
in instance mode (inst = scan % 7 + 1) with min_instance_points 0.  _scan_ref.clear_of_boundaries then has nothing to
reject, and every keypoint is an instance group that mixes points of many members: a centre compared bit for bit checks
the gather's transform and the merged order, because a point's rank in its cluster picks its accumulator.

The edges (local_map_kernels.hip.h, local_map_run in sgtd_accel.hip):
  lattice-600    lm_members_kernel on more scans than threads: thread t owns scans 16 t .. 16 t + 15, the strided loops
                 take a second and a third step; the max_members cut with more candidates than threads and ties at the cut
  full-lds       n_scans == SGTD_LM_MAX_SCANS: the last LDS slot, thread 255's range ending at the array's end
  rotated-600    general rotations through every gather kernel, lm_gather_kernel<4, false> among them
  anchors-4097   the pass planner's split after SGTD_SCAN_MAX_SCANS anchors; scan_device with S = 4096"""
import functools

import numpy as np

import _local_map_ref as ref
import _scan_ref as sref

MAX_SCANS = 4096      # SGTD_LM_MAX_SCANS == SGTD_SCAN_MAX_SCANS
PER = 16              # SGTD_LM_PER: consecutive scans owned by one thread of lm_members_kernel
UNSUPPORTED = -6      # SGTD_ERR_UNSUPPORTED


def inst_cfg():
    cfg = sref.default_cfg()
    cfg["min_instance_points"] = 0
    return cfg


def lib_cfg(cfg):
    return None if cfg is None else {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in cfg.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def eye_poses(t):
    """identity rotations at the translations t (n, 3)"""
    t = np.asarray(t, np.float32).reshape(-1, 3)
    p = np.zeros((len(t), 12), np.float32)
    p[:, [0, 5, 10]] = 1.0
    p[:, [3, 7, 11]] = t
    return p


def euler_poses(n, seed, t=None):
    """general rotations (yaw, pitch, roll) rounded to f32 — not exactly orthonormal — a few metres apart, or at the
    translations t (n, 3)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 3, 4))
    for k in range(n):
        y, p, r = rng.uniform(-np.pi, np.pi), rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4)
        rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
        ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
        rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
        out[k, :, :3] = rz @ ry @ rx
        out[k, :, 3] = rng.uniform(-3.0, 3.0, 3)
    if t is not None:
        out[:, :, 3] = np.asarray(t, np.float64).reshape(n, 3)
    return out.reshape(n, 12).astype(np.float32)


def inst_scans(counts, seed):
    """scans of counts[k] points within 8 m of the sensor, class 10, instance scan % 7 + 1: points (n, 3), labels, pt_off"""
    counts = np.asarray(counts, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    p = np.random.default_rng(seed).uniform(-8.0, 8.0, (int(off[-1]), 3)).astype(np.float32)
    scan = np.repeat(np.arange(len(counts)), counts)
    return p, (10 | ((scan % 7 + 1) << 16)).astype(np.uint32), off


def with_stride(points, stride):
    points = np.ascontiguousarray(points[:, :3], np.float32)
    if stride == 3:
        return points
    return np.ascontiguousarray(np.concatenate([points, np.full((len(points), 1), 0.5, np.float32)], axis=1))


# ---- mutants of the member rule ----
MUTANTS = ("tie_high", "cut_without_anchor", "rank_order")


def members(poses, j, radius=15.0, max_members=0, mutant=None):
    """_local_map_ref.members with one named change (None: none)"""
    assert mutant is None or mutant in MUTANTS
    poses = np.asarray(poses, np.float32).reshape(-1, 12)
    t = poses[:, [3, 7, 11]].astype(np.float64)
    d = t - t[j]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    rr = np.float64(radius) * np.float64(radius)
    others = [i for i in range(len(poses)) if i != j and d2[i] <= rr]
    keep = max_members if mutant == "cut_without_anchor" else max_members - 1
    if max_members > 0 and len(others) > keep:
        ranked = sorted(others, key=lambda i: (d2[i], -i if mutant == "tie_high" else i))[:keep]
        others = ranked if mutant == "rank_order" else sorted(ranked)
    return [j] + others


def cut(poses, j, radius, max_members):
    """the candidates of anchor j in (d2, index) rank: (d2, index) of the last kept and of the first cut"""
    t = np.asarray(poses, np.float32).reshape(-1, 12)[:, [3, 7, 11]].astype(np.float64)
    d2 = ((t - t[j]) ** 2).sum(axis=1)
    ranked = sorted((i for i in range(len(t)) if i != j and d2[i] <= radius * radius), key=lambda i: (d2[i], i))
    if len(ranked) < max_members:
        return None
    a, b = ranked[max_members - 2], ranked[max_members - 1]
    return (d2[a], a), (d2[b], b)


def f32_transform_cloud(points, labels, pt_off, poses, mem):
    """_local_map_ref.merged_cloud with the product inv(T_j) . T_i rounded to f32 before it is applied"""
    points = np.asarray(points, np.float32)
    poses = np.asarray(poses, np.float32).reshape(-1, 12)
    j = mem[0]
    tj_inv = ref.inv(ref.rt(poses[j]))
    xyz, lab = [points[pt_off[j]:pt_off[j + 1], :3].copy()], [labels[pt_off[j]:pt_off[j + 1]]]
    for i in mem[1:]:
        m, t = ref.mul(tj_inv, ref.rt(poses[i]))
        m, t = m.astype(np.float32).astype(np.float64), t.astype(np.float32).astype(np.float64)
        p = points[pt_off[i]:pt_off[i + 1], :3].astype(np.float64)
        q = np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + t[r] for r in range(3)], axis=1).astype(np.float32)
        xyz.append(q)
        lab.append(labels[pt_off[i]:pt_off[i + 1]])
    return np.concatenate(xyz).reshape(-1, 3), np.concatenate(lab).astype(np.uint32)


# ---- the worlds: name -> dict(p, l, off, poses, cfg, kw) ----
LATTICE_SEED = 0      # (chosen on the CPU: see test_local_map_edges.test_lattice_600)
LATTICE_ANCHORS = [0, 15, 16, 17, 255, 256, 257, 599]
LATTICE_RADIUS = 12.0
LATTICE_SHIFT = 592
CUTS = (2, 17, 257, 258)
ROTATED_RADIUS = 3.5
ROTATED_ANCHORS = [0, 15, 16, 17, 100, 255, 256, 257, 300, 431, 592, 599]


def lattice_translations(seed):
    """the 600 points of the 25 x 24 integer lattice dealt to the scan indices: runs of 16 points along a lattice row go to
    the 16 scans one thread of lm_members_kernel owns, the runs and the points inside a run in a seeded order (the eight
    points left over go to the last scans)"""
    rng = np.random.default_rng(seed)
    q = []
    for c in rng.permutation(37):
        q += [16 * c + k for k in rng.permutation(16)]
    q = (np.array(q + list(range(592, 600))) + LATTICE_SHIFT) % 600      # (the left-over run: the middle of the last lattice row)
    return np.stack([q // 24, q % 24, np.zeros(600, np.int64)], axis=1).astype(np.float32)


def _world(p, l, off, poses, **kw):
    return dict(p=p, l=l, off=off, poses=poses, cfg=inst_cfg(), kw=kw)


def _lattice(max_members=0):
    p, l, off = inst_scans(1 + np.arange(600) % 3, 600)
    return _world(p, l, off, eye_poses(lattice_translations(LATTICE_SEED)), radius=LATTICE_RADIUS, anchors=LATTICE_ANCHORS, max_members=max_members)


def _rotated():
    p, l, off = inst_scans(1 + np.arange(600) % 3, 600)
    return _world(p, l, off, euler_poses(600, 601, lattice_translations(LATTICE_SEED)), radius=ROTATED_RADIUS, anchors=ROTATED_ANCHORS)


FULL_LIVE = {0: 120, 7: 50, 16: 200, 255: 64, 256: 75, 1000: 90, 2047: 150, 4079: 55, 4080: 170, 4095: 101}


def _full_lds():
    counts = np.zeros(MAX_SCANS, np.int64)
    for k, n in FULL_LIVE.items():
        counts[k] = n
    p, l, off = inst_scans(counts, 4096)
    t = np.zeros((MAX_SCANS, 3))
    t[:, 0] = 0.5 * np.arange(MAX_SCANS)      # a line, half a metre a scan ...
    t[4080], t[4095] = (1.0, 2.0, 0.0), (-1.0, 3.0, 0.5)      # ... and the last two back at its start
    return _world(p, l, off, euler_poses(MAX_SCANS, 4097, t), radius=15.0, anchors=[0, 4080, 4095])


def _anchors_4097():
    p, l, off = inst_scans([2, 1, 2], 3)
    return _world(p, l, off, eye_poses([[0, 0, 0], [1, 0, 0], [2, 0, 0]]), radius=5.0, anchors=(np.arange(MAX_SCANS + 1) % 3).tolist())


WORLDS = {"lattice-600": _lattice, "lattice-600-cut-2": lambda: _lattice(2), "lattice-600-cut-17": lambda: _lattice(17),
          "lattice-600-cut-257": lambda: _lattice(257), "lattice-600-cut-258": lambda: _lattice(258), "rotated-600": _rotated,
          "full-lds": _full_lds, "anchors-4097": _anchors_4097}


@functools.lru_cache(maxsize=None)
def world(name):
    return WORLDS[name]()


def restate(p, l, off, poses, cfg, **kw):
    want = ref.local_map_rule(p, l, off, poses, anchors=kw.get("anchors"), radius=kw.get("radius", 15.0), max_members=kw.get("max_members", 0),
                              cfg=cfg)
    for a, (xyz, lab) in enumerate(want["clouds"]):
        assert sref.clear_of_boundaries(xyz, lab, cfg), "the merged cloud of anchor %d sits on a rounding boundary" % a
    return want


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement of a world, computed once (read, never written)"""
    w = world(name)
    return restate(w["p"], w["l"], w["off"], w["poses"], w["cfg"], **w["kw"])


def same_as(h, got, want, max_pass_points=0):
    gx, gl, go, gn = got
    assert np.array_equal(go, want["kp_off"]), (go, want["kp_off"])
    assert np.array_equal(gl, want["label"]) and np.array_equal(gn, want["n_points"])
    assert np.array_equal(bits(gx), bits(want["xyz"]))
    mem_off, member, merged, n_passes = h.local_map_members()
    assert np.array_equal(mem_off, want["mem_off"]) and np.array_equal(member, want["member"]), (member, want["member"])
    assert np.array_equal(merged, want["merged_points"])
    assert n_passes == ref.plan_passes(want["merged_points"], max_pass_points)


def too_many_scans():
    """MAX_SCANS + 1 scans of one point a millimetre apart"""
    p, l, off = inst_scans(np.ones(MAX_SCANS + 1, np.int64), 4098)
    t = np.zeros((MAX_SCANS + 1, 3))
    t[:, 0] = 0.001 * np.arange(MAX_SCANS + 1)
    return p, l, off, eye_poses(t)
