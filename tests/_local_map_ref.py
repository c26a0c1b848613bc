"""numpy restatement of sgtd_local_map_keypoints' rule (include/sgtd_accel.h): the member rule, inv / mul in the
header's operation order, the merged cloud, and then _scan_ref.scan_rule on it."""
import numpy as np

import _scan_ref as sref


def rt(pose12):
    """a pose row (12 f32, row-major 3x4) widened exactly: R (3, 3), t (3,) in f64"""
    m = np.asarray(pose12, np.float32).astype(np.float64).reshape(3, 4)
    return m[:, :3].copy(), m[:, 3].copy()


def inv(x):
    r, t = x
    ri = r.T.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        ti = np.array([-((ri[k, 0] * t[0] + ri[k, 1] * t[1]) + ri[k, 2] * t[2]) for k in range(3)])
    return ri, ti


def mul(x, y):
    xr, xt = x
    yr, yt = y
    r, t = np.zeros((3, 3)), np.zeros(3)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(3):
            for c in range(3):
                r[k, c] = (xr[k, 0] * yr[0, c] + xr[k, 1] * yr[1, c]) + xr[k, 2] * yr[2, c]
            t[k] = ((xr[k, 0] * yt[0] + xr[k, 1] * yt[1]) + xr[k, 2] * yt[2]) + xt[k]
    return r, t


def members(poses, j, radius=15.0, max_members=0):
    """the member list of anchor j: j first, then the others in ascending index"""
    poses = np.asarray(poses, np.float32).reshape(-1, 12)
    t = poses[:, [3, 7, 11]].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = t - t[j]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        rr = np.float64(radius) * np.float64(radius)
        others = [i for i in range(len(poses)) if i != j and d2[i] <= rr]
    if max_members > 0 and len(others) > max_members - 1:
        others = sorted(sorted(others, key=lambda i: (d2[i], i))[:max_members - 1])
    return [j] + others


def merged_cloud(points, labels, pt_off, poses, mem):
    """xyz (n, 3) f32 and labels of the local map whose member list is mem (the anchor first)"""
    points = np.asarray(points, np.float32)
    poses = np.asarray(poses, np.float32).reshape(-1, 12)
    j = mem[0]
    tj_inv = inv(rt(poses[j]))
    xyz, lab = [points[pt_off[j]:pt_off[j + 1], :3].copy()], [labels[pt_off[j]:pt_off[j + 1]]]
    for i in mem[1:]:
        m, t = mul(tj_inv, rt(poses[i]))
        p = points[pt_off[i]:pt_off[i + 1], :3].astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            q = np.stack([((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + t[r] for r in range(3)], axis=1).astype(np.float32)
        xyz.append(q)
        lab.append(labels[pt_off[i]:pt_off[i + 1]])
    return np.concatenate(xyz).reshape(-1, 3), np.concatenate(lab).astype(np.uint32)


def local_map_rule(points, labels, pt_off, poses, anchors=None, radius=15.0, max_members=0, cfg=None):
    """dict of: res (the scan rule's result per anchor), xyz, label, kp_off, n_points (concatenated), mem_off, member,
    merged_points, clouds (the merged xyz, labels per anchor)"""
    pt_off = np.asarray(pt_off, np.int64)
    n = len(pt_off) - 1
    anchors = list(range(n)) if anchors is None else [int(a) for a in anchors]
    res, mems, clouds = [], [], []
    for j in anchors:
        mem = members(poses, j, radius, max_members)
        xyz, lab = merged_cloud(points, labels, pt_off, poses, mem)
        mems.append(mem)
        clouds.append((xyz, lab))
        res.append(sref.scan_rule(xyz, lab, cfg))
    cat = lambda k, shape, dt: (np.concatenate([r[k] for r in res]) if res else np.zeros(shape, dt))
    return dict(res=res, xyz=cat("xyz", (0, 3), np.float32).reshape(-1, 3), label=cat("label", 0, np.uint32), n_points=cat("n_points", 0, np.int32),
                kp_off=np.concatenate([[0], np.cumsum([len(r["label"]) for r in res])]).astype(np.int64),
                mem_off=np.concatenate([[0], np.cumsum([len(m) for m in mems])]).astype(np.int64),
                member=np.array([i for m in mems for i in m], np.int32), merged_points=np.array([len(c[1]) for c in clouds], np.int64),
                clouds=clouds)


def path_poses(n, step=(3.0, 0.5, 0.3), yaw=0.05):
    """(n, 12) f32 poses along a path: scan k at k * step metres, turned by k * yaw about z"""
    p = np.zeros((n, 3, 4), np.float64)
    k = np.arange(n)
    p[:, 0, 0], p[:, 0, 1], p[:, 1, 0], p[:, 1, 1], p[:, 2, 2] = np.cos(k * yaw), -np.sin(k * yaw), np.sin(k * yaw), np.cos(k * yaw), 1.0
    p[:, :, 3] = k[:, None] * np.asarray(step)[None, :]
    return p.reshape(n, 12).astype(np.float32)


def small_cfg(min_seg=2):
    cfg = sref.default_cfg()
    cfg["min_seg"] = np.full(32, min_seg, np.int64)
    return cfg


def plan_passes(merged_points, max_pass_points):
    """the number of passes: consecutive anchors share one while the sum of their merged sizes stays within the cap"""
    cap = max_pass_points if max_pass_points > 0 else 1 << 26
    passes, room, held = 0, -1, 0
    for m in merged_points:
        assert m <= cap
        if room < 0 or m > room or held == 4096:      # (SGTD_SCAN_MAX_SCANS anchors a pass at the most)
            passes, room, held = passes + 1, cap, 0
        room -= m
        held += 1
    return passes
