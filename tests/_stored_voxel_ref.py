"""numpy restatement of sgtd_register_stored_local_loops' forming rule as include/sgtd_accel.h states it: eligible frames,
rows, maps, members and member poses.  All arithmetic is f64 on the stored f32 poses widened exactly, every operation
rounded once and written out (no @, no dot, no sum): the device's bits."""
import numpy as np

EYE = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])


def widen(pose12):
    """a stored pose (12 f32, row-major 3x4 [R | t]) -> the rel_pose layout in f64: R row-major, then t"""
    m = np.asarray(pose12, np.float32).astype(np.float64).reshape(3, 4)
    return np.concatenate([m[:, :3].reshape(9), m[:, 3]])


def inv(x):
    y = np.zeros(12)
    for r in range(3):
        for c in range(3):
            y[r * 3 + c] = x[c * 3 + r]
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            y[9 + r] = -((y[r * 3 + 0] * x[9] + y[r * 3 + 1] * x[10]) + y[r * 3 + 2] * x[11])
    return y


def mul(x, y):
    z = np.zeros(12)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            for c in range(3):
                z[r * 3 + c] = (x[r * 3 + 0] * y[c] + x[r * 3 + 1] * y[3 + c]) + x[r * 3 + 2] * y[6 + c]
            z[9 + r] = ((x[r * 3 + 0] * y[9] + x[r * 3 + 1] * y[10]) + x[r * 3 + 2] * y[11]) + x[9 + r]
    return z


def eligible(has_cloud, poses):
    """the eligible frame ids, ascending.  has_cloud: the ids with a stored cloud; poses: {id: 12 f32}, the stored poses"""
    return sorted(int(i) for i in poses if int(i) in has_cloud and np.isfinite(np.asarray(poses[i], np.float32)).all())


def rows(score, n_cand, cand_frame, rel_pose, max_per_query, cand_num, elig):
    """score [nq][cn], n_cand [nq], cand_frame [nq][cn], rel_pose [nq][cn][12] of the named stage -> [(query, cand, frame,
    init [12])] in (query, rank) order"""
    elig = set(elig)
    out = []
    for q in range(len(n_cand)):
        ok = [c for c in range(min(int(n_cand[q]), cand_num)) if score[q][c] >= 0]
        ok = sorted(ok, key=lambda c: (-score[q][c], c))[:min(max_per_query, cand_num)]
        out += [(q, c, int(cand_frame[q][c]), np.asarray(rel_pose[q][c], np.float64).reshape(12)) for c in ok if int(cand_frame[q][c]) in elig]
    return out


def members(j, elig, poses, radius, max_members=0):
    """the members of the map of frame j: j first, the others in ascending id"""
    t = {i: np.asarray(poses[i], np.float32).astype(np.float64)[[3, 7, 11]] for i in elig}
    rr = np.float64(radius) * np.float64(radius)
    d2 = {}
    for i in elig:
        if i == j:
            continue
        dx, dy, dz = t[i][0] - t[j][0], t[i][1] - t[j][1], t[i][2] - t[j][2]
        d2[i] = (dx * dx + dy * dy) + dz * dz
    others = [i for i in sorted(d2) if d2[i] <= rr]
    if max_members > 0 and len(others) > max_members - 1:
        others = sorted(sorted(others, key=lambda i: (d2[i], i))[:max_members - 1])
    return [int(j)] + others


def member_poses(mem, poses):
    """[k, 12]: the identity, written out, for mem[0]; mul(inv(T_j), T_i) for the others"""
    out = np.zeros((len(mem), 12))
    out[0] = EYE
    ij = inv(widen(poses[mem[0]]))
    for k in range(1, len(mem)):
        out[k] = mul(ij, widen(poses[mem[k]]))
    return out


def form(score, n_cand, cand_frame, rel_pose, max_per_query, cand_num, has_cloud, poses, radius, max_members=0):
    """-> dict of query, cand, frame, tgt_map [m], init [m, 12], map_frames, members (per map), map_off, map_frame (all
    members), map_pose [members, 12]"""
    elig = eligible(has_cloud, poses)
    r = rows(score, n_cand, cand_frame, rel_pose, max_per_query, cand_num, elig)
    map_frames = sorted(set(x[2] for x in r))
    mem = [members(j, elig, poses, radius, max_members) for j in map_frames]
    rel = [member_poses(m, poses) for m in mem]
    return dict(query=np.array([x[0] for x in r], np.int32), cand=np.array([x[1] for x in r], np.int32), frame=np.array([x[2] for x in r], np.int32),
                tgt_map=np.array([map_frames.index(x[2]) for x in r], np.int32), init=np.array([x[3] for x in r], np.float64).reshape(-1, 12),
                map_frames=map_frames, members=mem, map_off=np.concatenate([[0], np.cumsum([len(m) for m in mem])]).astype(np.int32),
                map_frame=np.array([i for m in mem for i in m], np.uint32), map_pose=np.concatenate(rel).reshape(-1, 12) if rel else np.zeros((0, 12)))
