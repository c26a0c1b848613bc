"""numpy restatement of sgtd_register_voxels' rule, written from the comment in include/sgtd_accel.h and from nothing
else.  It does not call the library.  The parts the rule shares with sgtd_register_clouds' (mul3, the covariances, SUM,
the residual's "M v", the damped solve, UNIT, ROT) are _register_ref's and _relax_ref's; every elementwise numpy operation
on float64 arrays and every Python float operation is one IEEE rounding and the sums are taken in the header's order, so
every number here is the device's to the bit.

Clouds are (n, 3) float64 arrays of exactly widened f32 values; poses are rows of 12 (rot row-major, t)."""
import numpy as np

import _register_ref as g
import _relax_ref as rr

VW = 64
HALF = 32768
CONVERGED, ITERATION_LIMIT, LM_FAILED, NO_CORRESPONDENCE, NO_POINTS = 0, 1, 2, 3, 4
DEFAULTS = dict(voxel_resolution=1.0, neighbor_mode=1, k_neighbors=20, max_iterations=64, lm_max_trials=10,
                lm_init_lambda_factor=1e-9, rotation_eps=2e-3, translation_eps=5e-4, plane_eps=1e-3, reserved=0)
INF = float("inf")
IDENTITY = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])


def offsets(mode):
    """the neighbourhood of a mode, in the header's order -> [mode, 3] int64"""
    if mode == 1:
        return np.array([[0, 0, 0]], np.int64)
    if mode == 7:
        return np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.int64)
    if mode == 27:
        return np.array([[i - 1, j - 1, k - 1] for i in range(3) for j in range(3) for k in range(3)], np.int64)
    raise ValueError("neighbor_mode: 1, 7 or 27")


def vsum(terms):
    """VSUM of the header over the rows of terms [n, ...] in the order given"""
    terms = np.asarray(terms, np.float64)
    acc = np.zeros((VW,) + terms.shape[1:])
    for r0 in range(0, terms.shape[0], VW):
        part = terms[r0:r0 + VW]
        acc[:part.shape[0]] = acc[:part.shape[0]] + part
    s = VW // 2
    while s >= 1:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0].copy()


def vsum_loop(terms):
    """the same, as a plain loop straight from the header's words"""
    terms = np.asarray(terms, np.float64)
    acc = [np.zeros(terms.shape[1:]) for _ in range(VW)]
    for r in range(terms.shape[0]):
        acc[r % VW] = acc[r % VW] + terms[r]
    s = VW // 2
    while s >= 1:
        for l in range(s):
            acc[l] = acc[l] + acc[l + s]
        s //= 2
    return np.array(acc[0], np.float64)


def coords(x, res):
    """q of every x [n, 3] -> (q [n, 3] int64, zeros where the point enters no voxel; ok [n])"""
    with np.errstate(all="ignore"):
        f = np.floor(x / np.float64(res) - 0.5)
        ok = (np.isfinite(x) & (f >= -HALF) & (f < HALF)).all(1)
    q = np.where(ok[:, None], np.where(np.isfinite(f), f, 0.0), 0.0).astype(np.int64)
    return q, ok


def rotated_cov(R, C):
    """G = (R C) R^T in the header's form, C [n, 3, 3]"""
    n = C.shape[0]
    RC = g.mul3(np.broadcast_to(R, (n, 3, 3)), C)
    return np.stack([np.stack([(RC[:, r, 0] * R[c, 0] + RC[:, r, 1] * R[c, 1]) + RC[:, r, 2] * R[c, 2] for c in range(3)], -1)
                     for r in range(3)], -2)


def build_map(members, res):
    """members: list of (cloud [n, 3] f64, cov [n, 3, 3], pose row or None) in member order -> dict of coord [v, 3] int32,
    n_points [v] int32, mean [v, 3], cov [v, 3, 3] in the map's voxel numbering, and lookup {(q0, q1, q2): voxel}"""
    xs, cs, qs = [], [], []
    for cloud, cov, pose in members:
        pose = IDENTITY if pose is None else np.asarray(pose, np.float64)
        R, t = pose[:9].reshape(3, 3), pose[9:]
        with np.errstate(all="ignore"):
            x = g.apply(R, t, cloud)
            G = rotated_cov(R, cov)
        q, ok = coords(x, res)
        xs.append(x[ok]); cs.append(G[ok]); qs.append(q[ok])
    x = np.concatenate(xs) if xs else np.zeros((0, 3))
    G = np.concatenate(cs) if cs else np.zeros((0, 3, 3))
    q = np.concatenate(qs) if qs else np.zeros((0, 3), np.int64)
    key = ((q[:, 0] + HALF) << 32) | ((q[:, 1] + HALF) << 16) | (q[:, 2] + HALF)
    order = np.argsort(key, kind="stable")                # (stable: member position, then point index)
    key = key[order]
    heads = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0] if key.size else np.zeros(0, np.int64)
    ends = np.concatenate([heads[1:], [key.size]]).astype(np.int64)
    v = heads.size
    out = dict(coord=np.zeros((v, 3), np.int32), n_points=np.zeros(v, np.int32), mean=np.zeros((v, 3)), cov=np.zeros((v, 3, 3)), lookup={})
    for k in range(v):
        run = order[heads[k]:ends[k]]
        n = np.float64(run.size)
        out["coord"][k] = q[run[0]]
        out["n_points"][k] = run.size
        out["mean"][k] = vsum(x[run]) / n
        out["cov"][k] = vsum(G[run]) / n
        out["lookup"][tuple(int(a) for a in q[run[0]])] = k
    return out


def correspondences(R, t, src, vmap, mode, res):
    """-> (vid [n, mode] int32, the voxel per offset or -1; x [n, 3])"""
    n = src.shape[0]
    vid = np.full((n, mode), -1, np.int32)
    with np.errstate(all="ignore"):
        x = g.apply(R, t, src) if n else np.zeros((0, 3))
    q, ok = coords(x, res)
    off = offsets(mode)
    look = vmap["lookup"]
    for i in np.nonzero(ok)[0]:
        for o in range(mode):
            qo = q[i] + off[o]
            if (qo >= -HALF).all() and (qo < HALF).all():
                vid[i, o] = look.get((int(qo[0]), int(qo[1]), int(qo[2])), -1)
    return vid, x


def information(R, CA, vmap, vid):
    """Mw [n, mode, 3, 3] for the correspondences (the others zero and never read)"""
    n, mode = vid.shape
    Mw = np.zeros((n, mode, 3, 3))
    if n == 0:
        return Mw
    G = rotated_cov(R, CA)
    for o in range(mode):
        ok = vid[:, o] >= 0
        if not ok.any():
            continue
        v = vid[ok, o]
        S = vmap["cov"][v] + G[ok]
        s = lambda r, c: S[:, r, c]
        a = [s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1), s(0, 2) * s(2, 1) - s(0, 1) * s(2, 2), s(0, 1) * s(1, 2) - s(0, 2) * s(1, 1),
             s(1, 2) * s(2, 0) - s(1, 0) * s(2, 2), s(0, 0) * s(2, 2) - s(0, 2) * s(2, 0), s(0, 2) * s(1, 0) - s(0, 0) * s(1, 2),
             s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0), s(0, 1) * s(2, 0) - s(0, 0) * s(2, 1), s(0, 0) * s(1, 1) - s(0, 1) * s(1, 0)]
        det = (s(0, 0) * a[0] + s(0, 1) * a[3]) + s(0, 2) * a[6]
        w = np.sqrt(vmap["n_points"][v].astype(np.float64))
        with np.errstate(all="ignore"):
            Mw[ok, o] = np.stack([w * (c / det) for c in a], -1).reshape(-1, 3, 3)
    return Mw


def _residual(x, vmap, vid, Mw, o):
    """offset o of every point: e = mean_v - x, y = Mw e, cost (rows without the correspondence are garbage)"""
    v = np.where(vid[:, o] >= 0, vid[:, o], 0)
    mean = vmap["mean"][v] if vmap["mean"].shape[0] else np.zeros((x.shape[0], 3))
    e = mean - x
    y = rr.dot3(Mw[:, o], e)
    cost = (e[:, 0] * y[:, 0] + e[:, 1] * y[:, 1]) + e[:, 2] * y[:, 2]
    return y, cost


def point_costs(R, t, src, vmap, vid, Mw):
    """per point: from +0.0, + the cost of each correspondence in offset order -> (cost [n], has [n])"""
    n, mode = vid.shape
    with np.errstate(all="ignore"):
        x = g.apply(R, t, src)
        c = np.zeros(n)
        for o in range(mode):
            ok = vid[:, o] >= 0
            _, cost = _residual(x, vmap, vid, Mw, o)
            c[ok] = c[ok] + cost[ok]
    return c, (vid >= 0).any(1)


def linearise(R, t, src, vmap, vid, Mw):
    """-> H (6x6, lower triangle filled), b [6], y0, n (correspondences)"""
    n, mode = vid.shape
    has = (vid >= 0).any(1)
    with np.errstate(all="ignore"):
        x = g.apply(R, t, src)
        z = np.zeros(n)
        A = np.stack([np.stack([z, -x[:, 2], x[:, 1]], -1), np.stack([x[:, 2], z, -x[:, 0]], -1), np.stack([-x[:, 1], x[:, 0], z], -1)], -2)
        Ht, bt, ct = np.zeros((n, 6, 6)), np.zeros((n, 6)), np.zeros(n)
        for o in range(mode):
            ok = vid[:, o] >= 0
            if not ok.any():
                continue
            M = Mw[:, o]
            y, cost = _residual(x, vmap, vid, Mw, o)
            MA = g.mul3(M, A)
            for a in range(3):
                for b in range(3):
                    if b <= a:
                        v = (A[:, 0, a] * MA[:, 0, b] + A[:, 1, a] * MA[:, 1, b]) + A[:, 2, a] * MA[:, 2, b]
                        Ht[ok, a, b] = Ht[ok, a, b] + v[ok]
                        Ht[ok, 3 + a, 3 + b] = Ht[ok, 3 + a, 3 + b] + M[ok, a, b]
                    Ht[ok, 3 + a, b] = Ht[ok, 3 + a, b] + (-MA[ok, a, b])
                v = (A[:, 0, a] * y[:, 0] + A[:, 1, a] * y[:, 1]) + A[:, 2, a] * y[:, 2]
                bt[ok, a] = bt[ok, a] + v[ok]
                bt[ok, 3 + a] = bt[ok, 3 + a] + (-y[ok, a])
            ct[ok] = ct[ok] + cost[ok]
        H = np.zeros((6, 6))
        for a in range(6):
            for b in range(a + 1):
                H[a, b] = g.ordered_sum(Ht[:, a, b], has)
        gg = np.array([g.ordered_sum(bt[:, a], has) for a in range(6)])
    return H, gg, g.ordered_sum(ct, has), int((vid >= 0).sum())


def final_pass(R, t, src, vmap, mode, res):
    """-> vid, n_corr, n_matched, fitness at the pose"""
    vid, x = correspondences(R, t, src, vmap, mode, res)
    n = src.shape[0]
    best = np.full(n, INF)
    with np.errstate(all="ignore"):
        for o in range(mode):
            ok = vid[:, o] >= 0
            if not ok.any():
                continue
            mu = vmap["mean"][np.where(ok, vid[:, o], 0)]
            dx, dy, dz = mu[:, 0] - x[:, 0], mu[:, 1] - x[:, 1], mu[:, 2] - x[:, 2]
            dd = (dx * dx + dy * dy) + dz * dz
            take = ok & (dd < best)
            best[take] = dd[take]
        has = (vid >= 0).any(1)
        nm = int(has.sum())
        fitness = g.ordered_sum(best, has) / np.float64(nm)
    return vid, int((vid >= 0).sum()), nm, fitness


def register_pair(src, CA, vmap, init=None, trace=None, **options):
    """one pair -> dict(pose [12], fitness, cost [2], n_matched, n_corr, iterations, status, voxel [n * mode] int32)"""
    o = dict(DEFAULTS)
    o.update(options)
    mode, res = o["neighbor_mode"], o["voxel_resolution"]
    R = np.eye(3) if init is None else np.asarray(init, np.float64)[:9].reshape(3, 3).copy()
    t = np.zeros(3) if init is None else np.asarray(init, np.float64)[9:].copy()
    nan = float("nan")
    out = dict(cost=np.array([nan, nan]), iterations=0)
    with np.errstate(all="ignore"):
        if src.shape[0] == 0 or vmap["coord"].shape[0] == 0:
            status = NO_POINTS
        else:
            status, lam, iters = None, 0.0, 0
            while status is None:
                vid, _ = correspondences(R, t, src, vmap, mode, res)
                Mw = information(R, CA, vmap, vid)
                H, gr, y0, n = linearise(R, t, src, vmap, vid, Mw)
                iters += 1
                if iters == 1:
                    out["cost"][0] = y0
                out["cost"][1] = y0
                if n == 0:
                    status = NO_CORRESPONDENCE
                    break
                if iters == 1:
                    m = 0.0
                    for a in range(6):
                        v = abs(H[a, a])
                        m = v if v > m else m
                    lam = o["lm_init_lambda_factor"] * m
                nu = 2.0
                ended = False
                for trial in range(o["lm_max_trials"]):
                    d, ok = g.solve_step(H, lam, gr)
                    if not ok:
                        lam = nu * lam
                        nu = 2.0 * nu
                        continue
                    q = rr.unit(np.array([1.0, 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]]))
                    dR = rr.rot_of(q)
                    Rt = g.mul3(dR, R)
                    tt = rr.dot3(dR, t) + d[3:]
                    cost, has = point_costs(Rt, tt, src, vmap, vid, Mw)
                    yi = g.ordered_sum(cost, has)
                    den = d[0] * (lam * d[0] - gr[0])
                    for a in range(1, 6):
                        den = den + d[a] * (lam * d[a] - gr[a])
                    rho = (y0 - yi) / den
                    mr = 0.0
                    for v in np.abs(dR - np.eye(3)).reshape(9):
                        mr = v if v > mr else mr
                    mt = 0.0
                    for v in np.abs(d[3:]):
                        mt = v if v > mt else mt
                    u, v = mr / o["rotation_eps"], mt / o["translation_eps"]
                    conv = bool((v if v > u else u) < 1.0)
                    if trace is not None:
                        trace.append(dict(iteration=iters, trial=trial, rho=float(rho), lam=float(lam), conv=conv, accepted=bool(rho >= 0)))
                    if not (rho >= 0):
                        if conv:
                            ended = True
                            break
                        lam = nu * lam
                        nu = 2.0 * nu
                        continue
                    R, t = Rt, tt
                    f = 2.0 * rho - 1.0
                    gg = 1.0 - (f * f) * f
                    third = 1.0 / 3.0
                    lam = lam * (gg if gg > third else third)
                    ended = True
                    break
                if not ended:
                    status = LM_FAILED
                elif conv:
                    status = CONVERGED
                elif iters >= o["max_iterations"]:
                    status = ITERATION_LIMIT
            out["iterations"] = iters
        vid, n_corr, nm, fitness = final_pass(R, t, src, vmap, mode, res)
        out.update(pose=np.concatenate([R.reshape(9), t]), status=status, n_matched=nm, n_corr=n_corr, voxel=vid.reshape(-1), fitness=fitness)
    return out


_COV_CACHE = {}


def cloud_cov(cloud32, k, plane_eps):
    """the covariances of a cloud, kept by the cloud's bytes (the tests share clouds among calls)"""
    key = (cloud32.tobytes(), cloud32.shape, k, plane_eps)
    if key not in _COV_CACHE:
        _COV_CACHE[key] = g.covariances(cloud32.astype(np.float64), k, plane_eps)[0]
    return _COV_CACHE[key]


def register(clouds, map_off, map_cloud, map_pose, src, tgt_map, init=None, **options):
    """a whole call: clouds = list of (n, 3 or 4) f32 arrays -> dict of per-pair arrays (pose, fitness, cost, n_matched,
    n_corr, iterations, status), matches (list of voxel arrays) and maps (list of build_map's dicts)"""
    o = dict(DEFAULTS)
    o.update(options)
    c32 = [np.ascontiguousarray(np.asarray(c, np.float32)[:, :3]) for c in clouds]
    wide = [c.astype(np.float64) for c in c32]
    used = sorted(set(int(v) for v in src) | set(int(map_cloud[j]) for j in range(int(map_off[-1]))))
    cov = {c: cloud_cov(c32[c], o["k_neighbors"], o["plane_eps"]) for c in used}
    maps = []
    for m in range(len(map_off) - 1):
        mem = [(wide[int(map_cloud[j])], cov[int(map_cloud[j])], None if map_pose is None else np.asarray(map_pose, np.float64).reshape(-1, 12)[j])
               for j in range(int(map_off[m]), int(map_off[m + 1]))]
        maps.append(build_map(mem, o["voxel_resolution"]))
    rows = [register_pair(wide[int(s)], cov[int(s)], maps[int(t)], None if init is None else np.asarray(init).reshape(-1, 12)[k], **options)
            for k, (s, t) in enumerate(zip(src, tgt_map))]
    n = len(rows)
    return dict(pose=np.array([r["pose"] for r in rows]).reshape(n, 12), fitness=np.array([r["fitness"] for r in rows], np.float64),
                cost=np.array([r["cost"] for r in rows]).reshape(n, 2), n_matched=np.array([r["n_matched"] for r in rows], np.int32),
                n_corr=np.array([r["n_corr"] for r in rows], np.int32), iterations=np.array([r["iterations"] for r in rows], np.int32),
                status=np.array([r["status"] for r in rows], np.int32), matches=[r["voxel"] for r in rows], maps=maps)
