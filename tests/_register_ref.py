"""numpy restatement of sgtd_register_clouds' rule, written from the comment in include/sgtd_accel.h and from nothing
else.  It does not call the library.  Every elementwise numpy operation on float64 arrays (+, -, *, /, sqrt) and every
Python float operation is one IEEE rounding, the sums are taken in the header's order, so every number here is the
device's to the bit.  UNIT, ROT, M v, the Cholesky and its substitutions are _relax_ref's; svd3 is written out below from
the one-sided Jacobi SVD the header names (sgtd_verify's), operation by operation.

Clouds are (n, 3) float64 arrays of exactly widened f32 values; poses are rows of 12 (rot row-major, t)."""
import math

import numpy as np

import _relax_ref as rr

W = 256
CONVERGED, ITERATION_LIMIT, LM_FAILED, NO_CORRESPONDENCE, NO_POINTS = 0, 1, 2, 3, 4
DEFAULTS = dict(k_neighbors=20, max_iterations=64, lm_max_trials=10, reserved=0, max_corr_dist=float("inf"),
                lm_init_lambda_factor=1e-9, rotation_eps=2e-3, translation_eps=5e-4, plane_eps=1e-3)
INF = float("inf")


def ordered_sum(terms, in_set):
    """SUM of the header: terms [n, ...] -> [...]; point i into accumulator i mod W, unmatched points skipped"""
    terms = np.asarray(terms, np.float64)
    in_set = np.asarray(in_set, bool)
    n = terms.shape[0]
    rows = -(-n // W) if n else 0
    pad = rows * W - n
    if pad:
        terms = np.concatenate([terms, np.zeros((pad,) + terms.shape[1:])])
        in_set = np.concatenate([in_set, np.zeros(pad, bool)])
    acc = np.zeros((W,) + terms.shape[1:])
    for r in range(rows):
        m = in_set[r * W:(r + 1) * W]
        if m.any():
            acc[m] = acc[m] + terms[r * W:(r + 1) * W][m]
    s = W // 2
    while s >= 1:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0].copy()


def ordered_sum_loop(terms, in_set):
    """the same, as a plain loop straight from the header's words"""
    terms = np.asarray(terms, np.float64)
    acc = [np.zeros(terms.shape[1:]) for _ in range(W)]
    for i in range(terms.shape[0]):
        if in_set[i]:
            acc[i % W] = acc[i % W] + terms[i]
    s = W // 2
    while s >= 1:
        for l in range(s):
            acc[l] = acc[l] + acc[l + s]
        s //= 2
    return np.array(acc[0], np.float64)


def mul3(a, b):
    """[., 3, 3] x [., 3, 3]: (a0*b0 + a1*b1) + a2*b2"""
    return np.stack([np.stack([(a[..., r, 0] * b[..., 0, c] + a[..., r, 1] * b[..., 1, c]) + a[..., r, 2] * b[..., 2, c]
                               for c in range(3)], -1) for r in range(3)], -2)


def svd3(H):
    """the one-sided (Hestenes) Jacobi SVD of a 3x3 in Python floats: -> U, V (lists of rows), singular values descending"""
    A = [[float(H[i][j]) for j in range(3)] for i in range(3)]
    Wm = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    U = [[0.0] * 3 for _ in range(3)]
    V = [[0.0] * 3 for _ in range(3)]
    for _ in range(60):
        off = 0.0
        for p in range(2):
            for q in range(p + 1, 3):
                alpha = beta = gamma = 0.0
                for k in range(3):
                    alpha = alpha + A[k][p] * A[k][p]
                    beta = beta + A[k][q] * A[k][q]
                    gamma = gamma + A[k][p] * A[k][q]
                rel = abs(gamma) / math.sqrt(alpha * beta + 1e-300)
                off = rel if off < rel else off
                if abs(gamma) < 1e-300:
                    continue
                zeta = (beta - alpha) / (2.0 * gamma)
                t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = c * t
                for k in range(3):
                    ap, aq = A[k][p], A[k][q]
                    A[k][p] = c * ap - s * aq
                    A[k][q] = s * ap + c * aq
                    wp, wq = Wm[k][p], Wm[k][q]
                    Wm[k][p] = c * wp - s * wq
                    Wm[k][q] = s * wp + c * wq
        if off < 1e-15:
            break
    sv = [math.sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]) for j in range(3)]
    order = [0, 1, 2]
    for i in range(1, 3):                      # the insertion sort of three, by descending value
        val = order[i]
        if sv[val] > sv[order[0]]:
            for j in range(i, 0, -1):
                order[j] = order[j - 1]
            order[0] = val
        else:
            j = i
            while sv[val] > sv[order[j - 1]]:
                order[j] = order[j - 1]
                j -= 1
            order[j] = val
    smax = sv[order[0]]
    rank = 0
    for jj in range(3):
        j = order[jj]
        for k in range(3):
            V[k][jj] = Wm[k][j]
        if sv[j] > 1e-12 * (smax if smax > 0 else 1.0):
            for k in range(3):
                U[k][jj] = A[k][j] / sv[j]
            rank = jj + 1
    if rank == 2:
        U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1]
        U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1]
        U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1]
    elif rank < 2:
        for i in range(3):
            for j in range(rank, 3):
                U[i][j] = 1.0 if i == j else 0.0
    return U, V


def d2_rows(x, w):
    """d2 of every x [n, 3] to every w [m, 3] -> [n, m]"""
    with np.errstate(all="ignore"):
        dx = w[None, :, 0] - x[:, None, 0]
        dy = w[None, :, 1] - x[:, None, 1]
        dz = w[None, :, 2] - x[:, None, 2]
        return (dx * dx + dy * dy) + dz * dz


def neighbours(cloud, k):
    """-> [n, k'] int64: per point its neighbours in (d2, index) order, -1 where fewer have a d2 below +inf"""
    n = cloud.shape[0]
    kk = min(k, n)
    out = np.full((n, kk), -1, np.int64)
    for first in range(0, n, 256):
        d = d2_rows(cloud[first:first + 256], cloud)
        d = np.where(d < INF, d, INF)                         # NaN and +inf are never chosen
        order = np.argsort(d, axis=1, kind="stable")[:, :kk]  # (stable: equal d2 in ascending index)
        ok = np.take_along_axis(d, order, 1) < INF
        out[first:first + 256] = np.where(ok, order, -1)
    return out


def covariances(cloud, k, plane_eps):
    """-> (C [n, 3, 3], neighbours [n, k'])"""
    n = cloud.shape[0]
    nb = neighbours(cloud, k)
    kk = nb.shape[1] if n else 0
    div = np.float64(kk)
    mu = np.zeros((n, 3))
    for s in range(kk):
        ok = nb[:, s] >= 0
        mu[ok] = mu[ok] + cloud[nb[ok, s]]
    mu = mu / div
    c = np.zeros((n, 3, 3))
    for s in range(kk):
        ok = nb[:, s] >= 0
        q = cloud[nb[ok, s]] - mu[ok]
        c[ok] = c[ok] + q[:, :, None] * q[:, None, :]
    c = c / div
    U = np.zeros((n, 3, 3))
    V = np.zeros((n, 3, 3))
    for i in range(n):
        u, v = svd3(c[i])
        for b in range(3):
            if (u[0][b] * v[0][b] + u[1][b] * v[1][b]) + u[2][b] * v[2][b] < 0.0:
                for a in range(3):
                    u[a][b] = -u[a][b]
        U[i], V[i] = u, v
    D = np.zeros((n, 3, 3))
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = plane_eps
    C = mul3(mul3(U, D), np.swapaxes(V, 1, 2))
    return C, nb


def apply(R, t, p):
    return np.stack([((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + t[r] for r in range(3)], -1)


def correspondences(R, t, src, tgt, max2):
    """-> (j [n] int64, -1 where the match is not kept; dd [n]: the smallest d2 found, +inf without one)"""
    n = src.shape[0]
    j = np.full(n, -1, np.int64)
    dd = np.full(n, INF)
    if n == 0 or tgt.shape[0] == 0:
        return j, dd
    x = apply(R, t, src)
    for first in range(0, n, 256):
        d = d2_rows(x[first:first + 256], tgt)
        d = np.where(d < INF, d, INF)
        a = np.argmin(d, axis=1)                              # (the first of equal minima: the lowest index)
        m = np.take_along_axis(d, a[:, None], 1)[:, 0]
        dd[first:first + 256] = m
        j[first:first + 256] = np.where(m < max2, a, -1)
    return j, dd


def information(R, CA, CB, j):
    """M_i for the kept matches (rows of the others are zero and never read)"""
    n = CA.shape[0]
    M = np.zeros((n, 3, 3))
    ok = j >= 0
    if not ok.any():
        return M
    Rn = np.broadcast_to(R, (int(ok.sum()), 3, 3))
    RC = mul3(Rn, CA[ok])
    G = np.stack([np.stack([(RC[:, r, 0] * R[c, 0] + RC[:, r, 1] * R[c, 1]) + RC[:, r, 2] * R[c, 2] for c in range(3)], -1)
                  for r in range(3)], -2)
    S = CB[j[ok]] + G
    s = lambda r, c: S[:, r, c]
    a = [s(1, 1) * s(2, 2) - s(1, 2) * s(2, 1), s(0, 2) * s(2, 1) - s(0, 1) * s(2, 2), s(0, 1) * s(1, 2) - s(0, 2) * s(1, 1),
         s(1, 2) * s(2, 0) - s(1, 0) * s(2, 2), s(0, 0) * s(2, 2) - s(0, 2) * s(2, 0), s(0, 2) * s(1, 0) - s(0, 0) * s(1, 2),
         s(1, 0) * s(2, 1) - s(1, 1) * s(2, 0), s(0, 1) * s(2, 0) - s(0, 0) * s(2, 1), s(0, 0) * s(1, 1) - s(0, 1) * s(1, 0)]
    det = (s(0, 0) * a[0] + s(0, 1) * a[3]) + s(0, 2) * a[6]
    with np.errstate(all="ignore"):
        M[ok] = np.stack([v / det for v in a], -1).reshape(-1, 3, 3)
    return M


def residuals(R, t, src, tgt, j, M):
    """-> x, y = M e, cost per point (rows of unmatched points are garbage and never summed)"""
    jj = np.where(j >= 0, j, 0)
    x = apply(R, t, src)
    e = tgt[jj] - x
    y = rr.dot3(M, e)
    cost = (e[:, 0] * y[:, 0] + e[:, 1] * y[:, 1]) + e[:, 2] * y[:, 2]
    return x, y, cost


def linearise(R, t, src, tgt, j, M):
    """-> H (6x6, lower triangle filled), b [6], y0, n"""
    ok = j >= 0
    n = src.shape[0]
    x, y, cost = residuals(R, t, src, tgt, j, M)
    z = np.zeros(n)
    A = np.stack([np.stack([z, -x[:, 2], x[:, 1]], -1), np.stack([x[:, 2], z, -x[:, 0]], -1), np.stack([-x[:, 1], x[:, 0], z], -1)], -2)
    MA = mul3(M, A)
    H = np.zeros((6, 6))
    for a in range(3):
        for b in range(3):
            if b <= a:
                H[a, b] = ordered_sum((A[:, 0, a] * MA[:, 0, b] + A[:, 1, a] * MA[:, 1, b]) + A[:, 2, a] * MA[:, 2, b], ok)
                H[3 + a, 3 + b] = ordered_sum(M[:, a, b], ok)
            H[3 + a, b] = ordered_sum(-MA[:, a, b], ok)
    g = np.zeros(6)
    for a in range(3):
        g[a] = ordered_sum((A[:, 0, a] * y[:, 0] + A[:, 1, a] * y[:, 1]) + A[:, 2, a] * y[:, 2], ok)
        g[3 + a] = ordered_sum(-y[:, a], ok)
    return H, g, ordered_sum(cost, ok), int(ok.sum())


def solve_step(H, lam, g):
    """(H + lambda I) d = -b -> (d, ok)"""
    Mx = np.tril(H).copy()
    for c in range(6):
        Mx[c, c] = H[c, c] + lam
    L, ok = rr.cholesky(Mx[None])
    if not ok[0]:
        return None, False
    return rr.solve(L, ok, (-g)[None])[0], True


def register_pair(src, tgt, CA, CB, init=None, trace=None, **options):
    """one pair -> dict(pose [12], fitness, cost [2], n_matched, iterations, status, match_j [n] int32, match_d2 [n])"""
    o = dict(DEFAULTS)
    o.update(options)
    R = np.eye(3) if init is None else np.asarray(init, np.float64)[:9].reshape(3, 3).copy()
    t = np.zeros(3) if init is None else np.asarray(init, np.float64)[9:].copy()
    max2 = np.float64(o["max_corr_dist"]) * np.float64(o["max_corr_dist"])
    nan = float("nan")
    out = dict(cost=np.array([nan, nan]), iterations=0)
    with np.errstate(all="ignore"):
        if src.shape[0] == 0 or tgt.shape[0] == 0:
            status = NO_POINTS
        else:
            status, lam, iters = None, 0.0, 0
            while status is None:
                j, _ = correspondences(R, t, src, tgt, max2)
                M = information(R, CA, CB, j)
                H, g, y0, n = linearise(R, t, src, tgt, j, M)
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
                    d, ok = solve_step(H, lam, g)
                    if not ok:
                        lam = nu * lam
                        nu = 2.0 * nu
                        continue
                    q = rr.unit(np.array([1.0, 0.5 * d[0], 0.5 * d[1], 0.5 * d[2]]))
                    dR = rr.rot_of(q)
                    Rt = mul3(dR, R)
                    tt = rr.dot3(dR, t) + d[3:]
                    _, _, cost = residuals(Rt, tt, src, tgt, j, M)
                    yi = ordered_sum(cost, j >= 0)
                    den = d[0] * (lam * d[0] - g[0])
                    for a in range(1, 6):
                        den = den + d[a] * (lam * d[a] - g[a])
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
        j, dd = correspondences(R, t, src, tgt, max2)
        ok = j >= 0
        n = int(ok.sum())
        out.update(pose=np.concatenate([R.reshape(9), t]), status=status, n_matched=n, match_j=j.astype(np.int32), match_d2=dd,
                   fitness=ordered_sum(dd, ok) / np.float64(n))
    return out


def register(clouds, src, tgt, init=None, **options):
    """a whole call: clouds = list of (n, 3 or 4) f32 arrays -> dict of per-pair arrays (pose, fitness, cost, n_matched,
    iterations, status), matches (list of (j, d2)) and cov {cloud: [n, 3, 3]} of the named clouds"""
    o = dict(DEFAULTS)
    o.update(options)
    wide = [np.asarray(c, np.float32)[:, :3].astype(np.float64) for c in clouds]
    cov = {}
    for c in sorted(set(int(v) for v in src) | set(int(v) for v in tgt)):
        cov[c] = covariances(wide[c], o["k_neighbors"], o["plane_eps"])[0]
    rows = [register_pair(wide[s], wide[t], cov[s], cov[t], None if init is None else init[k], **options)
            for k, (s, t) in enumerate(zip(src, tgt))]
    n = len(rows)
    return dict(pose=np.array([r["pose"] for r in rows]).reshape(n, 12), fitness=np.array([r["fitness"] for r in rows], np.float64),
                cost=np.array([r["cost"] for r in rows]).reshape(n, 2), n_matched=np.array([r["n_matched"] for r in rows], np.int32),
                iterations=np.array([r["iterations"] for r in rows], np.int32), status=np.array([r["status"] for r in rows], np.int32),
                matches=[(r["match_j"], r["match_d2"]) for r in rows], cov=cov)


# ---- scenes

def rot_axis(axis, angle):
    """the rotation by `angle` about `axis` (Rodrigues; test scenes only: not part of the rule)"""
    return rr.rot_vec(np.asarray(axis, np.float64) / np.linalg.norm(axis) * angle)


def planted_scene(n, seed):
    """the ground z = 0 over 20 m x 20 m (n / 2 points), a wall y = 6 (n / 4), a wall x = -8 (the rest), 0.02 m Gaussian
    noise along each surface's normal; the target is n + 100 independently drawn points, the source the scene's n points
    seen from a frame moved by 3 degrees about (0.2, -0.1, 1) and by (0.4, -0.3, 0.1) m, rounded to f32.
    -> (source f32 [n, 3], target f32 [n + 100, 3], R_true, t_true) with target ~ R_true source + t_true"""
    rng = np.random.default_rng(seed)

    def draw(m):
        a, b = m // 2, m // 4
        c = m - a - b
        g = np.stack([rng.uniform(-10, 10, a), rng.uniform(-10, 10, a), rng.normal(0.0, 0.02, a)], 1)
        w1 = np.stack([rng.uniform(-10, 10, b), 6.0 + rng.normal(0.0, 0.02, b), rng.uniform(0, 4, b)], 1)
        w2 = np.stack([-8.0 + rng.normal(0.0, 0.02, c), rng.uniform(-10, 10, c), rng.uniform(0, 4, c)], 1)
        return np.concatenate([g, w1, w2])

    scene, target = draw(n), draw(n + 100)
    Rm = rot_axis([0.2, -0.1, 1.0], np.deg2rad(3.0))
    tm = np.array([0.4, -0.3, 0.1])
    source = (scene - tm) @ Rm                      # p = Rm^T (x - tm): x = Rm p + tm
    return source.astype(np.float32), target.astype(np.float32), Rm, tm


def near_start(R_true, t_true):
    """a start 0.13 m / 0.9 degrees off the truth, as a pose row"""
    R0 = rot_axis([1.0, 0.5, -0.3], np.deg2rad(0.9)) @ R_true
    t0 = t_true + np.array([0.1, -0.07, 0.045])
    return np.concatenate([R0.reshape(9), t0])


def overshoot_case(seed=7):
    """a pair whose solve needs rejected trials: the planted scene of 300 points moved (200, 100, 0) m from the origin,
    started 10 degrees off about z: so far out, a rotation step's second-order term outgrows the residual.
    -> (source, target, init row); options k_neighbors=10, max_iterations=30, max_corr_dist +inf.  Measured on the
    restatement: iterations 5 and 7 reject two trials each; with lm_max_trials=1 the solve ends "LM failed" in iteration 5"""
    s, t, _, _ = planted_scene(300, seed)
    shift = [200.0, 100.0, 0.0]
    init = np.concatenate([rot_axis([0.0, 0.0, 1.0], np.deg2rad(10.0)).reshape(9), np.zeros(3)])
    return (s.astype(np.float64) + shift).astype(np.float32), (t.astype(np.float64) + shift).astype(np.float32), init


def pose_error(pose, R_true, t_true):
    """-> (translation error in m, rotation error in degrees)"""
    R, t = np.asarray(pose)[:9].reshape(3, 3), np.asarray(pose)[9:]
    c = (np.trace(R.T @ R_true) - 1.0) / 2.0
    return float(np.linalg.norm(t - t_true)), float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def same(a, b):
    """bit for bit, NaNs of any payload equal"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes())
