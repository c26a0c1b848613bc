"""numpy restatement of sgtd_refine_poses' rule, written from the comment in include/sgtd_accel.h and from nothing
else: the fixed summation order, the centroids, H, the Kabsch solve through numpy.linalg.svd, the residuals and the
re-selection.  It does not call the library.  Every elementwise numpy operation on float64 arrays is one IEEE rounding,
so the sums, centroids, H and the residuals are the header's values to the bit; the rotation comes from another SVD
and agrees with the device's to rounding only.

Shapes: p, w are [n_list, 3, 3] float64 — pair j, correspondence A / B / C, xyz (f32 vertex values widened exactly);
in_set is a bool [n_list]."""
import numpy as np

W = 256          # accumulators
THR2 = 9.0       # r2 < 9.0  <=>  sqrt(r2) < 3.0
MIN_PAIRS = 4


def ordered_sum(terms, in_set):
    """SUM of the header: terms [n_list, 3, ...] (pair, correspondence, components) -> [...]"""
    terms = np.asarray(terms, np.float64)
    in_set = np.asarray(in_set, bool)
    n = terms.shape[0]
    rows = -(-n // W) if n else 0
    pad = rows * W - n
    if pad:
        terms = np.concatenate([terms, np.zeros((pad,) + terms.shape[1:])])
        in_set = np.concatenate([in_set, np.zeros(pad, bool)])
    acc = np.zeros((W,) + terms.shape[2:])          # +0.0
    for r in range(rows):
        m = in_set[r * W:(r + 1) * W]               # accumulator l <- list position r * 256 + l
        if not m.any():
            continue
        for a in range(3):                          # A, B, C
            acc[m] = acc[m] + terms[r * W:(r + 1) * W, a][m]
    s = W // 2
    while s >= 1:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return acc[0].copy()


def ordered_sum_loop(terms, in_set):
    """the same, as a plain loop straight from the header's words (slow: for the test of ordered_sum)"""
    terms = np.asarray(terms, np.float64)
    shape = terms.shape[2:]
    acc = [np.zeros(shape) for _ in range(W)]
    for j in range(terms.shape[0]):
        if not in_set[j]:
            continue
        l = j % W
        for a in range(3):
            acc[l] = acc[l] + terms[j, a]
    for s in (128, 64, 32, 16, 8, 4, 2, 1):
        for l in range(s):
            acc[l] = acc[l] + acc[l + s]
    return np.array(acc[0], np.float64)


def moments(p, w, in_set):
    """-> n, cp, cw, H"""
    n = int(np.count_nonzero(in_set))
    d = np.float64(3 * n)
    cp = ordered_sum(p, in_set) / d
    cw = ordered_sum(w, in_set) / d
    dp, dw = p - cp, w - cw
    H = ordered_sum(dp[:, :, :, None] * dw[:, :, None, :], in_set)
    return n, cp, cw, H


def kabsch(H):
    """R = V U^T of H = U S V^T, with the diag(1, 1, -1) correction for a reflection"""
    U, _, Vt = np.linalg.svd(H)
    V = Vt.T
    R = V @ U.T
    if np.linalg.det(R) < 0:
        R = V @ np.diag([1.0, 1.0, -1.0]) @ U.T
    return R


def translation(R, cp, cw):
    return -((R[:, 0] * cp[0] + R[:, 1] * cp[1]) + R[:, 2] * cp[2]) + cw


def r2(R, t, p, w):
    """squared residual of every correspondence: [n_list, 3]"""
    e = [(((R[i, 0] * p[..., 0] + R[i, 1] * p[..., 1]) + R[i, 2] * p[..., 2]) + t[i]) - w[..., i] for i in range(3)]
    return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def rmse(R, t, p, w, in_set):
    n = int(np.count_nonzero(in_set))
    return np.sqrt(ordered_sum(r2(R, t, p, w), in_set) / np.float64(3 * n))


def reselect(R, t, p, w):
    return np.all(r2(R, t, p, w) < THR2, axis=1)


def collinear(H, rel=1e-6):
    """the rotation is ill-posed: H's second singular value is below `rel` of its first"""
    s = np.linalg.svd(H, compute_uv=False)
    return bool(s[1] < rel * s[0])


def refine(p, w, set0, iterations, verify_R, verify_t):
    """the whole rule -> dict(rot, t, n_pairs, cp, cw, H, moments[15], rmse, rmse_verify, set, fits, stop) where fits =
    fits made and stop = None, "few" (the next set had fewer than 4 pairs) or "same" (it equalled the current one)"""
    cur = np.asarray(set0, bool).copy()
    stop, fits = None, 0
    it = 1
    while True:
        n, cp, cw, H = moments(p, w, cur)
        R = kabsch(H)
        t = translation(R, cp, cw)
        fits += 1
        if it >= iterations:
            break
        nxt = reselect(R, t, p, w)
        if np.count_nonzero(nxt) < MIN_PAIRS:
            stop = "few"
            break
        if np.array_equal(nxt, cur):
            stop = "same"
            break
        cur = nxt
        it += 1
    return dict(rot=R, t=t, n_pairs=n, cp=cp, cw=cw, H=H, moments=np.concatenate([cp, cw, H.reshape(9)]),
                rmse=rmse(R, t, p, w, cur), rmse_verify=rmse(np.asarray(verify_R), np.asarray(verify_t), p, w, cur),
                set=cur, fits=fits, stop=stop)


def correspondences(q_vertex, q_idx, e_vertex):
    """p, w [n_list, 3, 3] float64 of one candidate's match list: q_vertex [n_desc, 9] f32 (sgtd_result_query_descs),
    q_idx [n_list], e_vertex [n_list, 9] f32 (sgtd_fetch_entries of the list's db_entry)"""
    p = np.asarray(q_vertex, np.float32).reshape(-1, 9)[np.asarray(q_idx, np.int64)].astype(np.float64).reshape(-1, 3, 3)
    w = np.asarray(e_vertex, np.float32).reshape(-1, 9).astype(np.float64).reshape(-1, 3, 3)
    return p, w
