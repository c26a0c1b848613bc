"""numpy restatement of sgtd_overlap's rule, written from the comment in include/sgtd_accel.h and from nothing else.
It does not call the library.  Every elementwise numpy operation on float64 arrays is one IEEE rounding, so with the
stated association every value is the header's to the bit.

q_xyz [n, 3] f32 and q_label [n] u32 are the query's keypoints, f_xyz [m, 3] f32 and f_label [m] u32 the frame's
(f_xyz None: the frame has no stored keypoints); R [3, 3] and t [3] float64 the candidate's relative pose."""
import numpy as np

W = 256          # accumulators


def ordered_sum(values, take):
    """SUM of the header over the keypoints i with take[i]: accumulator l <- i == l (mod 256) in ascending i, then the
    tree acc[l] += acc[l + s], s = 128 ... 1"""
    values = np.asarray(values, np.float64)
    take = np.asarray(take, bool)
    n = values.shape[0]
    rows = -(-n // W) if n else 0
    pad = rows * W - n
    if pad:
        values = np.concatenate([values, np.zeros(pad)])
        take = np.concatenate([take, np.zeros(pad, bool)])
    acc = np.zeros(W)                                   # +0.0
    for r in range(rows):
        m = take[r * W:(r + 1) * W]
        acc[m] = acc[m] + values[r * W:(r + 1) * W][m]
    s = W // 2
    while s >= 1:
        acc[:s] = acc[:s] + acc[s:2 * s]
        s //= 2
    return np.float64(acc[0])


def ordered_sum_loop(values, take):
    """the same, as a plain loop straight from the header's words (slow: for the test of ordered_sum)"""
    acc = [np.float64(0.0) for _ in range(W)]
    for i in range(len(values)):
        if take[i]:
            acc[i % W] = acc[i % W] + np.float64(values[i])
    for s in (128, 64, 32, 16, 8, 4, 2, 1):
        for l in range(s):
            acc[l] = acc[l] + acc[l + s]
    return np.float64(acc[0])


def transform(R, t, q_xyz):
    """x [n, 3] of the query keypoints under (R, t)"""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    p = np.asarray(q_xyz, np.float32).astype(np.float64).reshape(-1, 3)
    return np.stack([((R[c, 0] * p[:, 0] + R[c, 1] * p[:, 1]) + R[c, 2] * p[:, 2]) + t[c] for c in range(3)], axis=1)


def r2_matrix(R, t, q_xyz, q_label, f_xyz, f_label):
    """r2(i, j) [n, m] and the label gate same[i, j]"""
    x = transform(R, t, q_xyz)
    w = np.asarray(f_xyz, np.float32).astype(np.float64).reshape(-1, 3)
    e = x[:, None, :] - w[None, :, :]
    r2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    same = np.asarray(q_label, np.uint32).reshape(-1)[:, None] == np.asarray(f_label, np.uint32).reshape(-1)[None, :]
    return r2, same


def minima(R, t, q_xyz, q_label, f_xyz, f_label):
    """m_i [n]: +inf without a keypoint of the label; a NaN r2 never is the minimum"""
    r2, same = r2_matrix(R, t, q_xyz, q_label, f_xyz, f_label)
    with np.errstate(invalid="ignore"):
        return np.fmin.reduce(np.where(same, r2, np.inf), axis=1, initial=np.inf)


def overlap(R, t, q_xyz, q_label, f_xyz, f_label, radius):
    """the whole rule for one verified candidate -> dict(n_query_kp, n_frame_kp, n_hit_query, n_hit_frame, overlap, rms,
    m, hit_query, hit_frame)"""
    nq = int(np.asarray(q_label).reshape(-1).size)
    nan = np.float64("nan")
    if f_xyz is None:
        return dict(n_query_kp=nq, n_frame_kp=-1, n_hit_query=0, n_hit_frame=0, overlap=nan, rms=nan, m=None,
                    hit_query=None, hit_frame=None)
    rr = np.float64(radius) * np.float64(radius)
    r2, same = r2_matrix(R, t, q_xyz, q_label, f_xyz, f_label)
    with np.errstate(invalid="ignore"):
        m = np.fmin.reduce(np.where(same, r2, np.inf), axis=1, initial=np.inf)
        hit_q = m <= rr
        hit_f = (same & (r2 <= rr)).any(axis=0)
    nhq, nhf = int(np.count_nonzero(hit_q)), int(np.count_nonzero(hit_f))
    ov = np.float64(nhq) / np.float64(nq) if nq else nan
    rms = np.sqrt(ordered_sum(m, hit_q) / np.float64(nhq)) if nhq else nan
    return dict(n_query_kp=nq, n_frame_kp=int(same.shape[1]), n_hit_query=nhq, n_hit_frame=nhf, overlap=ov, rms=rms, m=m,
                hit_query=hit_q, hit_frame=hit_f)


NO_RESULT = dict(n_query_kp=-1, n_frame_kp=-1, n_hit_query=-1, n_hit_frame=-1, overlap=np.float64("nan"), rms=np.float64("nan"))
KEYS = ("n_query_kp", "n_frame_kp", "n_hit_query", "n_hit_frame", "overlap", "rms")


def same_value(a, b):
    """equal as numbers of the rule: integers equal, doubles the same bits or both NaN"""
    if isinstance(a, (int, np.integer)):
        return int(a) == int(b)
    a, b = np.float64(a), np.float64(b)
    return bool((np.isnan(a) and np.isnan(b)) or a.view(np.uint64) == b.view(np.uint64))


def search_loop_overlap(score, overlap_v, n_cand, cand_frame, icp_threshold, min_overlap):
    """sgtd_search_loop_overlap's rule for one query -> (best_cand, best_frame, best_score, best_overlap)"""
    bs, bc = 0.0, -1
    for c in range(int(n_cand)):
        if min_overlap > 0 and not (overlap_v[c] >= min_overlap):
            continue
        if score[c] > bs:
            bs, bc = float(score[c]), c
    if bc >= 0 and bs > icp_threshold:
        return bc, int(cand_frame[bc]), bs, float(overlap_v[bc])
    return -1, -1, 0.0, float("nan")
