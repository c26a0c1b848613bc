"""numpy restatement of sgtd_align_keypoints' rule, written from the comment in include/sgtd_accel.h and from nothing
else.  It does not call the library.  Every elementwise numpy operation on float64 arrays is one IEEE rounding, so the
assignments, the sums, the centroids, H and sgtd_overlap's figures are the header's values to the bit; the rotation
comes from another SVD (numpy.linalg.svd) and agrees with the device's to rounding only.

q_xyz [n, 3] f32 and q_label [n] u32 are the query's keypoints, f_xyz [m, 3] f32 and f_label [m] u32 the frame's
(f_xyz None: the frame has no stored keypoints); R0 [3, 3] and t0 [3] float64 the start pose."""
import numpy as np

import _overlap_ref as ov
import _refine_ref as rf

FRAGILE = 1e-6      # m^2: a decision this close to its threshold may fall the other way under a pose that differs by rounding


def assignment(R, t, q_xyz, q_label, f_xyz, f_label, radius):
    """a [n] int32 under the pose (R, t), m [n] (the minima; +inf without a keypoint of the label) and whether a
    decision is fragile: some m_i within FRAGILE of rr, or a best and a second-best r2 of one keypoint that close (copies
    of the best keypoint aside: their r2 is the best's under every pose, and the lowest index wins)"""
    rr = np.float64(radius) * np.float64(radius)
    r2, same = ov.r2_matrix(R, t, q_xyz, q_label, f_xyz, f_label)
    n, m_f = r2.shape
    a = np.full(n, -1, np.int32)
    m = np.full(n, np.inf)
    if n == 0 or m_f == 0:
        return a, m, False
    with np.errstate(invalid="ignore"):
        cand = same & ~np.isnan(r2)
        masked = np.where(cand, r2, np.inf)
        j = np.argmin(masked, axis=1)                         # (the first minimum: the lowest j)
        first = np.argmax(cand, axis=1)
        has = cand.any(axis=1)
        best = masked[np.arange(n), j]
        j = np.where(np.isinf(best), first, j)                # every r2 of the label +inf: the lowest j of the label
        m = np.where(has, best, np.inf)
        ok = has & (m <= rr)
        a[ok] = j[ok]
        fragile = bool((np.abs(m[has & np.isfinite(m)] - rr) < FRAGILE).any())
        if m_f >= 2:
            w = np.asarray(f_xyz, np.float32).reshape(-1, 3).view(np.uint32)
            twin = (w[None, :, :] == w[j][:, None, :]).all(axis=2)    # the same position bit for bit: the same r2 under any pose
            second = np.where(twin, np.inf, masked).min(axis=1)
            gap = second - m
            fragile = fragile or bool((gap[has & np.isfinite(second)] < FRAGILE).any())
    return a, m, fragile


def fit(q_xyz, f_xyz, a):
    """cp, cw, H of the assigned pairs, in the header's summation order"""
    p = np.asarray(q_xyz, np.float32).astype(np.float64).reshape(-1, 3)
    w = np.asarray(f_xyz, np.float32).astype(np.float64).reshape(-1, 3)
    take = a >= 0
    c = np.float64(np.count_nonzero(take))
    wa = w[np.where(take, a, 0)]
    with np.errstate(invalid="ignore"):
        cp = np.array([ov.ordered_sum(p[:, r], take) / c for r in range(3)])
        cw = np.array([ov.ordered_sum(wa[:, r], take) / c for r in range(3)])
        dp, dw = p - cp, wa - cw
        H = np.array([[ov.ordered_sum(dp[:, r] * dw[:, s], take) for s in range(3)] for r in range(3)])
    return cp, cw, H


def evaluate(R, t, q_xyz, q_label, f_xyz, f_label, radius):
    """sgtd_overlap's figures and the assignment under one pose -> (dict of ov.KEYS, a)"""
    e = ov.overlap(R, t, q_xyz, q_label, f_xyz, f_label, radius)
    a, _, _ = assignment(R, t, q_xyz, q_label, f_xyz, f_label, radius)
    return e, a


def align(R0, t0, q_xyz, q_label, f_xyz, f_label, radius, iterations):
    """the whole rule for one verified candidate -> dict(rot, t, n_fits, n_corr, stop, moments [15], before, after (dicts
    of ov.KEYS), assign, fragile, collinear)"""
    R, t = np.asarray(R0, np.float64).reshape(3, 3), np.asarray(t0, np.float64).reshape(3)
    nq = int(np.asarray(q_label).reshape(-1).size)
    nan15 = np.full(15, np.nan)
    if f_xyz is None:
        e = ov.overlap(R, t, q_xyz, q_label, None, None, radius)
        return dict(rot=R, t=t, n_fits=0, n_corr=0, stop=1, moments=nan15, before=e, after=e, assign=np.full(nq, -1, np.int32),
                    fragile=False, collinear=False)
    before = ov.overlap(R, t, q_xyz, q_label, f_xyz, f_label, radius)
    prev, stop, n_fits, n_corr, mom = None, 0, 0, 0, nan15
    fragile = collinear = False
    for it in range(1, iterations + 1):
        a, _, fr = assignment(R, t, q_xyz, q_label, f_xyz, f_label, radius)
        fragile = fragile or fr
        na = int(np.count_nonzero(a >= 0))
        if na < 3:
            stop = 1
            break
        if it >= 2 and np.array_equal(a, prev):
            stop = 2
            break
        cp, cw, H = fit(q_xyz, f_xyz, a)
        R = rf.kabsch(H)
        t = rf.translation(R, cp, cw)
        collinear = collinear or rf.collinear(H)
        n_fits, n_corr, mom, prev = n_fits + 1, na, np.concatenate([cp, cw, H.reshape(9)]), a
    after = ov.overlap(R, t, q_xyz, q_label, f_xyz, f_label, radius)
    a, _, fr = assignment(R, t, q_xyz, q_label, f_xyz, f_label, radius)
    return dict(rot=R, t=t, n_fits=n_fits, n_corr=n_corr, stop=stop, moments=mom, before=before, after=after, assign=a,
                fragile=fragile or fr, collinear=collinear)


NO_RESULT = dict(rot=np.zeros((3, 3)), t=np.zeros(3), n_fits=0, n_corr=0, stop=-1, moments=np.full(15, np.nan), before=ov.NO_RESULT,
                 after=ov.NO_RESULT)


def search_loop_aligned(score, overlap_after, rms_after, stop, n_cand, cand_frame, min_overlap, max_rms):
    """sgtd_search_loop_aligned's rule for one query -> (best_cand, best_frame, best_rms, best_overlap)"""
    bc = -1
    for c in range(int(n_cand)):
        if stop[c] < 0 or np.isnan(rms_after[c]):
            continue
        if min_overlap > 0 and not (overlap_after[c] >= min_overlap):
            continue
        if max_rms > 0 and not np.isinf(max_rms) and not (rms_after[c] <= max_rms):
            continue
        if bc < 0 or rms_after[c] < rms_after[bc] or (rms_after[c] == rms_after[bc] and score[c] > score[bc]):
            bc = c
    if bc < 0:
        return -1, -1, float("nan"), float("nan")
    return bc, int(cand_frame[bc]), float(rms_after[bc]), float(overlap_after[bc])
