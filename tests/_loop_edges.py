"""Workloads at the edge of sgtd_loop_frames' bound — the sweep's BOUND compare `(id >> id_bits) < qfv[k]` of
probe_kernels.hip.h, whose limit loop_bound_kernel (table_kernels.hip.h) sets to max(c + q - skip_near, frame_lo) and
sweep_plan turns into a local frame (0xFFFFFFFF, everything counts, at or past the table's span) — and a restatement of
the loop with a pluggable bound.  Plain helper module of tests/test_loop_edges.py (CPU: the restatement with the plain
bound equals the oracle driven through the reference's loop build -> select -> add on every workload; every mutant of the
bound changes the expected result on a named workload) and tests/test_gpu_loop_edges.py (GPU: every form of a loop batch
equals the oracle on them, bit for bit).

A workload (Session) is a short run of synthetic frames 25 m apart (sgtd_amd.synth, fixed streams: unrelated frames share
next to no descriptor), optionally after a prebuilt map of the same trajectory.  Some frames are exact copies ("twins")
of an earlier frame at a known distance d: a twin's descriptors all match, so the frame just inside or just outside the
bound moves hundreds of votes and a candidate.  Frames with fewer keypoints than descriptor_near_num have no descriptors.

The mutants of the bound (test_loop_edges.py asserts each on the workload and skip_near named here):
  le            `<=` for `<`                                        bound, skip_near 1   (the twin at distance 1 shows)
  skip_minus    skip_near - 1                                       bound, skip_near 8   (the twin at distance 8 shows)
  skip_plus     skip_near + 1                                       bound, skip_near 7   (the twin at distance 8 is lost)
  no_clamp      c + q - skip_near wraps below zero                  bound, skip_near 9   (frame 4 sees its later twin 12)
  clamp_zero    the clamp at 0, not frame_lo: the local limit wraps removed_head, skip_near 7
  chunk_first   the limit of the chunk's first frame for all        bound, skip_near 0   (no frame sees the session)
"""
import numpy as np

import _select_edges as se

SPACING = 25.0
NEVER = 0xFFFFFFFF
MUTANTS = dict(le=("bound", 1), skip_minus=("bound", 8), skip_plus=("bound", 7), no_clamp=("bound", 9),
               clamp_zero=("removed_head", 7), chunk_first=("bound", 0))


class Session:
    """F session frames after M map frames of one synthetic trajectory (global index: map 0 .. M-1, session M .. M+F-1).
    twins: {global index: the earlier global index it copies}; short: {global index: keypoints kept}; removed: the map
    frames taken out again before the session; first: the handle's first_frame_id; skips: the skip_near values tested"""

    def __init__(self, name, F, stream, twins, skips, M=0, short=None, removed=(), first=0, n_kp=40, cfg=None):
        self.name, self.F, self.M, self.stream, self.n_kp, self.first = name, F, M, stream, n_kp, first
        self.twins, self.short, self.removed, self.skips = dict(twins), dict(short or {}), tuple(removed), tuple(skips)
        self.cfg = dict(cfg or {})
        self.c = first + M                       # current_frame_id_ when the session begins
        self._frames = self._descs = self._recs = None

    def frames(self):
        """[(xyz, label)] by global index"""
        if self._frames is None:
            from sgtd_amd import synth
            m = synth.make_map(self.M + self.F, self.n_kp, stream=self.stream, spacing=SPACING)
            xyz, label = m.xyz.copy(), m.label.copy()
            for t, s in sorted(self.twins.items()):
                assert s < t
                xyz[t], label[t] = xyz[s], label[s]
            self._frames = [(xyz[i, :self.short.get(i, self.n_kp)], label[i, :self.short.get(i, self.n_kp)]) for i in range(self.M + self.F)]
        return self._frames

    def ragged(self, lo, hi):
        """frames lo .. hi-1 as (xyz [total, 3], label [total], kp_off)"""
        fr = self.frames()[lo:hi]
        off = np.concatenate([[0], np.cumsum([len(x) for x, _ in fr])]).astype(np.int64)
        return (np.concatenate([x for x, _ in fr]).astype(np.float32).reshape(-1, 3),
                np.concatenate([l for _, l in fr]).astype(np.uint32), off)

    def manager_cfg(self):
        out = dict(self.cfg)
        if self.first:
            out.update(first_frame_id=self.first)
        out.setdefault("max_frame_n", self.first + self.M + self.F + 8)
        return out

    def oracle_cfg(self):
        return {k: v for k, v in self.manager_cfg().items() if k != "first_frame_id"}

    def descs(self, oracle):
        """the oracle's descriptors of every frame, stamped first + global index"""
        if self._descs is None:
            o = oracle.OracleManager(**self.oracle_cfg())
            out = []
            for i, (x, l) in enumerate(self.frames()):
                o.set_current_frame_id(self.first + i)
                out.append(o.build(x, l))
            self._descs = out
        return self._descs

    def kept_map(self):
        return [m for m in range(self.M) if m not in self.removed]

    # ---- the oracle through the reference's loop -----------------------------------------------------------------------
    def oracle_loop(self, oracle, skip, rough=(), verify=(), icp=0.4):
        """before session frame i selects, the oracle holds the frames (kept map, then session) whose id lies below that of
        frame i minus skip.
        -> per frame select() with its nonzero votes {frame: votes}; rough lists and verification where asked"""
        d = self.descs(oracle)
        o = oracle.OracleManager(**self.oracle_cfg())
        order = self.kept_map() + list(range(self.M, self.M + self.F))
        out, added = [], 0
        for i in range(self.F):
            while added < len(order) and order[added] < self.M + i - skip:
                o.add(d[order[added]])
                added += 1
            r = o.select(d[self.M + i])
            v = o.votes()
            r["votes"] = {int(f): int(v[f]) for f in np.flatnonzero(v)}
            if i in rough:
                r["rough"] = o.rough_matches()
            if i in verify:
                cands, best_s, best_k = [], 0.0, -1
                for k in range(len(r["cand_frame"])):
                    s, t, rot, _ = o.verify(k, int(r["cand_off"][k + 1] - r["cand_off"][k]))
                    cands.append((s, t, rot))
                    if s > best_s:
                        best_s, best_k = s, k
                r["verify"] = (cands, (best_k, int(r["cand_frame"][best_k]), best_s) if best_s > icp else (None, -1, 0.0))
            out.append(r)
        return out

    # ---- the restatement -----------------------------------------------------------------------------------------------
    def records(self, oracle):
        """every session frame's match records against the WHOLE table (kept map and every session frame, as the handle
        holds it when the batch runs), frames not looked at: [(descriptor, entry, entry frame)] per session frame, in
        the reference's order; and the table's frame range"""
        if self._recs is None:
            d = self.descs(oracle)
            t = se.RefTable()
            for g in self.kept_map() + list(range(self.M, self.M + self.F)):
                t.add(d[g].side, d[g].label, d[g].frame)
            frame = t.arrays()[1].astype(np.int64)
            rough = self.cfg.get("rough_dis_threshold", oracle.DEFAULTS["rough_dis_threshold"])
            recs = []
            for i in range(self.F):
                q = d[self.M + i]
                rq, _, re_ = se.ref_rough(t, q.side, q.label, NEVER, rough)
                recs.append((rq, re_, frame[re_] if len(re_) else np.zeros(0, np.int64)))
            self._recs = (recs, int(frame.min()), int(frame.max()))
        return self._recs

    def restated(self, oracle, skip, mutant=None, chunk=None):
        """the loop over the records with the bound as loop_bound_kernel and sweep_plan compute it in u32 (mutant: a wrong
        bound; chunk: frames per sgtd_loop_frames call, for the chunk_first mutant) -> per frame what oracle_loop gives"""
        recs, lo, hi = self.records(oracle)
        span = hi - lo + 1
        skip = skip + {"skip_minus": -1, "skip_plus": 1}.get(mutant, 0)
        out = []
        for q in range(self.F):
            q_of = (q // chunk) * chunk if (mutant == "chunk_first" and chunk) else (0 if mutant == "chunk_first" else q)
            lim = self.c + q_of - skip
            if mutant == "no_clamp":
                qf = lim & 0xFFFFFFFF
            else:
                qf = max(lim, 0 if mutant == "clamp_zero" else lo)
            ql = (qf - lo) & 0xFFFFFFFF
            local_limit = ql if ql < span else NEVER
            rq, re_, rf = recs[q]
            local = rf - lo
            see = (local <= local_limit) if mutant == "le" else (local < local_limit)
            out.append(select_from(rq[see], re_[see], rf[see]))
        return out

    def twin_votes(self, oracle, t):
        """the votes the twin source of frame t gets from t when it is visible: t's records against the source's entries"""
        recs, _, _ = self.records(oracle)
        rq, re_, rf = recs[t - self.M]
        return int(np.sum(rf == self.first + self.twins[t]))


def select_from(rq, re_, rf, candidate_num=se.CANDIDATE_NUM):
    """votes, the top-k rule (the first maximum, more than 1 and at least 5 votes) and the lists in record order"""
    frames, counts = np.unique(rf, return_counts=True)
    work = counts.astype(np.int64).copy()
    cf, cv, off, lq, le = [], [], [0], [], []
    for _ in range(candidate_num):
        if len(work) == 0:
            break
        k = int(np.argmax(work))                 # np.unique sorts the frames: the first maximum is the lowest frame
        if not (work[k] > 1 and work[k] >= 5):
            break
        cf.append(int(frames[k]))
        cv.append(int(work[k]))
        work[k] = 0
        sel = rf == frames[k]
        lq.append(rq[sel])
        le.append(re_[sel])
        off.append(off[-1] + int(sel.sum()))
    cat = (lambda a, t: np.concatenate(a).astype(t) if a else np.zeros(0, t))
    return dict(votes={int(f): int(n) for f, n in zip(frames, counts)}, cand_frame=np.array(cf, np.int32), cand_votes=np.array(cv, np.int32),
                cand_off=np.array(off, np.int64), q_idx=cat(lq, np.int32), db_entry=cat(le, np.int64))


def same_select(a, b):
    return (a["votes"] == b["votes"] and all(np.array_equal(a[k], b[k]) for k in ("cand_frame", "cand_votes", "cand_off", "q_idx", "db_entry")))


WIDE = dict(std_side_resolution=0.5, descriptor_max_len=50.0)          # u64 keys (tests/test_gpu_select_edges.py, res0.5_len50)
BIG = 2 ** 31 - 1


def sessions():
    out = [
        # twins at distance 1 (7 copies 6) and 8 (12 copies 4); skip_near d - 1, d, d + 1 for each, and past the session
        Session("bound", 14, 601, {7: 6, 12: 4}, skips=(0, 1, 2, 7, 8, 9, 20, BIG)),
        Session("bound_wide", 14, 601, {7: 6, 12: 4}, skips=(0, 1, 7, 8), cfg=WIDE),
        # frame 14 copies 9 (distance 5), which copies 3 (distance 11): two tied twins
        Session("tied", 16, 602, {9: 3, 14: 9}, skips=(0, 7, 4, 5, 11)),
        # a handle that begins at a large frame id
        Session("first_large", 12, 603, {5: 4, 10: 2}, skips=(0, 1, 8), first=1000000),
        # frames without descriptors: the first two (frame_lo > c), the last two, and one between twins
        Session("short", 14, 604, {9: 3, 11: 2}, skips=(0, 6, 7, 8, 9), short={0: 5, 1: 0, 6: 3, 12: 2, 13: 0}),
        # a map whose first three frames were removed: session frames 0 and 1 copy map frame 3 (= frame_lo) and the
        # bound of the first queries lies below frame_lo
        Session("removed_head", 10, 605, {8: 3, 9: 3, 14: 5}, skips=(7, 0, 5), M=8, removed=(0, 1, 2)),
        # a hole in the map: the bound of the first queries lies inside it; session frame 0 copies map frame 2 (below the
        # hole), frame 1 copies map frame 5 (above it)
        Session("removed_hole", 10, 606, {8: 2, 9: 5}, skips=(4, 3, 0), M=8, removed=(3, 4)),
        # a prebuilt map (tail and merged-tail forms): session frames copy map frames and one another
        Session("on_map", 10, 607, {6: 1, 9: 8, 11: 4}, skips=(0, 1, 2), M=6),
    ]
    return {s.name: s for s in out}


_ALL = None


def all_sessions():
    global _ALL
    if _ALL is None:
        _ALL = sessions()
    return _ALL
