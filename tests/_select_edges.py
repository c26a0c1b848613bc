"""Workloads at the edges of candidate_selector (STDesc.cpp:318-460) and a plain f64 restatement of it.  Plain helper
module of tests/test_select_edges.py (CPU: the restatement equals the oracle, the workloads reach the edges) and
tests/test_gpu_select_edges.py (GPU: every form of the selection equals the oracle on them).

A workload belongs to one rough_dis_threshold (a config setting, so a handle of its own).  It is a list of AddSTDescs
calls (caller-stamped frame ids) and a list of query sets, each one candidate_selector call of query frame QUERY_FRAME.
Every table frame carries BOOST entries (label BOOST_LABEL, all at BOOST_SIDE) and every query set one descriptor
matching them, so that every frame of the table has BOOST votes and a frame with one more match is a candidate: an edge
decision that goes the wrong way changes the candidates, their votes or their lists.  A query set holds at most
MAX_SET frames of its own, so all of them fit in the 50 candidates.  Families use label codes of their own.
"""
import math

import numpy as np

QUERY_FRAME = 19000
MAX_FRAME_N = 20000
CANDIDATE_NUM = 50
BOOST, BOOST_LABEL, BOOST_SIDE = 4, (15, 15, 15), (5.25, 6.25, 7.25)
MAX_SET = 44
ROUGHS = (0.01, 0.03, 0.12, 0.3, 1.0)
RUN_MAX = 48                         # SGTD_RUN_MAX of table_kernels.hip.h
LADDER = ([0.0] + [k * 2.0 ** -52 for k in range(1, 6)] + [10.0 ** -e for e in range(15, 0, -1)])
LADDER = LADDER + [-d for d in LADDER[1:]]
DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [1, 1, 0], [0, -1, 1],
                 [1, -1, 1], [-1, -1, -1], [0.36, 0.48, 0.8], [-0.6, 0.8, 0], [1, 1, 1], [-0.8, 0, -0.6]], np.float64)
DIRS /= np.linalg.norm(DIRS, axis=1, keepdims=True)


def nextafter(x, k):
    """x moved by k f64 ulps (k < 0: down)"""
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


def norm3(v):
    v = np.asarray(v, np.float64)
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


# ---- the restatement ---------------------------------------------------------------------------------------------
def label_code(l):
    """Combinatorial_Binary_Encoding (STDesc.cpp:3-16): three 4-bit fields"""
    return ((int(l[0]) & 15) << 8) | ((int(l[1]) & 15) << 4) | (int(l[2]) & 15)


def c_int(x):
    """(int) of a double: C truncation towards zero"""
    return int(math.trunc(x))


class RefTable:
    """data_base_ of AddSTDescs (:149-172): buckets keyed (code, (int)(s + 0.5) per side), insertion order"""

    def __init__(self):
        self.side, self.frame, self.buckets = [], [], {}

    def add(self, side, label, frame):
        for s, l, f in zip(side, label, frame):
            key = (label_code(l), c_int(s[0] + 0.5), c_int(s[1] + 0.5), c_int(s[2] + 0.5))
            self.buckets.setdefault(key, []).append(len(self.side))
            self.side.append(np.asarray(s, np.float64))
            self.frame.append(int(f))
        self._arr = None

    def arrays(self):
        if self._arr is None:
            self._arr = (np.array(self.side).reshape(-1, 3), np.array(self.frame, np.uint32),
                         {k: np.array(v, np.int64) for k, v in self.buckets.items()})
        return self._arr


def ref_rough(table, qside, qlabel, qframe, rough, thr_scale=1.0):
    """the match records of candidate_selector's loop (:318-403) in f64, in the reference's (i, cell, j) order: the 27
    voxel_round cells with C truncation, the norm() < 1.5 gate, dis < side.norm() * rough, the unsigned frame test
    -> (descriptor, cell, table entry) per record.  thr_scale != 1 is a mutant's (tests/_record_edges.py)"""
    side, frame, buckets = table.arrays()
    rec_q, rec_cell, rec_e = [], [], []
    for i in range(len(qside)):
        s = [float(v) for v in qside[i]]
        thr = float(norm3(s)) * rough * thr_scale
        code = label_code(qlabel[i])
        cell = 0
        for x in (-1, 0, 1):
            for y in (-1, 0, 1):
                for z in (-1, 0, 1):
                    p = (c_int(s[0] + x), c_int(s[1] + y), c_int(s[2] + z))
                    c = cell
                    cell += 1
                    d = [s[k] - (float(p[k]) + 0.5) for k in range(3)]
                    if not math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < 1.5:
                        continue
                    idx = buckets.get((code,) + p)
                    if idx is None:
                        continue
                    # unsigned subtraction of the frame ids > 0: the ids differ
                    idx = idx[(np.uint32(qframe) - frame[idx]) > 0]
                    dis = norm3(np.asarray(s) - side[idx])
                    hit = idx[dis < thr]
                    rec_q += [i] * len(hit)
                    rec_cell += [c] * len(hit)
                    rec_e += hit.tolist()
    return np.array(rec_q, np.int32), np.array(rec_cell, np.int32), np.array(rec_e, np.int64)


def ref_select(table, qside, qlabel, qframe, rough, candidate_num=CANDIDATE_NUM, max_frame_n=MAX_FRAME_N):
    """candidate_selector (:318-460) in f64: the records of ref_rough; votes, the top-k rule, the (i, cell, j) list
    order"""
    frame = table.arrays()[1]
    rec_q, rec_cell, rec_e = ref_rough(table, qside, qlabel, qframe, rough)
    rec_f = frame[rec_e] if len(rec_e) else np.zeros(0, np.uint32)
    votes = np.bincount(rec_f[rec_f < max_frame_n].astype(np.int64), minlength=max_frame_n).astype(np.float64)
    work = votes.copy()
    cf, cv, off, lq, le = [], [], [0], [], []
    for _ in range(candidate_num):
        k = int(np.argmax(work))             # the first maximum (:427-432 with max_vote starting at 1)
        if not (work[k] > 1 and work[k] >= 5):
            break
        cf.append(k)
        cv.append(int(work[k]))
        work[k] = 0
        sel = rec_f == k
        lq.append(rec_q[sel])
        le.append(rec_e[sel])
        off.append(off[-1] + int(sel.sum()))
    cat = (lambda a, t: np.concatenate(a).astype(t) if a else np.zeros(0, t))
    return dict(votes=votes, M=len(rec_e), rough=(rec_q, rec_cell, rec_e), cand_frame=np.array(cf, np.int32),
                cand_votes=np.array(cv, np.int32), cand_off=np.array(off, np.int64), q_idx=cat(lq, np.int32),
                db_entry=cat(le, np.int64))


# ---- workloads ---------------------------------------------------------------------------------------------------
class Workload:
    def __init__(self, rough, stamped=False):
        self.rough = rough
        # stamped: every AddSTDescs call carries one frame, whose id is the handle's current frame id (0, 1, 2, ...: what
        # a multi-device table takes, and frame ids in insertion order, what a tail segment needs)
        self.stamped = stamped
        self.adds = []             # (side [n, 3], label [n, 3], frame [n]) per AddSTDescs call
        self.sets = []             # (side [n, 3], label [n, 3], family) per candidate_selector call
        self.next_frame = 0
        self.tags = {}             # family -> set indices

    def frames(self, n, order=None):
        ids = list(range(self.next_frame, self.next_frame + n))
        self.next_frame += n
        assert self.next_frame < QUERY_FRAME
        return ids if order is None else [ids[k] for k in order]

    def add(self, side, label, frame, boost=True):
        side = np.asarray(side, np.float64).reshape(-1, 3)
        label = np.broadcast_to(np.asarray(label, np.int32).reshape(-1, 3), side.shape).copy()
        frame = np.broadcast_to(np.asarray(frame, np.uint32).reshape(-1), side.shape[:1]).copy()
        if boost:
            for f in sorted(set(frame.tolist())):
                side = np.concatenate([side, np.tile(BOOST_SIDE, (BOOST, 1))])
                label = np.concatenate([label, np.tile(BOOST_LABEL, (BOOST, 1)).astype(np.int32)])
                frame = np.concatenate([frame, np.full(BOOST, f, np.uint32)])
        if self.stamped:                                   # one call per frame, in frame order
            for f in sorted(set(frame.tolist())):
                m = frame == f
                self.adds.append((side[m], label[m], frame[m]))
            return
        self.adds.append((side, label, frame))

    def query(self, side, label, family):
        side = np.asarray(side, np.float64).reshape(-1, 3)
        label = np.broadcast_to(np.asarray(label, np.int32).reshape(-1, 3), side.shape)
        side = np.concatenate([side, [BOOST_SIDE]])
        label = np.concatenate([label, [BOOST_LABEL]]).astype(np.int32)
        self.tags.setdefault(family, []).append(len(self.sets))
        self.sets.append((side, label, family))

    def n_entries(self, upto=None):
        return sum(len(a[0]) for a in self.adds[:upto])

    def descs(self, mod, side, label, frame):
        d = mod.Descs(len(side))
        d.side[:] = side
        d.label[:] = label
        d.frame[:] = frame
        return d

    def load(self, mgr, mod, lo=0, hi=None):
        for side, label, frame in self.adds[lo:hi]:
            d = self.descs(mod, side, label, frame)
            mgr.add(d) if hasattr(mgr, "add") else mgr.AddSTDescs(d)

    def query_descs(self, mod, k):
        side, label, _ = self.sets[k]
        return self.descs(mod, side, label, np.full(len(side), QUERY_FRAME, np.uint32))

    def ref_table(self):
        t = RefTable()
        for a in self.adds:
            t.add(*a)
        return t


def _pack(wl, items, label, family):
    """items: (query sides, [(entry sides, ...) per frame]) -> frames + query sets of at most MAX_SET frames"""
    qs, nf = [], 0
    for q, frames in items:
        if nf + len(frames) > MAX_SET and qs:
            wl.query(np.concatenate(qs), label, family)
            qs, nf = [], 0
        for e in frames:
            e = np.asarray(e, np.float64).reshape(-1, 3)
            e = e[np.all((e >= 0) & (e < 65535.5), axis=1)]
            if len(e):
                wl.add(e, label, wl.frames(1))
        qs.append(np.asarray(q, np.float64).reshape(-1, 3))
        nf += len(frames)
    if qs:
        wl.query(np.concatenate(qs), label, family)


def shell(wl, label=(1, 1, 1)):
    """entries at thr (1 + d) from a query along many directions, query magnitudes 1e-3 ... 6e4, at a cell's inside and
    at its corner (the shell crosses into neighbouring cells)"""
    base = np.array([0.48, 0.6, 0.64])
    items = []
    for M in (1e-3, 0.5, 1.0, 50.0, 1e3, 6e4):
        for corner in (False, True):
            q = M * base
            if corner:
                q = np.floor(q) + 0.5 + 0.37 * wl.rough * norm3(q) * np.array([1, -1, 1]) / max(1.0, M ** 0.5)
            if corner and M < 1:
                continue
            thr = float(norm3(q)) * wl.rough
            frames = []
            for u in DIRS:
                e = np.array([q + thr * (1.0 + d) * u for d in LADDER])
                e = e[np.all(e >= 0, axis=1) & np.all(e < 65535, axis=1)]
                frames.append(e)
            items.append((q, frames))
    _pack(wl, items, label, "shell")


def slices(wl, label=(1, 2, 1)):
    """entries on, and an ulp or a hair beside, a half (second side) or a third (third side) of their cell, each with
    queries whose reach q +- thr ends just past it, from either side"""
    items = []
    for c in ((20, 30, 40), (3, 4, 5), (60, 2, 9)):
        qn = float(norm3(c))
        for ax, n in ((1, 2), (2, 3)):
            for b in range(n):
                B = c[ax] - 0.5 + b / n                       # a slice boundary of the cell (b = 0: the cell's own)
                es = [nextafter(B, k) for k in (-2, -1, 0, 1, 2)] + [B - 1e-9, B + 1e-9, B - 1e-6, B + 1e-6]
                ent, qs = [], []
                for v in es:
                    e = np.array(c, np.float64) + 0.1
                    e[ax] = v
                    ent.append(e)
                    thr = qn * wl.rough                          # (about: the query's own norm decides)
                    for sgn in (-1, 1):
                        for rel in (1e-7, 1e-4, -1e-7):
                            q = e.copy()
                            q[ax] = v + sgn * thr * (1.0 - rel)
                            q[ax] = v + sgn * float(norm3(q)) * wl.rough * (1.0 - rel)
                            if q[ax] >= 0:
                                qs.append(q)
                items.append((np.array(qs), [np.array(ent)]))
    _pack(wl, items, label, "slices")


def run_limit(rough, a, b):
    """the run rule of slice_assign_kernel: a and b could both match one query"""
    f = 2.0 * rough / (1.0 - rough) * (1.0 + 1e-9) if rough < 1 else np.inf
    return f * max(float(norm3(a)), float(norm3(b))) + 1e-9


def sub_cell(s):
    def ax(v, n):
        y = v + 0.5
        return min(max(c_int(y * n) - c_int(y) * n, 0), n - 1)
    return ax(s[1], 2) * 3 + ax(s[2], 3)


def runs(wl, label=(1, 3, 1)):
    """two entries of one frame in one bucket, in different sub-cells, at ||a - b|| just below / above the run rule's
    limit and between half the limit and the limit; the higher sub-cell inserted first; queries at their midpoint.
    Runs of 47 / 48 / 49 members whose only close pair is the first and the last.  Frame ids stamped in descending order,
    one call carrying two frames."""
    r = wl.rough
    items = []
    for c in ((0, 0, 0), (1, 1, 1), (2, 3, 2), (6, 5, 7)):
        for ax, B in ((1, c[1]), (2, c[2] - 0.5 + 1.0 / 3), (2, c[2] - 0.5 + 2.0 / 3)):
            for rel in (-1e-7, 1e-7, -0.45, -0.3, 0.2):
                a = np.array(c, np.float64) + 0.1 * (c[0] > 0)
                d = 0.5
                for _ in range(6):                      # fixed point: the limit depends on the entries' norms
                    a[ax], b = B - d / 2, None
                    b = a.copy()
                    b[ax] = B + d / 2
                    lim = run_limit(r, a, b) if r < 1 else 0.4
                    d = lim * (1.0 + rel)
                if not (np.all(a >= 0) and c_int(a[ax] + 0.5) == c[ax] == c_int(b[ax] + 0.5) and 0 < d < 1):
                    continue
                if sub_cell(a) == sub_cell(b):
                    continue
                hi_first = (a, b) if sub_cell(a) > sub_cell(b) else (b, a)
                m = (a + b) / 2
                items.append((np.array([m, a, b]), [np.array(hi_first)]))
    _pack(wl, items, label, "runs")
    if r <= 0.03:                                        # long runs: members on a grid further apart than the limit
        for n in (47, 48, 49):
            c = np.array([1.0, 1.0, 1.0]) if r > 0.01 else np.array([3.0, 3.0, 3.0])
            g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
            pts = c - 0.45 + 0.29 * g[:n - 1]
            last = pts[0].copy()
            last[2] += 0.55 * run_limit(r, pts[0], pts[0])
            if sub_cell(last) == sub_cell(pts[0]):
                last[2] = c[2] - 0.5 + 1.0 / 3 + 1e-3
                pts[0][2] = last[2] - 0.55 * run_limit(r, pts[0], pts[0]) * 0.9
            pts = np.concatenate([pts, [last]])
            pts = pts[::-1].copy()                        # (the close pair's higher sub-cell first)
            f = wl.frames(1)
            wl.add(pts, label, f)
            wl.query(np.concatenate([[(pts[0] + pts[-1]) / 2], pts[::5]]), label, "runs")
    # frame ids out of insertion order, and two frames in one call (unless the workload is stamped)
    ids = wl.frames(6, order=None if wl.stamped else [5, 3, 4, 0, 2, 1])
    rng = np.random.default_rng(int(r * 1000) + 5)
    c = np.array([4.0, 5.0, 6.0])
    sides = [c - 0.45 + 0.9 * rng.random((12, 3)) for _ in ids]
    for k in (0, 2):
        wl.add(np.concatenate([sides[k], sides[k + 1]]), label, np.repeat([ids[k], ids[k + 1]], 12))
    for k in (4, 5):
        wl.add(sides[k], label, ids[k])
    wl.query(c - 0.45 + 0.9 * rng.random((10, 3)), label, "runs")


def gate(wl, label=(1, 4, 1)):
    """query sides at exactly 1.5 from a probed cell's centre (an axis offset of 1.5; offsets (1, 1, 0.5)) and one ulp
    either side, each with an entry just inside the cell's corner facing the query"""
    items = []
    base = np.array([40.0, 50.0, 60.0])
    pats = []
    for ax in range(3):
        for sg in (1, -1):
            o = np.full(3, 0.5)
            o[ax] = 0.0                                   # side at an integer: the cell above (below) at 1.5 (0.5) ...
            pats.append((o, ax, sg))
    for ax in range(3):
        o = np.full(3, 0.5)
        o[ax] = 0.0                                       # two axes at 1 from the centre, the third at 0.5
        pats.append((o, ax, 0))
    for o, ax, sg in pats:
        q0 = base + o
        for k in (-1, 0, 1):
            for kax in range(3):
                q = q0.copy()
                q[kax] = nextafter(q[kax], k)
                ents = []
                for x in (-1, 0, 1):
                    for y in (-1, 0, 1):
                        for z in (-1, 0, 1):
                            p = np.array([c_int(q[0] + x), c_int(q[1] + y), c_int(q[2] + z)], np.float64)
                            lo, hi = p - 0.5, p + 0.5
                            e = np.clip(q, lo + 1e-9, hi - 1e-9)
                            ents.append(e)
                items.append((q, [np.array(ents)]))
    _pack(wl, items, label, "gate")


SPECIAL = [0.0, -0.0, 2.0 ** -60, 1e-17, 2.0 ** -53, 0.3, 0.49, 0.5, nextafter(0.5, -1), 0.77, nextafter(1.0, -1),
           1.0, nextafter(2.0, -1), 2.0, nextafter(64.0, -1), 64.0, 7.5, nextafter(7.5, -1),
           nextafter(65536.0, -1), 65534.5, nextafter(65534.5, -1)]


def cells(wl, label=(1, 5, 1)):
    """entries at n + 0.5 and one ulp below (the key's rounding); sides below 1 and 0.5 (cell 0 probed twice), below
    2^-53, +0.0 and -0.0; the largest double below 1, 2, 64 and 65536"""
    items = []
    for v in SPECIAL:
        for ax in range(3):
            q = np.array([3.3, 4.2, 5.1])
            q[ax] = v
            if v > 1e4:
                q = q + np.array([30000.0, 0, 0]) * (ax != 0)       # (a threshold that reaches the neighbours)
            ents = []
            for w in (v, v + 0.1, max(v - 0.2, 0.0), 0.0, 0.25, 0.499, c_int(v) + 0.5, nextafter(c_int(v) + 0.5, -1),
                      c_int(v) - 0.5 if v >= 1 else 0.1, nextafter(max(c_int(v) - 0.5, 0.0), -1) if v >= 1 else 0.2):
                e = q.copy()
                e[ax] = abs(w)
                ents.append(e)
            items.append((q, [np.array(ents)]))
    _pack(wl, items, label, "cells")


def homes(wl, label=(1, 6, 1)):
    """1 .. 9 query descriptors sharing one home cell over its sub-cell classes (passes of four, a ragged last pass,
    a union of different reaches), entries around"""
    rng = np.random.default_rng(int(wl.rough * 1000) + 11)
    items = []
    for k in range(1, 10):
        home = np.array([10.0 + 3 * k, 20.0, 30.0])
        q = home + np.stack([rng.random(k), (np.arange(k) + 0.5) / k, ((np.arange(k) * 7) % k + 0.5) / k], 1)
        ents = home - 1.4 + 3.8 * rng.random((60, 3))
        items.append((q, [ents[:30], ents[30:]]))
    _pack(wl, items, label, "homes")


def envelope(wl, label=(1, 7, 1)):
    """query sides at and past the home keys' marker 2^cbits - 1 of every config (descriptors of different real cells
    that would share a key), at and past 65536 (entries in the cells the 16-bit key would alias to), negative sides"""
    items = []
    for ax in range(3):
        vals = [15.3, 16.3, 20.3, 31.3, 32.3, 40.3, 63.3, 64.3, 70.3, 127.3, 128.3, 140.3, 255.3, 256.3, 300.3]
        qs, ents = [], []
        for v in vals:
            q = np.array([5.3, 6.4, 7.2])
            q[ax] = v
            qs.append(q)
            e = q.copy()
            e[(ax + 1) % 3] += 0.4
            ents.append(e)
        items.append((np.array(qs), [np.array(ents[:8]), np.array(ents[8:])]))
    for v in (65535.2, 65535.7, 65536.0, 65536.2, 65537.9, 65600.0, 70000.0, 131072.5):
        for ax in range(3):
            q = np.array([1.3, 2.4, 1.2])
            q[ax] = v
            ents = []
            for w in (0.2, 0.7, 1.4, 2.2, 65534.7, 65535.2, nextafter(65535.5, -1)):
                e = q.copy()
                e[ax] = w
                ents.append(e)
            items.append((q, [np.array(ents)]))
    for v in (-0.3, -0.7, -1.2, -2.6, -2.0 ** -60):
        for ax in range(3):
            q = np.array([20.2, 30.1, 25.3])
            q[ax] = v
            ents = []
            for w in (0.0, 0.2, 0.45, 0.6, 1.3):
                e = q.copy()
                e[ax] = w
                ents.append(e)
            items.append((q, [np.array(ents)]))
    _pack(wl, items, label, "envelope")


def big_frame(wl, label=(1, 8, 1), n=8300):
    """one query frame of more than 8192 descriptors (SGTD_SMALL_SLOTS)"""
    rng = np.random.default_rng(3)
    c = np.array([8.0, 9.0, 10.0])
    for f in wl.frames(20):
        wl.add(c - 2 + 4 * rng.random((150, 3)), label, f)
    wl.query(c - 2 + 4 * rng.random((n, 3)), label, "big")


def workload(rough, stamped=False):
    wl = Workload(rough, stamped)
    for fam in (shell, slices, runs, gate, cells, homes, envelope):
        fam(wl)
    if rough == 0.03:
        big_frame(wl)
    return wl
