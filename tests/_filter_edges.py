"""Workloads at the edges of the per-query restriction path (sgtd_set_frame_filter, sgtd_set_position_prior: the filter
pass over the match records, the diagnostic compaction, the re-basing of the caller's rows to the table's span, the rows
a prior makes) and a plain restatement of the rule.  Plain helper module of tests/test_filter_edges.py (CPU: the
restatement equals the oracle of the allowed frames, every family reaches its edges, every mutant is caught) and
tests/test_gpu_filter_edges.py (GPU: every form equals the restatement on them).

The rule (include/sgtd_accel.h): under rows R query q is answered as by a table that holds only the entries of the frames
R[q] allows — same ids, order and current frame id.  So the expected answer is _select_edges.ref_select over a RefTable
of the allowed frames' entries; entry ids of the full table map to it by their rank among the allowed entries.

A descriptor case is a _record_edges.Case whose query carries one descriptor `a` matched by L table entries at the
identical side and label, one per frame (record j of its list is frame j of the table), and one descriptor matched by
BOOST entries of every frame: an allowed frame with its record alive has BOOST + 1 votes and is a candidate, one whose
record was wrongly killed has BOOST, a forbidden one 0 — the vote vector says which record died, M how many.  Every case
carries its filters as they go to the ABI (frame_lo, n_frames, the row words), never id lists alone.
"""
import numpy as np

import _record_edges as rec
import _select_edges as se

BOOST = se.BOOST
FILT_PREFETCH = 256                  # records of a list filter_records_kernel holds in flight, one quad per lane
LDS_FRAMES = 65536 * 8               # the widest span whose row filter_records_kernel stages in LDS (launch_filter)
TABLE_LO = 1000                      # first frame of the caller-stamped tables
LIST_LENGTHS = (0, 1, 3, 4, 5, 255, 256, 257, 260, 511, 513, 1030)
SLOT_COUNTS = (1, 63, 64, 65, 257, 600)
BIT_SPANS = (128, 129, 191)
BIT_OFFSETS = (-65, -64, -63, -1, 1, 63, 64, 65)        # the filter range's start relative to the table's first frame
WIDE_SPANS = (LDS_FRAMES, LDS_FRAMES + 1)
ROUGH_LENGTHS = (0, 1, 63, 64, 65, 200)
FAMILY_KEYS = {"lists": 0, "slots": 700, "dead": 1400, "bits": 1500, "wide": 1600, "rough": 1700}

MUTANTS = ("f_le_span", "bit31", "word_border", "row0", "tail_last_ignored", "past256_ignored", "dead_twice",
           "shift_sign", "no_last_mask")
KEYS = ("cand_frame", "cand_votes", "cand_off", "q_idx", "db_entry")


# ---- filters as the ABI takes them -------------------------------------------------------------------------------
class Filt:
    """the arguments of sgtd_set_frame_filter: rows uint64 [n_rows, ceil(n_frames / 64)]"""

    def __init__(self, name, frame_lo, n_frames, rows):
        self.name, self.lo, self.n = name, int(frame_lo), int(n_frames)
        self.rows = np.ascontiguousarray(rows, np.uint64)
        assert self.rows.ndim == 2 and self.rows.shape[1] == (self.n + 63) // 64 and self.lo >= 0 and self.n >= 1


def make_filter(name, frame_lo, n_frames, allowed_rows, garbage=True):
    """rows over [frame_lo, frame_lo + n_frames): bit f - frame_lo set for the ids of allowed_rows[r] inside the range.
    garbage: the bits of the last word at and beyond n_frames are set as well (frames outside the range are never
    allowed: the library has to ignore them)"""
    words = (n_frames + 63) // 64
    bits = np.zeros((len(allowed_rows), words * 64), bool)
    for r, ids in enumerate(allowed_rows):
        d = np.asarray(ids, np.int64).reshape(-1) - frame_lo
        bits[r, d[(d >= 0) & (d < n_frames)]] = True
    if garbage:
        bits[:, n_frames:] = True
    rows = np.packbits(bits, axis=1, bitorder="little").reshape(len(allowed_rows), words, 8)
    return Filt(name, frame_lo, n_frames, np.ascontiguousarray(rows).view("<u8").reshape(len(allowed_rows), words))


def filt_allows(filt, r, frames, table_lo=0, mutant=None):
    """the rule: is frame id frames[i] allowed to query r?  bit (f - frame_lo) of row r (row 0 when there is one), and
    only inside [frame_lo, frame_lo + n_frames).  mutant: one of the row mutants of MUTANTS (a wrong restatement)"""
    rows = filt.rows
    words = rows.shape[1]
    row = rows[0 if rows.shape[0] == 1 or mutant == "row0" else r]
    frames = np.asarray(frames, np.int64)
    f = frames - filt.lo
    if mutant == "shift_sign":           # the re-base shifts the caller's row the wrong way
        f = (frames - table_lo) - (table_lo - filt.lo)
    hi = {"f_le_span": filt.n + 1, "no_last_mask": words * 64}.get(mutant, filt.n)
    inside = (f >= 0) & (f < hi)
    fc = np.clip(f, 0, words * 64)
    word = fc >> 6
    if mutant == "word_border":          # the first bit of a word read from the word before
        word = np.where(fc % 64 == 0, word - 1, word)
    inside &= (word >= 0) & (word < words)
    bit = (fc & (31 if mutant == "bit31" else 63)).astype(np.uint64)
    return inside & (((row[np.clip(word, 0, words - 1)] >> bit) & np.uint64(1)) == 1)


class FCase(rec.Case):
    def __init__(self, name, family, **kw):
        super().__init__(name, family, **kw)
        self._next_key = FAMILY_KEYS[family]
        self.filters = []

    @property
    def table_lo(self):
        return int(min(self.eframe))

    @property
    def span(self):
        return int(max(self.eframe)) - self.table_lo + 1

    def frames(self):
        return np.unique(np.asarray(self.eframe, np.int64))

    def add_filter(self, name, frame_lo, n_frames, allowed, garbage=True):
        self.filters.append(make_filter(name, frame_lo, n_frames, [allowed], garbage))

    def records(self, k, scale=1.0):
        """the match records of query k over the whole table (cached)"""
        key = (k, scale)
        if key not in self.__dict__.setdefault("_recs", {}):
            side, label = rec.key_sides_labels(self.queries[k])
            self._recs[key] = se.ref_rough(self.full_table(), side, label, self.query_frame, rec.ROUGH, thr_scale=scale)
        return self._recs[key]

    def full_table(self):
        if "_tab" not in self.__dict__:
            self._tab = self.ref_table()
        return self._tab

    def n_dead(self, k):
        """records within 1e-12 (relative) beyond the threshold: nothing f32 can decide, dead by the f64 test"""
        return len(self.records(k, 1.0 + 1e-12)[0]) - len(self.records(k)[0])


def held_entries(c, filt, r=0, mutant=None):
    """mask over the table entries of case c: the entries of the frames the filter allows to query r"""
    return filt_allows(filt, r, np.asarray(c.eframe, np.int64), c.table_lo, mutant)


def ref_filtered(c, k, filt, r=0, mutant=None):
    """the expected answer of query k of case c under `filt` (row r): ref_select over a table of the allowed frames'
    entries — votes, M, candidates, offsets, lists and the rough list, entry ids those of that table; `held`: the mask of
    its entries over the full table (rank among the held entries = id in that table).  A row mutant changes the allowed
    set; a record mutant is a wrong filter pass over the full table's records (ref_by_records)"""
    if mutant in ("tail_last_ignored", "past256_ignored", "dead_twice"):
        return ref_by_records(c, k, filt, r, mutant)
    held = held_entries(c, filt, r, mutant)
    side, label, frame = c.entry_arrays()
    tab = se.RefTable()
    tab.add(side[held], label[held], frame[held])
    qs, ql = rec.key_sides_labels(c.queries[k])
    ans = se.ref_select(tab, qs, ql, c.query_frame, rec.ROUGH, c.cn, c.max_frame_n)
    rq, rcell, re_ = ans.pop("rough")
    tside, tframe, _ = tab.arrays()
    ans["rough"] = dict(q_idx=rq, cell=rcell, db_entry=re_, frame=tframe[re_] if len(re_) else np.zeros(0, np.uint32),
                        dis=se.norm3(qs[rq] - tside[re_]) if len(re_) else np.zeros(0))
    ans["held"] = held
    return ans


def ref_by_records(c, k, filt, r=0, mutant=None):
    """the filter pass restated over the records of the full table: record j of a list dies when its frame is not
    allowed, M loses each killed record once; the passes of _record_edges.ref_passes over the survivors.  Entry ids are
    mapped to the table of the held entries, as ref_filtered gives them"""
    rq, _, re_ = c.records(k)
    frame = c.full_table().arrays()[1]
    kill = ~filt_allows(filt, r, frame[re_], c.table_lo) if len(re_) else np.zeros(0, bool)
    lengths = np.bincount(rq, minlength=len(c.queries[k])) if len(rq) else np.zeros(len(c.queries[k]), np.int64)
    j = np.arange(len(rq)) - (np.cumsum(lengths) - lengths)[rq] if len(rq) else np.zeros(0, np.int64)
    if mutant == "tail_last_ignored":
        kill &= ~((lengths[rq] % 4 != 0) & (j == lengths[rq] - 1))
    if mutant == "past256_ignored":
        kill &= j < FILT_PREFETCH
    keep = ~kill
    ans = rec.ref_passes(rq[keep], re_[keep], frame, len(c.queries[k]), c.cn, c.max_frame_n)
    if mutant == "dead_twice":
        ans["M"] -= c.n_dead(k)
    held = held_entries(c, filt, r)
    ans["db_entry"] = (np.cumsum(held) - 1)[ans["db_entry"]]
    ans["held"] = held
    return ans


def same(a, b):
    return a["M"] == b["M"] and np.array_equal(a["votes"], b["votes"]) and all(np.array_equal(a[k], b[k]) for k in KEYS)


def list_positions(c, k, filt, desc=0):
    """(frame, killed) per record of descriptor `desc`'s list, in list order"""
    rq, _, re_ = c.records(k)
    fr = c.full_table().arrays()[1][re_[rq == desc]].astype(np.int64)
    return fr, ~filt_allows(filt, 0, fr, c.table_lo)


# ---- families ----------------------------------------------------------------------------------------------------
def _one_list(name, family, L, frames, **kw):
    """a table of `frames`; the first L hold one entry of key a, all hold BOOST entries of key b; the query is (a, b)"""
    c = FCase(name, family, **kw)
    a, b = c.keys(2)
    for i, f in enumerate(frames):
        if i < L:
            c.entries([a], f)
        c.entries([b] * BOOST, f)
        c.end_call()
    c.query([a, b])
    c.info = dict(L=L, a=a, b=b)
    return c


def lists():
    """list lengths around the 256 records in flight and the 64-lane trips behind them, every L % 4; filters that kill
    quad position p of every quad (p = 0 .. 3), only the last record, all but the last; `shard`: a range from frame 5
    that ends inside the table, flips at frames 63 | 64 and 127 | 128 (the 64-frame blocks of a sharded table)"""
    out = []
    for L in LIST_LENGTHS:
        F = L + 3
        c = _one_list("lists/L%d" % L, "lists", L, range(F))
        c.tail_at = max(F // 2, 1)
        ids = np.arange(F)
        for p in range(4):
            c.add_filter("p%d" % p, 0, F, ids[ids % 4 != p])
        if L:
            c.add_filter("last", 0, F, ids[ids != L - 1])
            c.add_filter("only_last", 0, F, ids[ids >= L - 1])
        if F >= 130:
            al = (set(ids[ids % 3 == 0].tolist()) | {63, 128}) - {64, 127}
            c.add_filter("shard", 5, F - 7, sorted(al))
        out.append(c)
    return out


def slots():
    """queries of 1, 63, 64, 65, 257 and 600 descriptors (the last one the boost descriptor): descriptor i has 1 + i % 5
    records over 12 frames"""
    out = []
    for n in SLOT_COUNTS:
        c = FCase("slots/n%d" % n, "slots")
        k = c.keys(n - 1)
        b = c.keys(1)[0]
        i = np.repeat(np.arange(n - 1), 1 + np.arange(n - 1) % 5)
        j = np.arange(len(i)) - np.repeat(np.cumsum(1 + np.arange(n - 1) % 5) - (1 + np.arange(n - 1) % 5), 1 + np.arange(n - 1) % 5)
        f = (i + j) % 12
        for fr in range(12):
            c.entries(k[i[f == fr]], fr)
            c.entries([b] * BOOST, fr)
            c.end_call()
        c.query(np.concatenate([k, [b]]))
        c.tail_at = 6
        ids = np.arange(12)
        c.add_filter("even", 0, 12, ids[ids % 2 == 0])
        c.add_filter("but34", 0, 12, ids[(ids != 3) & (ids != 4)])
        c.info = dict(n=n)
        out.append(c)
    return out


def _ladder():
    """_select_edges.LADDER around dis == thr as shifts, inside and beyond the threshold interleaved"""
    inside = [d for d in se.LADDER if d < 0]
    beyond = [d for d in se.LADDER if d >= 0]
    out = []
    for i in range(max(len(inside), len(beyond))):
        out += inside[i:i + 1] + beyond[i:i + 1]
    return [1.0 + d for d in out]


def dead():
    """one entry per frame at thr (1 + d) from the query's descriptor, d over the ladder, inside and beyond the threshold
    alternating in insertion (= list) order: the records the sweep cannot decide and the f64 test resolves to dead lie
    between live ones; filters that forbid every inside frame, every second one, none"""
    c = FCase("dead/ladder", "dead")
    a, b = c.keys(2)
    sh = _ladder()
    for f, s in enumerate(sh):
        c.entries([a], f, shift=s)
        c.entries([b] * BOOST, f)
        c.end_call()
    c.query([a, b])
    c.tail_at = len(sh) // 2
    ids = np.arange(len(sh))
    live = ids[np.asarray(sh) < 1.0]
    c.add_filter("no_live", 0, len(sh), np.setdiff1d(ids, live))
    c.add_filter("half_live", 0, len(sh), np.setdiff1d(ids, live[::2]))
    c.add_filter("all", 0, len(sh), ids)
    c.info = dict(a=a, shifts=sh)
    return [c]


def _bit_pattern(span, on):
    """local frames allowed: 0, 63, 65, span - 1 and every seventh in between, not 64 (on) — or the complement"""
    loc = np.arange(span)
    al = np.isin(loc, [0, 63, 65, span - 1]) | (loc % 7 == 3)
    al[64] = False
    return loc[al if on else ~al]


def bits():
    """tables stamped from TABLE_LO with spans 128, 129, 191 (span % 64 = 0, 1, 63), every frame present; filter ranges
    that start 1, 63, 64, 65 below and above the table's first frame and end beyond the table or three frames inside it,
    one wholly below and one wholly above; flips at local 0, 63, 64, 65 and span - 1 in both polarities"""
    out = []
    for span in BIT_SPANS:
        c = _one_list("bits/span%d" % span, "bits", span, range(TABLE_LO, TABLE_LO + span))
        for s in BIT_OFFSETS:
            ends_inside = abs(s) in (65, 63)
            end = TABLE_LO + span - 3 if ends_inside else TABLE_LO + span + 70
            for on in (True, False):
                c.add_filter("s%+d/%s/%s" % (s, "inside" if ends_inside else "past", "on" if on else "off"), TABLE_LO + s,
                             end - (TABLE_LO + s), TABLE_LO + _bit_pattern(span, on))
        c.add_filter("below", TABLE_LO - 200, 150, np.arange(TABLE_LO - 200, TABLE_LO - 50))
        c.add_filter("above", TABLE_LO + span + 10, 100, np.arange(TABLE_LO + span + 10, TABLE_LO + span + 110))
        c.info["span"] = span
        out.append(c)
    return out


def wide_locals(span):
    far = 64 * 4000
    return np.array([0, 1, 63, 64, 65, 127, 128, far - 1, far, far + 1, far + 63, far + 64, span - 130, span - 129, span - 128,
                     span - 66, span - 65, span - 64, span - 63, span - 3, span - 2, span - 1])


def wide():
    """frame ids stamped so that the span is exactly 524 288 (the last launch with the row in LDS, 64 KB of it) and
    524 289 (the first with the row in memory): 22 frames — the first, the last, both sides of word borders at the front,
    far into the row and at its end; a range from 65 below the table, one from 1 above it"""
    out = []
    for span in WIDE_SPANS:
        loc = wide_locals(span)
        c = _one_list("wide/span%d" % span, "wide", len(loc), TABLE_LO + loc, max_frame_n=600000)
        ids = TABLE_LO + loc
        c.add_filter("s-65/even", TABLE_LO - 65, span + 65 + 10, ids[0::2])
        c.add_filter("s-65/odd", TABLE_LO - 65, span + 65 + 10, ids[1::2])
        c.add_filter("s+1/thirds", TABLE_LO + 1, span - 3, ids[np.arange(len(ids)) % 3 != 1])
        c.info["span"] = span
        out.append(c)
    return out


def rough():
    """the compaction's list lengths (0, 1, 63, 64, 65, 200 records: none, one and several 64-record steps) beside a
    ladder list with already-dead records, under filters that keep all, none and every second frame"""
    c = FCase("rough/steps", "rough")
    k = c.keys(len(ROUGH_LENGTHS))
    a, b = c.keys(2)
    sh = _ladder()
    F = max(ROUGH_LENGTHS)
    for f in range(F):
        c.entries(k[np.asarray(ROUGH_LENGTHS) > f], f)
        if f < len(sh):
            c.entries([a], f, shift=sh[f])
        c.entries([b] * BOOST, f)
        c.end_call()
    c.query(np.concatenate([k, [a, b]]))
    c.tail_at = F // 2
    ids = np.arange(F)
    c.add_filter("all", 0, F, ids)
    c.add_filter("none", 0, F, [])
    c.add_filter("alternating", 0, F, ids[ids % 2 == 1])
    c.info = dict(a=a, shifts=sh, keys=k)
    return [c]


FAMILIES = (lists, slots, dead, bits, wide, rough)


def cases(families=None):
    out = []
    for fam in FAMILIES:
        if families is None or fam.__name__ in families:
            out += fam()
    return out


# ---- keypoint batches: per-query rows --------------------------------------------------------------------------------
KP_FRAMES, KP_QUERIES, KP_POINTS = 16, 12, 200


def kp_world(synth):
    """a map of 16 keypoint frames (ids TABLE_LO ..) and 12 queries, query q a second look at frame gt[q], all distinct
    -> (map, queries, gt, the filters; their per-query rows have a closing row for a query without keypoints that a batch
    appends): `per_query` — row q allows gt[q] and a third of the other frames, never the
    frame of another query (row q - 1 or row 0 used for query q loses q's own frame), from a range that starts 3 below
    the table; `shared` — one row; `above` — per-query rows from a range that starts 2 above the table's first frame"""
    m = synth.make_map(KP_FRAMES, KP_POINTS, stream=411, spacing=25.0)
    gt = (np.arange(KP_QUERIES) * 5) % KP_FRAMES
    qs = synth.make_queries(m, KP_QUERIES, stream=412, frames=gt)
    loc = np.arange(KP_FRAMES)
    rows = []
    for q in range(KP_QUERIES):
        al = ((loc + q) % 3 == 0) & ~np.isin(loc, gt)
        al[gt[q]] = True
        rows.append(TABLE_LO + loc[al])
    rows.append(TABLE_LO + loc)                   # (the row of a batch's closing query without a keypoint)
    n = KP_FRAMES
    filters = dict(
        per_query=make_filter("per_query", TABLE_LO - 3, n + 8, rows),
        shared=make_filter("shared", TABLE_LO - 3, n + 8, [TABLE_LO + loc[loc % 4 != 1]]),
        above=make_filter("above", TABLE_LO + 2, n - 5, rows))
    return m, qs, gt, filters


# ---- position priors: the rule's edge decisions ----------------------------------------------------------------------
def _f32(*v):
    return np.array(v, np.float32)


_DEN = float(np.float32(1e-45))          # the smallest f32 denormal, exact in f64
_UP = float(np.nextafter(np.float32(1.5), np.float32(2)))
# (name, translation f32 [3], center, radius, allowed): the prior's decision for a frame with that pose
PRIOR_EDGES = (
    ("r3_exact", _f32(2, 3, 6), (0.0, 0.0, 0.0), 7.0, True),                     # 4 + 9 + 36 == 49 exactly
    ("r3_ulp_below", _f32(2, 3, 6), (0.0, 0.0, 0.0), float(np.nextafter(7.0, 0.0)), False),
    ("r3_ulp_above", _f32(2, 3, 6), (0.0, 0.0, 0.0), float(np.nextafter(7.0, 8.0)), True),
    ("r2_exact", _f32(3, 4, 99), (0.0, 0.0), 5.0, True),
    ("r2_ulp_below", _f32(3, 4, 99), (0.0, 0.0), float(np.nextafter(5.0, 0.0)), False),
    ("r2_ulp_above", _f32(3, 4, 99), (0.0, 0.0), float(np.nextafter(5.0, 6.0)), True),
    ("nan_z_dims2", _f32(3, 4, np.nan), (0.0, 0.0), 5.0, True),                   # only the tested coordinates count
    ("inf_z_dims2", _f32(3, 4, np.inf), (0.0, 0.0), np.inf, True),
    ("nan_z_dims3", _f32(3, 4, np.nan), (0.0, 0.0, 0.0), np.inf, False),
    ("r0_centre2", _f32(1.5, -2.25, 0.5), (1.5, -2.25), 0.0, True),
    ("r0_centre3", _f32(1.5, -2.25, 0.5), (1.5, -2.25, 0.5), 0.0, True),
    ("r0_ulp_off", _f32(_UP, -2.25, 0.5), (1.5, -2.25), 0.0, False),
    ("inf_coord", _f32(np.inf, 0, 0), (0.0, 0.0), np.inf, False),
    ("neg_inf_coord3", _f32(0, 0, -np.inf), (0.0, 0.0, 0.0), np.inf, False),
    ("overflow_r_inf", _f32(3e38, 0, 0), (-1e200, 0.0), np.inf, True),           # d2 = +inf <= rr = +inf
    ("overflow_r_1e200", _f32(3e38, 0, 0), (-1e200, 0.0), 1e200, True),           # rr overflows as well
    ("overflow_r_1e100", _f32(3e38, 0, 0), (-1e200, 0.0), 1e100, False),
    ("neg_zero", _f32(-0.0, -0.0, -0.0), (0.0, 0.0, 0.0), 0.0, True),
    ("denormal_r0", _f32(1e-45, 0, 0), (0.0, 0.0), 0.0, False),                  # (2^-149)^2 > 0 in f64
    ("denormal_exact", _f32(1e-45, 0, 0), (0.0, 0.0), _DEN, True),
    ("denormal_ulp_below", _f32(0, 1e-45, 0), (0.0, 0.0, 0.0), float(np.nextafter(_DEN, 0.0)), False),
)
PRIOR_EDGE_LOCALS = (0, 63, 64, 65, 128)          # the local frame that carries the edge pose, in turn


def prior_scene(span, edge, k):
    """poses of a stamped table of `span` frames for PRIOR_EDGES[k]: local frame PRIOR_EDGE_LOCALS[k % 5] carries the
    edge pose; the others lie on a circle of radius 3 around (10, 10, 10) -> (t f32 [span, 3], edge local frame)"""
    loc = PRIOR_EDGE_LOCALS[k % len(PRIOR_EDGE_LOCALS)]
    ang = np.arange(span) * 0.37
    t = np.stack([10 + 3 * np.cos(ang), 10 + 3 * np.sin(ang), 10 + 0 * ang], 1).astype(np.float32)
    t[loc] = edge[1]
    return t, loc


def pose_rows(t):
    """(n, 12) f32 rows of the 3x4 [I | t]"""
    p = np.zeros((len(t), 12), np.float32)
    p[:, [0, 5, 10]] = 1.0
    p[:, [3, 7, 11]] = t
    return p
