"""Workloads at the edges of the passes over the match records (STDesc.cpp:404-453: votes per frame, the arg-max rounds
that pick candidate_num frames, the ordered match lists), a plain restatement of those passes, and the geometry of
pairs_query_kernel's tiles.  Plain helper module of tests/test_record_edges.py (CPU: the restatement equals the oracle,
every family reaches its edge, mutants of the restatement are caught) and tests/test_gpu_record_edges.py (GPU: every form
of the passes equals the oracle on them).

A case is one handle: table entries (key, frame) in insertion order and a row of queries, each one candidate_selector
call.  Keys are (side, label) pairs that a query descriptor and a table entry share exactly (as _verify_edges.key_of, the
key space extended over the second and third side): the list of query descriptor i is the table entries that share its
key, in insertion order, and a frame's votes are the number of its entries that share a key with the query, counted once
per query descriptor that carries the key.  Entries may be moved off their key's side (`shift`, in units of the
descriptor's threshold along -x): 0.9 gives a match in a lower cell than the key's own, 1 + a few ulps a record the sweep
cannot decide in f32 and resolve_undecided_kernel kills.
"""
import numpy as np

import _select_edges as se

# ---- copies of the kernels' constants (tests/test_record_edges.py compares them with the headers) -----------------
SGTD_PQ_THREADS = 512
SGTD_PQ_WORDS = 4
SGTD_VT_BINS = 4096
SGTD_TOPK_BINS = 8192
SGTD_TOPK_POOL = 1024
SGTD_CAND_HASH = 256
SGTD_MAX_CAND = 64
VOTES_TILE_FRAMES = 36 * 1024          # frames per tile of votes_query_kernel (plan_select)
WAVE = 64
PQ_WAVES = SGTD_PQ_THREADS // WAVE
PQ_TILE_QUADS = PQ_WAVES * SGTD_PQ_WORDS * WAVE
PQ_TILE_RECS = PQ_TILE_QUADS * 4
PQ_DESCS = SGTD_PQ_THREADS

ROUGH = 0.03
N_LABEL = 15 ** 3


def key_sides_labels(keys):
    """(side [n, 3], label [n, 3]) of keys: label triples in 1..15, side triples 3 m apart in every coordinate (the 27
    cells selection probes around one side never reach another's; thresholds stay below 2.5 m)"""
    k = np.asarray(keys, np.int64)
    j = k // N_LABEL
    assert np.all(j < 216)
    label = np.stack([1 + k % 15, 1 + (k // 15) % 15, 1 + (k // 225) % 15], 1).astype(np.int32)
    side = np.stack([4.25 + 3.0 * (j % 6), 30.25 + 3.0 * ((j // 6) % 6), 45.25 + 3.0 * (j // 36)], 1)
    return side, label


def hash_slot(f):
    """the candidates' hash of pairs_query_kernel<false> / block_count_kernel<false, .>"""
    return ((int(f) * 0x9E3779B1) & 0xFFFFFFFF) >> 24


# ---- the restatement of :404-453 ---------------------------------------------------------------------------------
def record_tiles(lengths):
    """per descriptor i with a list of lengths[i] records: (super-block, first quad of the list in the super-block's
    stream of quads) — record j of the list lies in quad pre + j // 4, tile quad // PQ_TILE_QUADS"""
    L = np.asarray(lengths, np.int64)
    sb = np.arange(len(L)) // PQ_DESCS
    quads = (L + 3) >> 2
    pre = np.zeros(len(L), np.int64)
    for b in range(int(sb.max()) + 1 if len(L) else 0):
        m = sb == b
        pre[m] = np.cumsum(quads[m]) - quads[m]
    return sb, pre


def pq_geometry(lengths):
    """what pairs_query_kernel makes of a query's per-descriptor list lengths: per super-block of PQ_DESCS descriptors
    dict(sb0, K (non-empty lists), RQ (quads), n_tiles, starts [n_tiles, PQ_WAVES, SGTD_PQ_WORDS]) — starts[t, w, u]
    is the number the kernel compares with 64 to leave the marks for the search per quad: the lists that start behind
    the wave's first quad r0 = t * PQ_TILE_QUADS + w * SGTD_PQ_WORDS * 64 and at or before quad r0 + 64 (u + 1)"""
    L = np.asarray(lengths, np.int64)
    out = []
    for sb0 in range(0, len(L), PQ_DESCS):
        n = L[sb0:sb0 + PQ_DESCS]
        quads = (n + 3) >> 2
        pre = np.cumsum(quads) - quads
        start = pre[n > 0]
        RQ = int(quads.sum())
        n_tiles = (RQ + PQ_TILE_QUADS - 1) // PQ_TILE_QUADS
        starts = np.zeros((n_tiles, PQ_WAVES, SGTD_PQ_WORDS), np.int64)
        for t in range(n_tiles):
            for w in range(PQ_WAVES):
                r0 = t * PQ_TILE_QUADS + w * SGTD_PQ_WORDS * WAVE
                k0 = int(np.searchsorted(start, r0, side="right")) - 1
                for u in range(SGTD_PQ_WORDS):
                    starts[t, w, u] = int(np.searchsorted(start, r0 + WAVE * (u + 1), side="right")) - (k0 + 1)
        out.append(dict(sb0=sb0, K=int((n > 0).sum()), RQ=RQ, n_tiles=n_tiles, starts=starts))
    return out


MUTANTS = ("tie_high", "floor4", "floor6", "no_zero", "rounds_plus", "rounds_minus", "clip4095", "clip8191",
           "sort_entry", "sort_desc_entry", "tile_reversed", "drop_partial_quad", "dead_kept", "unmasked_offsets")


def ref_passes(rec_q, rec_e, frame, n_desc, candidate_num, max_frame_n, mutant=None, keep=None):
    """:404-453 over the records (descriptor, table entry) in stream order, frame[entry] the entries' frames: the votes
    per frame, the arg-max rounds (first maximum, max_vote >= 5, a picked frame zeroed, at most candidate_num rounds),
    the list offsets and each list in stream order.  keep: a bit mask over the candidates — lists and offsets of the kept
    ones only (sgtd_finish_lists).  mutant: one of MUTANTS (a wrong restatement)"""
    rec_f = frame[rec_e] if len(rec_e) else np.zeros(0, np.uint32)
    votes = np.bincount(rec_f[rec_f < max_frame_n].astype(np.int64), minlength=max_frame_n).astype(np.int64)
    work = votes.copy()
    if mutant == "clip4095":
        work = np.minimum(work, 4095)
    if mutant == "clip8191":
        work = np.minimum(work, 8191)
    floor = {"floor4": 4, "floor6": 6}.get(mutant, 5)
    rounds = candidate_num + {"rounds_plus": 1, "rounds_minus": -1}.get(mutant, 0)
    cf, cv = [], []
    for _ in range(rounds):
        k = int(np.argmax(work)) if mutant != "tie_high" else len(work) - 1 - int(np.argmax(work[::-1]))
        if not (work[k] > 1 and work[k] >= floor):
            break
        cf.append(k)
        cv.append(int(work[k]))
        if mutant != "no_zero":
            work[k] = 0
    # the lists: the records of the candidate's frame in stream order
    lengths = np.bincount(rec_q, minlength=n_desc) if len(rec_q) else np.zeros(n_desc, np.int64)
    sb, pre = record_tiles(lengths)
    first = np.cumsum(lengths) - lengths
    j = np.arange(len(rec_q)) - first[rec_q] if len(rec_q) else np.zeros(0, np.int64)
    tile = sb[rec_q] * (1 << 20) + (pre[rec_q] + j // 4) // PQ_TILE_QUADS if len(rec_q) else j
    live = np.ones(len(rec_q), bool)
    if mutant == "drop_partial_quad":
        live = j < (lengths[rec_q] // 4) * 4
    off, lq, le = [0], [], []
    for s, f in enumerate(cf):
        kept = keep is None or (keep >> s) & 1
        sel = np.nonzero((rec_f == f) & live)[0]
        if mutant == "sort_entry":
            sel = sel[np.argsort(rec_e[sel], kind="stable")]
        if mutant == "sort_desc_entry":
            sel = sel[np.lexsort((rec_e[sel], rec_q[sel]))]
        if mutant == "tile_reversed":
            sel = np.concatenate([sel[tile[sel] == t][::-1] for t in np.unique(tile[sel])]) if len(sel) else sel
        if kept:
            lq.append(rec_q[sel])
            le.append(rec_e[sel])
        off.append(off[-1] + (len(sel) if kept or mutant == "unmasked_offsets" else 0))
    cat = (lambda a, t: np.concatenate(a).astype(t) if a else np.zeros(0, t))
    return dict(votes=votes.astype(np.float64), M=len(rec_e), lengths=lengths, cand_frame=np.array(cf, np.int32),
                cand_votes=np.array(cv, np.int32), cand_off=np.array(off, np.int64), q_idx=cat(lq, np.int32),
                db_entry=cat(le, np.int64))


def masked(exp, keep):
    """the oracle's answer `exp` under sgtd_finish_lists(keep): offsets are the prefix sums over the kept candidates,
    kept lists are the oracle's, nothing for the others"""
    nc = len(exp["cand_frame"])
    n = np.diff(exp["cand_off"])
    kept = np.array([(keep >> s) & 1 for s in range(nc)], bool)
    off = np.concatenate([[0], np.cumsum(np.where(kept, n, 0))]).astype(np.int64)
    idx = [np.arange(exp["cand_off"][s], exp["cand_off"][s + 1]) for s in range(nc) if kept[s]]
    idx = np.concatenate(idx).astype(np.int64) if idx else np.zeros(0, np.int64)
    return dict(exp, cand_off=off, q_idx=exp["q_idx"][idx], db_entry=exp["db_entry"][idx])


def keep_masks(nc):
    """all, none, bit 0 only, the highest candidate only, alternating"""
    full = (1 << nc) - 1
    return {"all": full, "none": 0, "bit0": 1 & full, "highest": (1 << (nc - 1)) if nc else 0,
            "alternating": 0x5555555555555555 & full}


# ---- cases -------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, family, candidate_num=50, max_frame_n=20000):
        self.name, self.family = name, family
        self.cn, self.max_frame_n = candidate_num, max_frame_n
        self.ekey, self.eframe, self.eshift = [], [], []      # table entries in insertion order
        self.calls = []                                       # ends of the AddSTDescs calls (entry counts)
        self.queries = []                                     # key arrays, one candidate_selector call each
        self.tail_at = None          # entries added before a first query (the rest goes to a tail segment)
        self.info = {}
        self._next_key = 0

    # -- building
    def keys(self, n):
        k = np.arange(self._next_key, self._next_key + n)
        self._next_key += n
        return k

    def entries(self, keys, frame, shift=0.0):
        keys = np.asarray(keys, np.int64).reshape(-1)
        self.ekey += keys.tolist()
        self.eframe += np.broadcast_to(np.asarray(frame, np.int64), keys.shape).tolist()
        self.eshift += np.broadcast_to(np.asarray(shift, np.float64), keys.shape).tolist()

    def end_call(self):
        if not self.calls or self.calls[-1] != len(self.ekey):
            self.calls.append(len(self.ekey))

    def frames_by_votes(self, keys, votes, frames, one_call=False):
        """frame frames[k] gets votes[k] entries over `keys` (entry j carries keys[j % len(keys)]): a query that holds
        every key once gives it votes[k] votes; one AddSTDescs call per frame (one_call: one for all)"""
        keys = np.asarray(keys)
        for v, f in zip(votes, frames):
            self.entries(keys[np.arange(v) % len(keys)], f)
            if not one_call:
                self.end_call()
        self.end_call()

    def query(self, keys):
        self.queries.append(np.asarray(keys, np.int64).reshape(-1))

    # -- use
    @property
    def query_frame(self):
        return self.max_frame_n - 1

    @property
    def stamped(self):
        """one call per frame, frame ids 0, 1, 2, ... in order: what a multi-device handle and a tail segment take"""
        self.end_call()
        f = np.asarray(self.eframe)
        lo = 0
        for k, hi in enumerate(self.calls):
            if not np.all(f[lo:hi] == k):
                return False
            lo = hi
        return True

    def entry_arrays(self):
        side, label = key_sides_labels(self.ekey)
        sh = np.asarray(self.eshift)
        if np.any(sh != 0):
            thr = se.norm3(side) * ROUGH
            side = side.copy()
            side[:, 0] = side[:, 0] - thr * sh
        return side, label, np.asarray(self.eframe, np.uint32)

    def _descs(self, mod, side, label, frame):
        d = mod.Descs(len(side))
        d.side[:] = side
        d.label[:] = label
        d.frame[:] = frame
        return d

    def load(self, mgr, mod, lo=0, hi=None):
        """AddSTDescs calls lo .. hi into an STDescManager or an OracleManager"""
        self.end_call()
        side, label, frame = self.entry_arrays()
        ends = [0] + self.calls
        for c in range(lo, len(self.calls) if hi is None else hi):
            a, b = ends[c], ends[c + 1]
            d = self._descs(mod, side[a:b], label[a:b], frame[a:b])
            mgr.add(d) if hasattr(mgr, "add") else mgr.AddSTDescs(d)

    def query_descs(self, mod, k):
        side, label = key_sides_labels(self.queries[k])
        return self._descs(mod, side, label, np.full(len(side), self.query_frame, np.uint32))

    def config(self):
        return dict(candidate_num=self.cn, max_frame_n=self.max_frame_n, rough_dis_threshold=ROUGH)

    def ref_table(self):
        t = se.RefTable()
        t.add(*self.entry_arrays())
        return t

    def ref_records(self, table, k, mutant=None):
        side, label = key_sides_labels(self.queries[k])
        rq, _, re_ = se.ref_rough(table, side, label, self.query_frame, ROUGH,
                                  thr_scale=1.0 + 1e-12 if mutant == "dead_kept" else 1.0)
        return rq, re_

    def ref_answer(self, table, k, mutant=None, keep=None):
        rq, re_ = self.ref_records(table, k, mutant)
        return ref_passes(rq, re_, table.arrays()[1], len(self.queries[k]), self.cn, self.max_frame_n, mutant, keep)


def vote_floor():
    """frames with 4, 5 and 6 votes (query 0: candidates are the frames with 6 and 5); a query for which no frame
    reaches 5 (query 1: n_cand 0, every offset 0, no list); a query with exactly one candidate (query 2)"""
    c = Case("vote_floor", "vote_floor")
    a, b, d = c.keys(8), c.keys(8), c.keys(6)
    for f, (na, nb, nd) in enumerate(((4, 4, 0), (5, 0, 4), (6, 2, 0), (4, 3, 5))):
        c.entries(a[:na], f)
        c.entries(b[:nb], f)
        c.entries(d[:nd], f)
        c.end_call()
    for q in (a, b, d):
        c.query(q)
    return [c]


def cut():
    """per candidate_num cn in 1, 3, 50, 64 five queries over frames of their own: cn - 1, cn and cn + 1 qualifying frames
    (distinct vote counts, not in frame order, beside frames with 4 votes); cn - 2 frames with 7 votes, five tied at 6 and
    two at 5 (more tied at the cut than slots are left: the lowest ids win); cn + 2 frames all tied at 5"""
    out = []
    for cn in (1, 3, 50, 64):
        c = Case("cut/cn%d" % cn, "cut", candidate_num=cn)
        f0 = 0
        for n in (cn - 1, cn, cn + 1):
            k = c.keys(16)
            votes = [5 + (i * 11) % n for i in range(n)] + [4, 4]
            c.frames_by_votes(k, votes, range(f0, f0 + len(votes)))
            f0 += len(votes)
            c.query(k)
        k = c.keys(16)
        votes = [5, 6, 6] + [7] * max(cn - 2, 0) + [6, 5, 6, 6]
        c.frames_by_votes(k, votes, range(f0, f0 + len(votes)))
        f0 += len(votes)
        c.query(k)
        k = c.keys(16)
        c.frames_by_votes(k, [5] * (cn + 2), range(f0, f0 + cn + 2))
        c.query(k)
        out.append(c)
    return out


def pool():
    """1023, 1024 and 1025 frames at or above the threshold of the top-k (SGTD_TOPK_POOL = 1024: the pool path takes up to
    1024, the general path more), the tie at 5 votes and at 7 (with frames of 5 and 6 votes below it); three frames
    strictly above the tie at the highest, a middle and a low frame id"""
    out = []
    for tie in (5, 7):
        for n in (SGTD_TOPK_POOL - 1, SGTD_TOPK_POOL, SGTD_TOPK_POOL + 1):
            c = Case("pool/tie%d/n%d" % (tie, n), "pool")
            k = c.keys(8)
            votes = np.full(n, tie)
            votes[[n - 1, n // 2, 3]] = [tie + 3, tie + 1, tie + 2]
            if tie > 5:
                votes = np.concatenate([votes, [5, 6, 6, 5, 4]])
            c.frames_by_votes(k, votes.tolist(), range(len(votes)))
            c.query(k)
            c.info = dict(tie=tie, n=n)
            out.append(c)
    return out


def _frame_64(c, ka, kb, v, f):
    """v votes from v // 64 entries of key ka (64 query descriptors carry it) and v % 64 of key kb (one does)"""
    c.entries(np.full(v // 64, ka), f)
    c.entries(np.full(v % 64, kb), f)
    c.end_call()


def bins():
    """vote counts around the last bin of both threshold searches: 4094 .. 4097 (SGTD_VT_BINS) and 8190 .. 8195
    (SGTD_TOPK_BINS), the votes rising with the frame id (a search that clips them sees ties and picks the lowest id), at
    candidate_num 50 and at 3 (the cut inside the clipped bin: five frames at or beyond 8191 and nine at or beyond 4095, true counts different); the third largest
    count at 63, 64, 127 and 128 with candidate_num 3 (the lane boundaries of the suffix search: 64 bins per lane in
    votes_topk_kernel, 128 in topk_kernel)"""
    out = []
    for cn in (50, 3):
        c = Case("bins/clip/cn%d" % cn, "bins", candidate_num=cn)
        ka, kb = c.keys(2)
        for f, v in enumerate((4094, 4095, 4096, 4097, 8190, 8191, 8192, 8193, 8195, 8194)):
            _frame_64(c, ka, kb, v, f)
        c.query([ka] * 64 + [kb])
        out.append(c)
    for third in (63, 64, 127, 128):
        c = Case("bins/lane%d" % third, "bins", candidate_num=3)
        ka, kb = c.keys(2)
        for f, v in enumerate((third - 1, 150, third, 5, third - 2, 200, 4)):
            _frame_64(c, ka, kb, v, f)
        c.query([ka] * 64 + [kb])
        c.info = dict(third=third)
        out.append(c)
    return out


def _collision(lo, hi):
    """two frame ids in [lo, hi) with the same slot in the candidates' hash"""
    seen = {}
    for f in range(lo, hi):
        h = hash_slot(f)
        if h in seen:
            return seen[h], f
        seen[h] = f
    raise AssertionError


def span():
    """caller-stamped frame ids from frame_lo = 1000, candidates at local frame 0 and at span - 1, span % 16 in 0, 1, 15:
    the same content narrow (spans 160, 161, 175: the votes in LDS) and wide (spans 140000, 140001, 140015 with
    max_frame_n 200000: votes outside LDS, topk_kernel, cand_prefix_kernel, the candidates' hash).  The wide builds also
    hold two candidate frames with the same hash slot and candidates at local frames 36863 and 36864.  (One query is
    too small a batch for the tiled votes_query_kernel: the wide builds run votes_kernel<false>; the tile edge is the
    spread keypoint maps')"""
    out = []
    lo = 1000
    for wide in (False, True):
        for rem in (0, 1, 15):
            n = (140000 if wide else 160) + rem
            c = Case("span/%s/rem%d" % ("wide" if wide else "narrow", rem), "span", max_frame_n=200000 if wide else 20000)
            k = c.keys(8)
            frames = [lo + n // 2, lo, lo + 7, lo + n - 1, lo + 20]
            votes = [5, 6, 4, 7, 5]
            if wide:
                a, b = _collision(lo + 50000, lo + 60000)
                frames += [a, b, lo + VOTES_TILE_FRAMES - 1, lo + VOTES_TILE_FRAMES]
                votes += [8, 6, 9, 5]
                c.info["collide"] = (a, b)
            order = np.argsort(frames)           # (insertion in frame order: ids are caller-stamped, not out of order)
            c.frames_by_votes(k, [votes[i] for i in order], [frames[i] for i in order])
            c.query(k)
            c.info.update(lo=lo, span=n)
            out.append(c)
    return out


def _lists_case(name, lengths, n_frames=6, family="lists", cn=50, order=None):
    """one query of len(lengths) descriptors with keys of their own; list i has lengths[i] entries, entry j in frame
    (i + j) % n_frames; inside a frame the entries of the later descriptors come first (stream order is not entry
    order).  order: the frames' insertion order (None: by id, one call per frame)"""
    c = Case(name, family, candidate_num=cn)
    L = np.asarray(lengths, np.int64)
    k = c.keys(len(L))
    i = np.repeat(np.arange(len(L)), L)
    j = np.arange(len(i)) - np.repeat(np.cumsum(L) - L, L)
    f = (i + j) % n_frames
    for fr in (range(n_frames) if order is None else order):
        m = np.nonzero(f == fr)[0]
        m = m[np.lexsort((j[m], -i[m]))]
        c.entries(k[i[m]], fr)
        c.end_call()
    c.query(k)
    c.info["lengths"] = L
    return c


def _ragged_lengths(nd):
    """lengths 1 .. 9 (every n % 4), empty lists at the front, in between and at the end"""
    i = np.arange(nd)
    return np.where((i < 2) | (i % 7 == 3) | (i >= nd - 2), 0, 1 + (i * 5) % 9)


def lists():
    """the geometry of pairs_query_kernel (super-blocks of 512 descriptors, tiles of 2048 quads = 8192 records, 8 waves x
    4 quad-words of 64 quads): queries of 511, 512, 513, 1024, 1025 descriptors with lengths of every n % 4 and empty lists
    at the front, in between and at the end; 1537 descriptors with a whole super-block of empty lists in the middle;
    super-blocks of 2047, 2048, 2049 and 4097 quads; one list of 25001 records (a wave's share and three tiles start in
    mid-list); 512 lists of 1 .. 4 records (64 starts per quad-word: the search per quad); a wave that sees exactly 63, 64
    and 65 starts"""
    out = []
    for nd in (511, 512, 513, 1024, 1025):
        out.append(_lists_case("lists/nd%d" % nd, _ragged_lengths(nd)))
    L = _ragged_lengths(1537)
    L[512:1024] = 0
    out.append(_lists_case("lists/empty_block", L))
    for rq in (2047, 2048, 2049, 4097):
        per = 4 if rq < 4000 else 8
        q = np.full(512, per)
        q[300] += rq - int(q.sum())
        L = 4 * q - (np.arange(512) % 4)                  # (quads kept, n % 4 over 0 .. 3)
        out.append(_lists_case("lists/rq%d" % rq, L))
    out.append(_lists_case("lists/long", [3, 25001, 6]))
    out.append(_lists_case("lists/short", 1 + np.arange(512) % 4))
    for n in (63, 64, 65):
        # list 0 ends so that n lists of one quad start in quads (0, 256] of wave 0, the last of them at quad 256 with
        # two quads; long lists behind
        q = np.array([257 - n] + [1] * (n - 1) + [2] + [300, 300, 5])
        L = 4 * q - (np.arange(len(q)) % 3)
        c = _lists_case("lists/starts%d" % n, L)
        c.info["starts"] = n
        out.append(c)
    return out


def mix():
    """candidate and other records interleaved, candidate_num 64 and 64 candidates (query 0): descriptor 0's list is 8192
    records of 2048 frames of 4 votes (tile 0: no candidate record); descriptor 1's is 8192 records of one candidate
    (tile 1); descriptors 2 .. 40 each match 1 .. 3 entries of every one of the 64 candidates and one entry each of 40
    other frames (tile 2 spreads over all slots, slot 63 among them; equal-slot records from different descriptors and
    waves); descriptor 41 matches, in the first 8 candidates, one entry in its key's cell, two entries 0.9 thresholds away
    in the cell below, inserted BEHIND it (stream order (i, cell, j) is not (i, entry) order), and seven entries 1 .. 5
    ulps, 1e-15 and 1e-14 beyond the threshold (dead records inside candidate frames' lists)"""
    c = Case("mix", "mix", candidate_num=64)
    k = c.keys(42)
    n_low, n_other = 2048, 40
    cands = list(range(n_low, n_low + 64))
    others = list(range(n_low + 64, n_low + 64 + n_other))
    beyond = [1.0 + u * 2.0 ** -52 for u in range(1, 6)] + [1.0 + 1e-15, 1.0 + 1e-14]
    for f in range(n_low):
        c.entries(np.full(4, k[0]), f)
        c.end_call()
    for s, f in enumerate(cands):
        if s == 0:
            c.entries(np.full(PQ_TILE_RECS, k[1]), f)
        for d in range(40, 1, -1):
            c.entries(np.full(1 + (d + s) % 3, k[d]), f)
        if s < 8:
            c.entries([k[41]], f)
            c.entries([k[41]] * 2, f, shift=0.9)
            c.entries([k[41]] * len(beyond), f, shift=beyond)
        c.end_call()
    for f in others:
        c.entries(k[2:41], f)
        c.end_call()
    c.query(k)
    c.info = dict(n_dead=8 * len(beyond), cands=cands)
    return [c]


def ids():
    """frame ids out of insertion order (IdMap::by_frame); a tail segment (query once, then append); a largest frame of
    2^13, 2^13 + 1, 2^16 and 2^17 entries (13, 14, 16 and 17 bits of in-frame rank), the matched entries at its end, at
    candidate_num 50 and 64 — by the launch code candidate_num 64 with 17 rank bits takes the block form (select_form 0)"""
    out = []
    out.append(_lists_case("ids/by_frame", _ragged_lengths(513), family="ids", order=[5, 3, 4, 0, 2, 1]))
    c = _lists_case("ids/tail", _ragged_lengths(513), family="ids")
    c.tail_at = 3
    out.append(c)
    for cn in (50, 64):
        for n, bits in ((1 << 13, 13), ((1 << 13) + 1, 14), (1 << 16, 16), (1 << 17, 17)):
            c = Case("ids/big%d/cn%d" % (n, cn), "ids", candidate_num=cn)
            k = c.keys(9)
            c.frames_by_votes(k[:8], [6, 5], [0, 1])
            c.entries(np.full(n - 7, k[8]), 2)          # (a key no query carries)
            c.entries(k[:7], 2)
            c.end_call()
            c.frames_by_votes(k[:8], [8], [3])
            c.query(k[:8])
            c.info = dict(bits=bits, big=n)
            out.append(c)
    return out


def stale():
    """three queries in a row on one handle: 40 candidates with lists of 60 .. 99 records, then a query no frame reaches
    5 votes for, then three candidates in other frames: nothing of the first call (slot_of, votes, pair_off, the pair
    buffer) may show in the later answers"""
    c = Case("stale", "stale")
    a, b, d = c.keys(100), c.keys(8), c.keys(8)
    for f in range(40):
        c.entries(a[:60 + f], f)
        c.entries(b[:(f % 5)], f)
        c.end_call()
    for f in range(40, 43):
        c.entries(d[:5 + (f - 40)], f)
        c.entries(b[:4], f)
        c.end_call()
    for q in (a, b, d):
        c.query(q)
    return [c]


FAMILIES = (vote_floor, cut, pool, bins, span, lists, mix, ids, stale)


def cases(families=None):
    out = []
    for fam in FAMILIES:
        if families is None or fam.__name__ in families:
            out += fam()
    return out


# ---- keypoint workloads (query_frames / loop_frames take keypoints: edges are made from frames) ------------------
def dup_frames(synth, n_kp=24, seed=5):
    """a map with groups of bit-identical small frames (exact vote ties across frames): one group of 1030 members (more
    than SGTD_TOPK_POOL: the general path), groups of 49, 50, 51 and 3 members (around candidate_num 50; the synthetic
    map's later frames resemble each other, so the last groups tie with one another); the queries are
    the groups' frames themselves and one frame of another stream -> (xyz [F, n_kp, 3], label [F, n_kp], group of every
    frame, query xyz, query label)"""
    sizes = (SGTD_TOPK_POOL + 6, 49, 50, 51, 3)
    base = synth.make_map(len(sizes) + 1, n_kp, stream=seed)
    group = np.repeat(np.arange(len(sizes)), sizes)
    rng = np.random.default_rng(seed)
    group = group[rng.permutation(len(group))]
    return base.xyz[group].copy(), base.label[group].copy(), group, base.xyz.copy(), base.label.copy()


def tiny(seed=2, n_map=48, n_query=16):
    """hand-placed frames of 3 .. 6 keypoints: subsets of 14 points within 18 m of each other, for descriptor_near_num 3
    (a frame with fewer keypoints than descriptor_near_num builds nothing): 1 .. 6 descriptors per frame, so the votes
    hover around 5.  The queries are the first map frames again: their own frame gets as many votes as they have
    descriptors — 4, 5 and 6 occur, most queries have n_cand == 0 -> (xyz [total, 3], label [total], kp_off) of the map
    and of the queries"""
    rng = np.random.default_rng(seed)
    pts = (rng.random((14, 3)) * np.array([18, 18, 4])).astype(np.float32)
    lab = rng.integers(1, 6, 14).astype(np.uint32)
    sizes = np.tile([3, 4, 5, 6], n_map // 4)
    idx = [rng.choice(14, k, replace=False) for k in sizes]
    xyz, label = np.concatenate([pts[i] for i in idx]), np.concatenate([lab[i] for i in idx])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return (xyz, label, off), (xyz[:off[n_query]].copy(), label[:off[n_query]].copy(), off[:n_query + 1].copy())


TINY_CONFIG = dict(descriptor_near_num=3)
