"""Workloads at the structural edges of sgtd_remove_frames (remove_kernels.hip.h; remove_entries and sgtd_remove_frames of
sgtd_accel.hip; multi::remove_frames of multi_impl.hip.h) and a numpy model of its two passes.  Plain helper module of
tests/test_remove_edges.py (CPU: the model equals field[keep] on every workload, the workloads reach the counts they are
for, wrong compactions — the model's switches — are told apart by a named workload) and tests/test_gpu_remove_edges.py
(GPU: every form of a handle, after the removal, holds field[keep] bit for bit and answers as the oracle of the survivors).

A workload is a list of AddSTDescs calls and a list of removal steps.  Entry i (its ORIGINAL insertion index) sits alone
in cell i at cell + DELTA on even cells (so a table can be finalized and queried: one bucket per entry), its label is
twelve bits of a hash of i, and every 32-bit word of angle, center, vertex and node_id is (i, word index, field) folded
into one pattern: a word that lands in the wrong place or comes from another entry, word or field is identifiable.
Two entries in five carry a non-canonical float in one value of angle, center and vertex (NaNs with payloads, negative
denormals): the kernel moves 32-bit words and every comparison is on bit patterns.  A keep pattern over entry indices is
realised with frame ids: STAY for the entries that stay, GO and GO2 for those that leave (one call carries all three,
interleaved).  stats()["n_frames"] counts add calls, so it is asserted only where `per_frame` holds (every call one id,
every frame one call).

Constants restated from the sources:
  TILE 1024, THREADS 256, ROUNDS 4     SGTD_RM_TILE, SGTD_RM_THREADS, SGTD_RM_ROUNDS   remove_kernels.hip.h:16-18
  MASKS 16                             SGTD_RM_MASKS (one 64-bit keep mask per wave and round)   remove_kernels.hip.h:19
  SCAN_BLOCK 2048                      SGTD_SCAN_THREADS x SGTD_SCAN_ITEMS   table_kernels.hip.h:21-22
  LDS_SWITCH 65536 bytes of bitmap     remove_entries, `if (lds <= 65536)`: 524 288 frames   sgtd_accel.hip
  FLAG_GRID 4 x CU count               remove_entries, `e->n_cus * 4`   sgtd_accel.hip
  SHARD_BLOCK 64                       SGTD_SHARD_BLOCK   multi.hip.h

The model's switches (test_remove_edges.py asserts each on the workload named here, and that the plain model equals
field[keep] everywhere):
  low_half_only     rank from v_mbcnt_lo alone                          rank/single_gone
  before_shifted    before[] one mask late (the inclusive sum)          counts/E1025/all_but_first
  wave_major        masks stored wave-major, read round-major           counts/E1024/every_other_round
  ne_1024           the last tile's entries taken as 1024 (pass 1)      counts/E1025/all_but_first
  head_from_entry   head from the entry offset, not the word offset     align/k1_m5   (W = 6 and 3; for 9 and 1 the two agree mod 4)
  tail_dropped      the scalar tail of the output not stored            align/k0_m5
  count_not_reset   the wave counts carried over to the next tile       large
  span_short        the bitmap's span one short: `<` where frame_hi needs `<=`    bitmap/span33/hi
  present_lane0     `present` not set by the first lane of a wave       bitmap/wave_runs
"""
import numpy as np

import _table_edges as te

TILE, THREADS, ROUNDS, WAVE, MASKS, SCAN_BLOCK = 1024, 256, 4, 64, 16, 2048
WAVES = THREADS // WAVE
LDS_SWITCH_BYTES = 65536
LDS_SWITCH_FRAMES = LDS_SWITCH_BYTES * 8            # 524 288: the last span whose bitmap is copied into LDS
CUS_MI355X = 256
FLAG_GRID = 4 * CUS_MI355X
SHARD_BLOCK = 64
FIELDS = (("side", 6), ("angle", 6), ("center", 6), ("vertex", 9), ("label", 3), ("frame", 1), ("node_id", 3))
WIDTH = dict(FIELDS)
NAMES7 = tuple(f for f, _ in FIELDS)
FID = dict(angle=1, center=2, vertex=3, node_id=4)
STAY, GO, GO2 = 7, 4, 9
DELTA = te.DELTA
MUTANTS = ("low_half_only", "before_shifted", "wave_major", "ne_1024", "head_from_entry", "tail_dropped", "count_not_reset",
           "span_short", "present_lane0")


# ---- the fields of entry i -------------------------------------------------------------------------------------------
def _pattern(fid, W, idx):
    i = idx.astype(np.uint32)[:, None]
    k = np.arange(W, dtype=np.uint32)[None, :]
    return (i & np.uint32(0x3FFFFF)) | (k << np.uint32(22)) | (np.uint32(fid) << np.uint32(26)) | (((i * np.uint32(5) + k * np.uint32(3)) & np.uint32(7)) << np.uint32(29))


def _specials(w, fid, idx, n_values):
    """entries i % 5 == 2: value i % n_values is a NaN with i in its payload (inf for a zero payload); i % 5 == 4: value
    (i + 1) % n_values is a negative denormal (float32) or has a negative-denormal high word (float64)"""
    wpv = w.shape[1] // n_values                        # words per value: the high word decides
    low = np.uint32(0x3FFFFF if wpv == 1 else 0xFFFFF)
    expo = np.uint32(0x7F800000 if wpv == 1 else 0x7FF00000)
    i = idx.astype(np.uint32)
    sign = np.uint32(((fid >> 1) & 1) << 31)
    quiet = np.uint32((fid & 1) << (22 if wpv == 1 else 19))
    a = np.flatnonzero(idx % 5 == 2)
    w[a, (idx[a] % n_values) * wpv + wpv - 1] = expo | sign | quiet | (i[a] & low & ~quiet)
    b = np.flatnonzero(idx % 5 == 4)
    w[b, ((idx[b] + 1) % n_values) * wpv + wpv - 1] = np.uint32(0x80000000) | quiet | (i[b] & low & ~quiet)
    return w


def make_fields(idx, frame):
    """the seven fields of the entries with original indices idx (numpy arrays of the dtypes of manager.Descs)"""
    idx = np.asarray(idx, np.int64)
    cell = np.stack([2 * (idx >> 14) + 100, 2 * ((idx >> 7) & 127) + 100, 2 * (idx & 127) + 100], 1)
    h = ((idx * 2654435761) >> 8) & 0xFFF
    out = dict(side=cell + DELTA, label=np.stack([(h >> 8) & 15, (h >> 4) & 15, h & 15], 1).astype(np.int32),
               frame=np.asarray(frame, np.uint32).copy())
    out["angle"] = _specials(_pattern(FID["angle"], 6, idx), FID["angle"], idx, 3).view(np.float64)
    out["center"] = _specials(_pattern(FID["center"], 6, idx), FID["center"], idx, 3).view(np.float64)
    out["vertex"] = _specials(_pattern(FID["vertex"], 9, idx), FID["vertex"], idx, 9).view(np.float32)
    out["node_id"] = _pattern(FID["node_id"], 3, idx).view(np.int32)
    return out


def words(a):
    """a field as its 32-bit words, one row per entry"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32).reshape(len(a), -1)


class FieldCase(te.Case):
    """a _table_edges.Case whose optional fields are given, not derived from the insertion index"""

    def __init__(self, name, fields, bounds=None, **kw):
        E = len(fields["frame"])
        bounds = [(0, E)] if bounds is None else bounds
        te.Case.__init__(self, name, [(fields["side"][a:b], fields["label"][a:b], fields["frame"][a:b]) for a, b in bounds if b > a], **kw)
        self._opt = {k: fields[k] for k in ("angle", "center", "vertex", "node_id")}


# ---- a workload ------------------------------------------------------------------------------------------------------
SMALL_FORMS = ("answered", "unfinalized", "loaded", "view", "add0", "add1", "add1025", "twice", "pending")


class Workload:
    """frame: the frame id of every entry, in insertion order; bounds: the AddSTDescs calls [(lo, hi)]; steps: the removal
    calls, in order (lists of frame ids); cut: the call index at which the `tail` form finalizes first; query: the forms
    that finalize also compare the census and the dump with the oracle of the survivors"""

    def __init__(self, name, frame, steps, bounds=None, cfg=None, query=False, forms=SMALL_FORMS, cut=None, note=None):
        self.name, self.query, self.cut, self.note = name, query, cut, note
        self.frame = np.asarray(frame, np.uint32)
        self.E = len(self.frame)
        self.bounds = [(0, self.E)] if bounds is None else list(bounds)
        self.steps = [[int(x) for x in s] for s in steps]
        self.cfg = dict(cfg or {})
        ids = [set(self.frame[a:b].tolist()) for a, b in self.bounds]
        self.per_frame = all(len(s) == 1 for s in ids) and len(set().union(*ids)) == len(ids)
        first = self.cfg.get("first_frame_id", 0)
        self.stamped = self.per_frame and [min(s) for s in ids] == list(range(first, first + len(ids)))
        forms = tuple(forms) + (("tail",) if cut is not None else ()) + (("multi",) if self.stamped and first == 0 else ())
        self.forms = forms
        self._fields = None
        hi = int(self.frame.max()) if self.E else 0
        self.cfg.setdefault("rough_dis_threshold", te.ROUGH)
        self.cfg.setdefault("max_frame_n", max(te.se.MAX_FRAME_N, hi + 8))

    def fields(self):
        if self._fields is None:
            self._fields = make_fields(np.arange(self.E), self.frame)
        return self._fields

    def keep(self, n_steps=None):
        gone = [x for s in self.steps[:n_steps] for x in s]
        return ~np.isin(self.frame, np.asarray(gone, np.int64).astype(np.uint32)) if gone else np.ones(self.E, bool)

    def descs(self, mod, lo, hi):
        d = mod.Descs(hi - lo)
        for f in NAMES7:
            getattr(d, f)[...] = self.fields()[f][lo:hi]
        return d

    def survivors(self, n_steps=None, extra=None):
        """the fields of what is left after the first n_steps removals (+ extra, the fields of entries added afterwards)"""
        k = self.keep(n_steps)
        out = {f: v[k] for f, v in self.fields().items()}
        if extra is not None:
            out = {f: np.concatenate([out[f], extra[f]]) for f in out}
        return out

    def added(self, n):
        """n entries for a call after the removal: original indices E .., a frame id above every other"""
        return make_fields(np.arange(self.E, self.E + n), np.full(n, int(self.frame.max()) + 1, np.uint32))

    def case(self, n_steps=None, extra=None, tag=""):
        """the survivors as a Case (one AddSTDescs call): what the oracle is given"""
        return FieldCase("%s/survivors%s%s" % (self.name, "" if n_steps is None else n_steps, tag), self.survivors(n_steps, extra),
                         cfg={k: v for k, v in self.cfg.items() if k != "first_frame_id"})

    def n_tiles(self):
        return -(-self.E // TILE)


def from_keep(name, keep, **kw):
    """a table in one call whose entries stay (STAY) or leave (GO, GO2 by a hash of the index: the `twice` form's two calls)"""
    keep = np.asarray(keep, bool)
    i = np.arange(len(keep))
    frame = np.where(keep, STAY, np.where(((i * 7) >> 1) & 1, GO2, GO))
    return Workload(name, frame, [[GO, GO2]], **kw)


def split_steps(steps):
    """every removal call as two (the `twice` form): the ids at even and at odd positions"""
    out = []
    for s in steps:
        out += [s[::2], s[1::2]] if len(s) > 1 else [s]
    return out


# ---- 1. counts -------------------------------------------------------------------------------------------------------
COUNT_E = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)
COUNT_PATTERNS = ("all_but_first", "all_but_last", "only_first", "only_last", "every_other_entry", "every_other_wave", "every_other_round")
COUNT_QUERY_E = (5, 257, 1025, 2049)


def count_keep(E, pattern):
    i = np.arange(E)
    return {"all_but_first": i != 0, "all_but_last": i != E - 1, "only_first": i == 0, "only_last": i == E - 1,
            "every_other_entry": i % 2 == 1, "every_other_wave": (i // WAVE) % 2 == 1, "every_other_round": (i // THREADS) % 2 == 1}[pattern]


def counts():
    return [from_keep("counts/E%d/%s" % (E, p), count_keep(E, p), query=E in COUNT_QUERY_E) for E in COUNT_E for p in COUNT_PATTERNS]


# ---- 2. rank ---------------------------------------------------------------------------------------------------------
RANK_WAVES = ((0, 0), (1, 0), (3, 3))               # (round, wave): the tile's first wave, the first of round 1, the last of round 3
RANK_LANES = (0, 31, 32, 63)
SPLIT_CHUNKS = 5                                    # 65 splits in chunks of 13 tiles


def _wave_at(r, w):
    return r * THREADS + w * WAVE


def rank():
    out = []
    for kind in ("gone", "kept"):
        keep = np.zeros(len(RANK_WAVES) * len(RANK_LANES) * TILE, bool) if kind == "kept" else np.ones(len(RANK_WAVES) * len(RANK_LANES) * TILE, bool)
        t = 0
        for r, w in RANK_WAVES:
            for lane in RANK_LANES:
                keep[t * TILE + _wave_at(r, w) + lane] = kind == "kept"
                t += 1
        out.append(from_keep("rank/single_" + kind, keep, query=kind == "kept"))
    # the split at every lane: tile j of a chunk splits its three waves at s, the lanes below (above) s kept; the other
    # waves keep every other entry, so before[] is not a multiple of 64
    per = 65 // SPLIT_CHUNKS
    for side in ("below", "above"):
        for c in range(SPLIT_CHUNKS):
            keep = (np.arange(per * TILE) % 2 == 0)
            for j in range(per):
                s = c * per + j
                for n, (r, w) in enumerate(RANK_WAVES):
                    sp = s if n != 2 else 64 - s                      # the last wave runs the other way
                    lanes = np.arange(WAVE)
                    at = j * TILE + _wave_at(r, w)
                    keep[at:at + WAVE] = (lanes < sp) if (side == "below") == (n != 1) else (lanes >= sp)
            out.append(from_keep("rank/split_%s_%d" % (side, c), keep))
    return out


def split_of(name, tile, n):
    """the split lane and direction of RANK_WAVES[n] in tile `tile` of workload rank/split_<side>_<c>"""
    side, c = name.split("_")[1], int(name.split("_")[2])
    s = c * (65 // SPLIT_CHUNKS) + tile
    return (s if n != 2 else 64 - s), ((side == "below") == (n != 1))


# ---- 3. tiles --------------------------------------------------------------------------------------------------------
def tiles():
    i = np.arange(3 * TILE)
    t = i // TILE
    out = [from_keep("tiles/middle_empty", t != 1, query=True), from_keep("tiles/first_empty", t != 0),
           from_keep("tiles/one_between", (t != 1) | (i == TILE + 517))]
    i = np.arange(2 * TILE + 300)
    out.append(from_keep("tiles/last_partial_empty", i // TILE != 2))
    return out


# ---- 4. align --------------------------------------------------------------------------------------------------------
ALIGN_K, ALIGN_M = tuple(range(9)), (1, 2, 3, 4, 5)


def align():
    """two tiles: the first keeps k entries (the second tile's output offset), the second keeps m"""
    out = []
    for k in ALIGN_K:
        for m in ALIGN_M:
            keep = np.zeros(2 * TILE, bool)
            keep[(np.arange(k) * 113 + 5) % TILE] = True
            keep[TILE + (np.arange(m) * 211 + 40) % TILE] = True
            out.append(from_keep("align/k%d_m%d" % (k, m), keep, query=(k, m) in ((1, 5), (3, 2))))
    return out


def output_split(tile_off, kept, W):
    """(head, 16-byte vectors, tail) of a tile's output, remove_compact_kernel's arithmetic"""
    kw, d0 = kept * W, tile_off * W
    head = min((4 - (d0 & 3)) & 3, kw)
    nv = (kw - head) >> 2
    return head, nv, kw - head - 4 * nv


# ---- 5. bitmap -------------------------------------------------------------------------------------------------------
SPANS = (1, 31, 32, 33, 64, 65)


def _per_frame(name, ids, sizes, steps, **kw):
    frame = np.repeat(np.asarray(ids, np.int64), sizes)
    b = np.cumsum([0] + list(sizes))
    return Workload(name, frame, steps, bounds=list(zip(b[:-1].tolist(), b[1:].tolist())), **kw)


def bitmap():
    out = []
    for S in SPANS:
        ids = np.arange(40, 40 + S)
        sizes = [(f % 4) + 1 for f in range(S)]
        which = dict(lo=[40], hi=[40 + S - 1], both=[40, 40 + S - 1], hole=[40 + S // 2])
        for k, gone in which.items():
            if (S == 1 and k != "lo") or (S < 3 and k == "hole"):
                continue
            out.append(_per_frame("bitmap/span%d/%s" % (S, k), ids, sizes, [gone], query=S in (1, 33, 65)))
    # runs of one frame that begin on lane 0 of every wave: the frame's bit in `present` comes from that lane alone
    out.append(_per_frame("bitmap/wave_runs", [3, 4, 5, 6, 7], [64, 128, 64, 64, 64], [[3, 7]], query=True))
    # a table far from frame 0: ids below frame_lo, above frame_hi and the largest id remove nothing
    big = 70016
    ids = np.arange(big, big + 35)
    out.append(_per_frame("bitmap/first_large", ids, [(f % 3) + 2 for f in range(35)],
                          [[5, big - 1], [big + 35, 2 ** 32 - 1], [2 ** 32 - 1, big + 4, 0], [big, big + 1, big + 34]],
                          cfg=dict(first_frame_id=big, max_frame_n=big + 100), query=True))
    for hi, tag in ((LDS_SWITCH_FRAMES - 1, "lds_last"), (LDS_SWITCH_FRAMES, "global_first")):
        for end, gone in (("lo", [0]), ("hi", [hi])):
            out.append(_per_frame("bitmap/%s/%s" % (tag, end), [0, hi], [70, 70], [gone], cfg=dict(max_frame_n=hi + 8)))
    return out


# ---- 6. order --------------------------------------------------------------------------------------------------------
def order():
    sizes = [350, 350, 350, 350, 350, 351]
    out = [_per_frame("order/descending", [900, 41, 40, 17, 5, 3], sizes, [[41, 5]], query=True)]
    frame = np.repeat([900, 41, 40, 3, 40, 17], sizes)                # A = 40, B = 3
    b = np.cumsum([0] + sizes).tolist()
    bounds = [(b[0], b[1]), (b[1], b[3])] + [(b[k], b[k + 1]) for k in (3, 4, 5)]
    out.append(Workload("order/aba_remove_a", frame, [[40]], bounds=bounds, query=True))
    out.append(Workload("order/aba_remove_b", frame, [[3]], bounds=bounds, query=True))
    return out


# ---- 7. tail ---------------------------------------------------------------------------------------------------------
TAIL_SIZES = [300, 423, 301, 500, 77, 260, 1, 199]                     # frames 0 .. 7; the calls from `cut` on are the tail


def tail():
    ids = list(range(8))
    return [_per_frame("tail/" + k, ids, TAIL_SIZES, [gone], cut=5, query=True)
            for k, gone in (("main_only", [1, 3]), ("tail_only", [6, 5]), ("both", [0, 2, 5, 7]))]


# ---- 8. stamped (and so sharded) -------------------------------------------------------------------------------------
STAMPED_F = 200


def stamped():
    ids = list(range(STAMPED_F))
    sizes = [(f % 5) + 9 for f in ids]
    which = dict(shard1_all=[f for f in ids if (f // SHARD_BLOCK) % 3 == 1], f63=[63], f64=[64], f63_64=[63, 64], f127_128=[127, 128],
                 mixed=[0, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192, 199])
    return [_per_frame("stamped/" + k, ids, sizes, [gone], query=k in ("shard1_all", "mixed")) for k, gone in which.items()]


# ---- 9. large --------------------------------------------------------------------------------------------------------
LARGE_E = SCAN_BLOCK * TILE + 1


def large_keep(E=LARGE_E):
    """a plain rule that takes another share out of every tile, whole tiles (index 3 mod 7) included; the last tile's one
    entry stays"""
    i = np.arange(E, dtype=np.int64)
    t = i // TILE
    keep = (((i * 2654435761) >> 7) % 1021 >= (t * 389) % 1021) & (t % 7 != 3)
    keep[-1] = True
    return keep


def large():
    """2048 x 1024 + 1 entries: 2049 tiles, the last of one entry — more tiles than the flag kernel's 4 x 256 workgroups
    (a second tile per workgroup) and one scan block of tile counts plus one"""
    return from_keep("large", large_keep(), forms=("unfinalized",))


_ALL = None


def workloads():
    """every small workload, by name"""
    global _ALL
    if _ALL is None:
        ws = counts() + rank() + tiles() + align() + bitmap() + order() + tail() + stamped()
        _ALL = {w.name: w for w in ws}
        assert len(_ALL) == len(ws)
    return _ALL


# ---- the model of the two passes -------------------------------------------------------------------------------------
FILL = np.uint32(0xDEADBEEF)


def _bits_of(ids, lo, span):
    bits = np.zeros((span + 31) // 32, np.uint32)
    for f in ids:
        d = int(f) - lo
        if f >= lo and 0 <= d < span:
            bits[d >> 5] |= np.uint32(1 << (d & 31))
    return bits


def model_flags(frame, gone, grid=FLAG_GRID, mutant=None):
    """pass 1 as remove_flag_kernel does it: workgroup b of `grid` walks the tiles b, b + grid, ..; per tile 4 rounds of 4
    waves, one 64-bit mask each at [round * 4 + wave].  -> (masks [tiles, 16] of uint64, tile counts, present bitmap,
    removed bitmap, lo, span)"""
    frame = np.asarray(frame, np.uint32).astype(np.int64)
    n = len(frame)
    lo, hi = int(frame.min()), int(frame.max())
    span = hi - lo + 1
    bits = _bits_of(gone, lo, span)
    test_span = span - 1 if mutant == "span_short" else span
    n_tiles = -(-n // TILE)
    stays = frame[~np.isin(frame, np.asarray(list(gone), np.int64))]
    padded = np.full(n_tiles * TILE, stays[0] if len(stays) else lo, np.int64)      # what lies behind the table: a frame id that stays
    padded[:n] = frame
    masks = np.zeros((n_tiles, MASKS), np.uint64)
    count = np.zeros(n_tiles, np.int64)
    present = np.zeros_like(bits)
    lanes = np.arange(WAVE)
    for b in range(min(grid, n_tiles)):
        cnt = np.zeros(WAVES, np.int64)
        for t in range(b, n_tiles, grid):
            if mutant != "count_not_reset":
                cnt[:] = 0
            for r in range(ROUNDS):
                for w in range(WAVES):
                    i = t * TILE + r * THREADS + w * WAVE + lanes
                    inn = (i < n) if mutant != "ne_1024" else np.ones(WAVE, bool)
                    d = np.where(inn, padded[i] - lo, 0)
                    inside = inn & (d < test_span)
                    gone_l = inside & (((bits[np.minimum(d, span - 1) >> 5] >> (d & 31).astype(np.uint32)) & 1) == 1)
                    kept = inn & ~gone_l
                    m = np.uint64(0)
                    for l in np.flatnonzero(kept):
                        m |= np.uint64(1) << np.uint64(l)
                    masks[t, (w * ROUNDS + r) if mutant == "wave_major" else (r * WAVES + w)] = m
                    cnt[w] += int(kept.sum())
                    prev = np.concatenate([d[:1], d[:-1]])                  # __shfl_up: lane 0 reads itself
                    first = (prev != d) | ((lanes == 0) & (mutant != "present_lane0"))
                    for x in d[inside & first]:
                        present[x >> 5] |= np.uint32(1 << (x & 31))
            count[t] = cnt.sum()
    return masks, count, present, bits, lo, span


def _popcount64(m):
    return bin(int(m)).count("1")


def model_compact(src_words, masks, tile_off, kept_total, mutant=None):
    """pass 2 as remove_compact_kernel<W> does it, tile by tile: before[] from the masks' popcounts, the rank inside a
    wave from the low and the high half of its mask, the pack, and the output as head / 16-byte vectors / tail.  A 16-byte
    store is modelled at its address rounded down to 16 bytes (the model's convention for a misaligned vector store).
    -> the destination buffer [kept_total * W + slack] of words, FILL where nothing was stored"""
    n, W = src_words.shape
    n_tiles = len(masks)
    dst = np.full((kept_total + TILE) * W + 8, FILL, np.uint32)
    flat = src_words.reshape(-1)
    for t in range(n_tiles):
        e0 = t * TILE
        ne = min(TILE, n - e0)
        pop = [_popcount64(m) for m in masks[t]]
        inc = np.cumsum(pop)
        before = inc if mutant == "before_shifted" else np.concatenate([[0], inc[:-1]])
        total = int(inc[-1])
        lds = np.full(TILE * W, FILL, np.uint32)
        for r in range(ROUNDS):
            for w in range(WAVES):
                mi = r * WAVES + w
                m = int(masks[t, mi])
                m_lo, m_hi = m & 0xFFFFFFFF, m >> 32
                for lane in range(WAVE):
                    if not (m >> lane) & 1:
                        continue
                    j = r * THREADS + w * WAVE + lane
                    mb_lo = bin(m_lo & ((1 << min(lane, 32)) - 1)).count("1")
                    mb_hi = bin(m_hi & ((1 << max(lane - 32, 0)) - 1)).count("1")
                    at = int(before[mi]) + mb_lo + (0 if mutant == "low_half_only" else mb_hi)
                    val = flat[(e0 + j) * W:(e0 + j + 1) * W] if j < ne else np.zeros(W, np.uint32)
                    if at < TILE:
                        lds[at * W:(at + 1) * W] = val
        kw = total * W
        d0 = int(tile_off[t]) * W
        head = min((4 - ((int(tile_off[t]) if mutant == "head_from_entry" else d0) & 3)) & 3, kw)
        nv = (kw - head) >> 2
        dst[d0:d0 + head] = lds[:head]
        for v in range(nv):
            a = (d0 + head + 4 * v) & ~3
            dst[a:a + 4] = lds[head + 4 * v:head + 4 * v + 4]
        if mutant != "tail_dropped":
            dst[d0 + head + 4 * nv:d0 + kw] = lds[head + 4 * nv:kw]
    return dst


def model_remove(fields, gone, grid=FLAG_GRID, mutant=None, names=NAMES7):
    """both passes over the named fields -> ({field: words [kept, W]}, state) where state is (kept, frame_lo, frame_hi,
    frames gone) as remove_entries derives them (frame_lo / frame_hi None when `present` names no survivor)"""
    masks, count, present, bits, lo, span = model_flags(fields["frame"], gone, grid, mutant)
    off = np.concatenate([[0], np.cumsum(count)[:-1]])
    kept = int(off[-1] + count[-1])
    out = {}
    for f in names:
        W = WIDTH[f]
        out[f] = model_compact(words(fields[f]), masks, off, kept, mutant)[:kept * W].reshape(kept, W)
    stay = [32 * w + b for w in range(len(bits)) for b in range(32) if (int(present[w]) & ~int(bits[w])) >> b & 1]
    gone_frames = sum(bin(int(present[w]) & int(bits[w])).count("1") for w in range(len(bits)))
    return out, (kept, lo + stay[0] if stay else None, lo + stay[-1] if stay else None, gone_frames)


def model_fast(src_words, keep, mutant=None):
    """the two passes vectorised for the large workload: only the switches that need many tiles (None, count_not_reset
    with FLAG_GRID workgroups).  -> words [kept', W]"""
    n = len(keep)
    n_tiles = -(-n // TILE)
    count = np.bincount(np.arange(n) // TILE, weights=keep, minlength=n_tiles).astype(np.int64)
    if mutant == "count_not_reset":
        for t in range(FLAG_GRID, n_tiles):
            count[t] += count[t - FLAG_GRID]
    off = np.concatenate([[0], np.cumsum(count)[:-1]])
    true_count = np.bincount(np.arange(n) // TILE, weights=keep, minlength=n_tiles).astype(np.int64)
    W = src_words.shape[1]
    dst = np.full((int(off[-1] + count[-1]) + TILE, W), FILL, np.uint32)
    idx = np.flatnonzero(keep)
    rank = np.arange(len(idx)) - np.repeat(np.concatenate([[0], np.cumsum(true_count)[:-1]]), true_count)
    dst[off[idx // TILE] + rank] = src_words[idx]
    return dst[:int(off[-1] + count[-1])]
