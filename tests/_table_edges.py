"""Workloads at the structural edges of the hash-table build (AddSTDescs, STDesc.cpp:149-172, as build_idmap /
build_segment of sgtd_accel.hip build it) and a plain restatement of the structure sgtd_table_dump shows.  Plain helper
module of tests/test_table_edges.py (CPU: the restatement equals the oracle, the workloads reach the counts they are
for, mutants of the restatement fail) and tests/test_gpu_table_edges.py (GPU: every form in which a table comes to exist
equals the oracle on them).

A workload (Case) is a list of AddSTDescs calls with caller-stamped frames; the optional fields of every entry are
distinct bit patterns of its insertion index.  Cells are even numbers and every side sits at cell + DELTA (unless a
workload says otherwise), so the 27 cells a census descriptor probes hold its own bucket only; rough_dis_threshold is
0.01.  The census of a table is one query descriptor per bucket at the sides and label of the bucket's first entry.

Constants restated from the sources (the reach assertions of test_table_edges.py are written against them):
  RS_ROUND 256, RS_TILE 4096   SGTD_RS_THREADS, SGTD_RS_TILE   table_kernels.hip.h:123-125
  SCAN_BLOCK 2048              SGTD_SCAN_THREADS x SGTD_SCAN_ITEMS   table_kernels.hip.h:21-22
  RUN_MAX 48                   SGTD_RUN_MAX   table_kernels.hip.h:290
  HASH_MIN 1024                build_segment, `u32 cap = 1024; while (cap < 2ull * U)`   sgtd_accel.hip
  BLOCK_MAX 4 MiB              copy_in, `bo.total <= (4u << 20)`   sgtd_accel.hip
  RANK_BITS 13                 build_idmap   sgtd_accel.hip
  REMOVE_TILE 1024             remove_kernels.hip.h
"""
import numpy as np

import _select_edges as se
from _select_edges import RefTable, label_code, ref_rough  # noqa: F401  (the restatement's pieces, not written again)

ROUGH = 0.01
RS_ROUND, RS_TILE, SCAN_BLOCK, RUN_MAX, HASH_MIN, BLOCK_MAX, RANK_BITS, REMOVE_TILE = 256, 4096, 2048, 48, 1024, 4 << 20, 13, 1024
SCAN_DEEP_E = SCAN_BLOCK * SCAN_BLOCK + 1      # device_scan recurses a second time: more than 2048 block sums
DELTA = np.array([0.125, 0.125, 0.125])
CENSUS_MAX = 8192
WAVES_MI355X = 256 * 8 * 4                      # slice_partition_kernel's launch on 256 CUs: n_cus * 8 workgroups of 4 waves
BIG_FORMS = ("one_call", "tail", "loaded")
ALL_FORMS = ("one_call", "per_frame", "tail", "tail_moved", "tail_merged", "aged_tail", "loaded", "removed", "multi", "view")


# ---- the restatement ---------------------------------------------------------------------------------------------
def hash_key(k):
    """hash_key of common.hip.h (u32 arithmetic).  Used ONLY to construct keys that collide, never to predict an output"""
    k = np.asarray(k, np.uint64)
    M = np.uint64(0xFFFFFFFF)
    lo, hi = k & M, k >> np.uint64(32)
    h = ((lo * np.uint64(0x9E3779B1)) & M) ^ ((hi * np.uint64(0x85EBCA77)) & M)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & M
    h ^= h >> np.uint64(12)
    return h


def pack_key(code, x, y, z):
    f = (lambda v: np.asarray(v).astype(np.uint64))
    return (f(code) << np.uint64(48)) | (f(x) << np.uint64(32)) | (f(y) << np.uint64(16)) | f(z)


def desc_block_total(n):
    """desc_block_offsets(n).total of table_kernels.hip.h: the seven fields, each padded to 16 bytes"""
    return sum((n * b + 15) & ~15 for b in (24, 24, 24, 36, 12, 4, 12))


def structure_loop(side, label, frame):
    """what sgtd_table_dump shows, from AddSTDescs as the reference runs it: keys (x, y, z, code) ascending by
    (code, x, y, z), bucket_off, entry ids with every bucket in insertion order.  Python integers, one entry at a time"""
    t = RefTable()
    t.add(side, label, frame)
    order = sorted(t.buckets)                       # (code, x, y, z)
    keys = np.array([[k[1], k[2], k[3], k[0]] for k in order], np.int64).reshape(-1, 4)
    off, ids = [0], []
    for k in order:
        ids += t.buckets[k]
        off.append(len(ids))
    return keys, np.array(off, np.int64), np.array(ids, np.int64)


def key_fields(side, label):
    """(code, x, y, z) per entry, vectorised: (int)(s + 0.5) is C truncation"""
    cell = np.trunc(np.asarray(side, np.float64) + 0.5).astype(np.int64)
    lab = np.asarray(label, np.int64) & 15
    return (lab[:, 0] << 8) | (lab[:, 1] << 4) | lab[:, 2], cell[:, 0], cell[:, 1], cell[:, 2]


def structure_vec(side, label, frame, mutant=None):
    """the same by one stable lexicographic sort of the four key fields (np.lexsort is stable).  mutant: a wrong build —
    "unstable" (buckets not in insertion order), "tile_drop" (the last element of every 4096-tile lost), "low48" (the
    key compared on its low 48 bits: the label code ignored), "heads_shifted" (bucket heads from the flags shifted by one)"""
    code, x, y, z = key_fields(side, label)
    g = np.arange(len(code), dtype=np.int64)
    if mutant == "tile_drop":
        keep = (g % RS_TILE) != RS_TILE - 1
        code, x, y, z, g = code[keep], x[keep], y[keep], z[keep], g[keep]
    if mutant == "low48":
        code = np.zeros_like(code)
    if len(g) == 0:
        return np.zeros((0, 4), np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64)
    tie = -g if mutant == "unstable" else g
    order = np.lexsort((tie, z, y, x, code))
    k = np.stack([x, y, z, code], 1)[order]
    head = np.ones(len(order), bool)
    head[1:] = np.any(k[1:] != k[:-1], axis=1)
    if mutant == "heads_shifted":
        head = np.concatenate([[True], head[:-1]])
    at = np.flatnonzero(head)
    return k[at], np.concatenate([at, [len(order)]]).astype(np.int64), g[order]


def rank_bits(frame, before=None):
    """the rank bits build_idmap chooses for a table of these frame ids (None: refused); before: the bits of the build
    before this one, which are kept while they still do"""
    frame = np.asarray(frame, np.int64)
    if len(frame) == 0:
        return before or RANK_BITS
    longest = int(np.unique(frame, return_counts=True)[1].max())
    span = int(frame.max() - frame.min()) + 1
    need = 1
    while need < 32 and (1 << need) < longest:
        need += 1
    fits = (lambda b: b < 32 and span < (1 << (32 - b)) - 1)
    bits = before or RANK_BITS
    if bits < need or not fits(bits):
        bits = max(need, RANK_BITS)
        if not fits(bits):
            bits = need
        if not fits(bits):
            return None
    return bits


def ids_round_trip(frame, bits):
    """every entry's 32-bit id (local frame << bits | rank inside the frame, in insertion order) decoded back to its
    insertion index, in u32 arithmetic as the device does it; the identity for the bits rank_bits chooses"""
    frame = np.asarray(frame, np.int64)
    lo = int(frame.min())
    order = np.argsort(frame, kind="stable")                 # by_frame
    f_sorted = frame[order] - lo
    first = np.zeros(int(f_sorted.max()) + 1, np.int64)
    heads = np.flatnonzero(np.concatenate([[True], f_sorted[1:] != f_sorted[:-1]]))
    first[f_sorted[heads]] = heads
    rank = np.arange(len(frame)) - first[f_sorted]
    ident = ((f_sorted << bits) | rank) & 0xFFFFFFFF
    back_f, back_r = ident >> bits, ident & ((1 << bits) - 1)
    pos = first[np.minimum(back_f, len(first) - 1)] + back_r
    out = np.full(len(frame), -1, np.int64)
    ok = pos < len(frame)
    out[order[ok]] = order[pos[ok]]
    return out


# ---- a workload --------------------------------------------------------------------------------------------------
class Case:
    """calls: [(side, label, frame[, bare])] — bare: the call passes every optional field as NULL.  cut: the calls before
    it are the table that is finalized first, the rest is appended (the tail forms, loaded).  extra: query descriptors
    (side, label) added to the census.  census: False for a dump-only workload"""

    def __init__(self, name, calls, cut=None, forms=ALL_FORMS, cfg=None, extra=(), census=True):
        self.name, self.cut, self.cfg, self.census_on = name, cut, dict(cfg or {}), census
        self.calls = []
        for c in calls:
            s = np.asarray(c[0], np.float64).reshape(-1, 3)
            l = np.broadcast_to(np.asarray(c[1], np.int32).reshape(-1, 3), s.shape).copy()
            f = np.broadcast_to(np.asarray(c[2], np.uint32).reshape(-1), s.shape[:1]).copy()
            self.calls.append((s, l, f, bool(c[3]) if len(c) > 3 else False))
        self.extra = [(np.asarray(s, np.float64), np.asarray(l, np.int32)) for s, l in extra]
        cat = (lambda k, w, t: np.concatenate([c[k] for c in self.calls]) if self.calls else np.zeros((0,) + w, t))
        self.side, self.label, self.frame = cat(0, (3,), np.float64), cat(1, (3,), np.int32), cat(2, (), np.uint32)
        self.E = len(self.frame)
        self.bare = np.concatenate([np.full(len(c[2]), c[3]) for c in self.calls]) if self.calls else np.zeros(0, bool)
        self.stamped = all(len(set(c[2].tolist())) == 1 for c in self.calls) and \
            [int(c[2][0]) for c in self.calls] == list(range(len(self.calls))) and not self.bare.any()
        self.monotone = bool(np.all(np.diff(self.frame.astype(np.int64)) >= 0))
        forms = [f for f in forms if not (f == "multi" and not self.stamped)]
        if cut is None:
            forms = [f for f in forms if f not in ("tail", "tail_moved", "tail_merged", "aged_tail", "loaded")]
        self.forms = tuple(forms)
        hi = int(self.frame.max()) if self.E else 0
        self.qframe = se.QUERY_FRAME if hi < se.QUERY_FRAME else hi + 1
        self.cfg.setdefault("rough_dis_threshold", ROUGH)
        self.cfg.setdefault("max_frame_n", max(se.MAX_FRAME_N, self.qframe + 2))
        self._s = self._opt = None

    # the optional fields: distinct bit patterns of the insertion index (zeros for a bare call)
    def optional(self):
        if self._opt is None:
            self._opt = self._optional()
        return self._opt

    def _optional(self):
        g = np.arange(self.E, dtype=np.float64)[:, None]
        live = ~self.bare[:, None]
        angle = np.where(live, g * 3 + np.arange(3) + 0.25, 0.0)
        center = np.where(live, -(g * 3 + np.arange(3) + 0.5), 0.0)          # (+0.0 for a bare call: a memset, not -0.0)
        vertex = np.where(live, g * 9 + np.arange(9) + 0.125, 0.0).astype(np.float32)
        node = ((np.arange(self.E)[:, None] * 3 + np.arange(3) + 1) * live).astype(np.int32)
        return dict(angle=angle, center=center, vertex=vertex, node_id=node)

    def descs(self, mod, lo, hi, null_bare=False):
        """entries [lo, hi) as one AddSTDescs argument (null_bare: a bare range passes NULL optional fields)"""
        d = mod.Descs(hi - lo)
        d.side[:], d.label[:], d.frame[:] = self.side[lo:hi], self.label[lo:hi], self.frame[lo:hi]
        if hi > lo and self.bare[lo:hi].all():
            if null_bare:
                d.angle = d.center = d.vertex = d.node_id = None
            return d
        for k, v in self.optional().items():
            getattr(d, k)[:] = v[lo:hi]
        return d

    def call_bounds(self):
        b = np.cumsum([0] + [len(c[2]) for c in self.calls])
        return list(zip(b[:-1].tolist(), b[1:].tolist()))

    def run_bounds(self, lo=0, hi=None):
        """maximal runs of one frame id and one kind of call: the per_frame form's calls"""
        hi = self.E if hi is None else hi
        if hi <= lo:
            return []
        f, b = self.frame[lo:hi].astype(np.int64), self.bare[lo:hi]
        cutp = np.flatnonzero((f[1:] != f[:-1]) | (b[1:] != b[:-1])) + 1 + lo
        edges = [lo] + cutp.tolist() + [hi]
        return list(zip(edges[:-1], edges[1:]))

    def cut_entry(self):
        return self.call_bounds()[self.cut][0] if self.cut is not None and self.cut < len(self.calls) else self.E

    def expected_tail(self, tail_max=None):
        """stats()["tail_entries"] after the calls from `cut` on were appended to the finalized first part (do_finalize's
        can_tail): 0 where the append has to rebuild"""
        c = self.cut_entry()
        n = self.E - c
        if n == 0 or c == 0:
            return 0
        limit = tail_max if tail_max else max(262144, c // 8)
        b0 = rank_bits(self.frame[:c])
        ok = (self.monotone and n <= limit and rank_bits(self.frame, b0) == b0
              and int(self.frame[c:].min()) > int(self.frame[:c].max()))
        return n if ok else 0

    def structure(self):
        if self._s is None:
            self._s = structure_vec(self.side, self.label, self.frame)
        return self._s

    def census(self):
        """[(side, label)] of at most CENSUS_MAX descriptors each: one per bucket at its first entry's sides and label
        (+ the extra descriptors); more than CENSUS_MAX buckets: the first and the last CENSUS_MAX"""
        keys, off, ids = self.structure()
        if not self.census_on or len(keys) == 0:
            return []
        first = ids[off[:-1]]
        parts = [first] if len(first) <= CENSUS_MAX else [first[:CENSUS_MAX], first[-CENSUS_MAX:]]
        out = []
        for k, p in enumerate(parts):
            s, l = self.side[p], self.label[p]
            if k == 0 and self.extra:
                s = np.concatenate([s] + [e[0].reshape(-1, 3) for e in self.extra])
                l = np.concatenate([l] + [e[1].reshape(-1, 3) for e in self.extra])
            out.append((s, l))
        return out

    def query_descs(self, mod, k):
        s, l = self.census()[k]
        d = mod.Descs(len(s))
        d.side[:], d.label[:], d.frame[:] = s, l, self.qframe
        return d

    def free_frames(self, n=3):
        """n frame ids the workload does not use, inside its span where there is room (the decoys of the removed form)"""
        used, out, f = set(self.frame.tolist()), [], int(self.frame.min())
        while len(out) < n:
            if f not in used:
                out.append(f)
            f += 1
        return out

    def n_frames(self):
        return len(set(self.frame.tolist()))


# ---- building blocks ---------------------------------------------------------------------------------------------
def key_pool(rng, n, label=None):
    """n distinct keys (cell x, y, z even, label triple) spread over all seven key bytes that can vary and the code's
    high nibble"""
    cells = (rng.integers(0, 32767, (4 * n + 8, 3)) * 2).astype(np.int64)
    labs = rng.integers(0, 16, (4 * n + 8, 3)).astype(np.int32) if label is None else np.tile(np.asarray(label, np.int32), (4 * n + 8, 1))
    _, keep = np.unique(np.concatenate([cells, labs], 1), axis=0, return_index=True)
    keep = np.sort(keep)[:n]
    return cells[keep], labs[keep]


def spread_frames(n, n_frames, first=0):
    """n entries over n_frames frames, monotone and contiguous"""
    return (first + np.arange(n, dtype=np.int64) * n_frames // max(n, 1)).astype(np.uint32)


def per_frame_calls(side, label, frame):
    f = np.asarray(frame, np.int64)
    edges = [0] + (np.flatnonzero(f[1:] != f[:-1]) + 1).tolist() + [len(f)]
    return [(side[a:b], label[a:b], frame[a:b]) for a, b in zip(edges[:-1], edges[1:]) if b > a]


def pooled(name, E, seed, n_frames=5, per_key=12, pins=(), **kw):
    """E entries drawn from a pool of about E / per_key keys; pins: ((i, j), pool index) forces entries i and j onto one key"""
    rng = np.random.default_rng(seed)
    K = max(1, E // per_key)
    cells, labs = key_pool(rng, K)
    pick = rng.integers(0, K, E)
    for k, (i, j) in enumerate(pins):
        if j < E:
            pick[i] = pick[j] = k % K
    side = cells[pick] + DELTA
    frame = spread_frames(E, min(n_frames, E))
    calls = per_frame_calls(side, labs[pick], frame)
    kw.setdefault("cut", max(1, len(calls) - 1) if len(calls) > 1 else None)
    return Case(name, calls, **kw)


# ---- 1. sort_counts ----------------------------------------------------------------------------------------------
SORT_E = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193)


def sort_counts(E):
    return pooled("sort_counts/E%d" % E, E, 100 + E, pins=((RS_ROUND - 1, RS_ROUND), (RS_TILE - 1, RS_TILE)))


def radix_passes(case):
    """the key order after each 8-bit pass of a stable LSD sort (skipped passes left out): [(byte, keys in that order)]"""
    code, x, y, z = key_fields(case.side, case.label)
    k = pack_key(code, x, y, z)
    out = []
    for b in range(8):
        d = (k >> np.uint64(8 * b)) & np.uint64(255)
        if len(k) and np.all(d == d[0]):
            continue
        k = k[np.argsort(d, kind="stable")]
        out.append((b, k.copy()))
    return out


# ---- 2. digit_skip -----------------------------------------------------------------------------------------------
SKIP_E, SKIP_ODD_AT = 300, 137
SKIP_CELL, SKIP_LABEL = np.array([0x0204, 0x0406, 0x0608]), np.array([1, 2, 3])


def _skip_case(name, cells, labels, **kw):
    frame = spread_frames(len(cells), 3)
    calls = per_frame_calls(cells + DELTA, np.asarray(labels, np.int32), frame)
    return Case(name, calls, cut=2, **kw)


def digit_skip():
    out = []
    cells = np.tile(SKIP_CELL, (SKIP_E, 1))
    labels = np.tile(SKIP_LABEL, (SKIP_E, 1))
    out.append(_skip_case("digit_skip/all_equal", cells, labels))
    for byte in range(8):                        # z lo, z hi, y lo, y hi, x lo, x hi, code lo, code hi nibble
        c, l = cells.copy(), labels.copy()
        if byte < 6:
            c[SKIP_ODD_AT, 2 - byte // 2] ^= 0x02 << (8 * (byte % 2))
        elif byte == 6:
            l[SKIP_ODD_AT, 2] ^= 0x02
        else:
            l[SKIP_ODD_AT, 0] ^= 0x02
        out.append(_skip_case("digit_skip/one_differs_byte%d" % byte, c, l))
    for name, other in (("top_byte_only", (0, 15, 15)), ("code_all_bits", (0, 0, 0))):
        l = np.tile([15, 15, 15], (SKIP_E, 1))
        l[::3] = other
        out.append(_skip_case("digit_skip/" + name, cells, l))
    corner = np.array([[a, b, c] for a in (0, 65535) for b in (0, 65535) for c in (0, 65535)])
    rng = np.random.default_rng(7)
    out.append(_skip_case("digit_skip/cells_0_and_65535", corner[rng.integers(0, 8, SKIP_E)], labels))
    return out


# ---- 3. scan_counts / 4. scan_deep -------------------------------------------------------------------------------
def _distinct_cells(n):
    i = np.arange(n, dtype=np.int64)
    return np.stack([2 * (i // 16384), 2 * ((i // 128) % 128), 2 * (i % 128)], 1)     # ascending key order with i


def scan_counts(E, kind):
    """kind: "U1" one bucket, "UE" every key distinct, "between": buckets of 2047, 1, 1 entries and one of the rest —
    bucket heads at sorted positions 2047, 2048 and (E >= 2050) 2049"""
    if kind == "U1":
        bucket = np.zeros(E, np.int64)
    elif kind == "UE":
        bucket = np.arange(E, dtype=np.int64)
    else:
        sizes = [SCAN_BLOCK - 1] + [1] * min(2, E - (SCAN_BLOCK - 1))
        sizes += [E - sum(sizes)] if E > sum(sizes) else []
        bucket = np.repeat(np.arange(len(sizes)), sizes)
    rng = np.random.default_rng(E)
    bucket = bucket[rng.permutation(E)]
    cells = _distinct_cells(int(bucket.max()) + 1)[bucket] + np.array([100, 100, 100])
    frame = spread_frames(E, 6)
    calls = per_frame_calls(cells + DELTA, np.tile([2, 3, 4], (E, 1)), frame)
    # (the file measured 4.2 times its yardstick, test_gpu_select_edges.py: the 32768 / 32769 workloads keep three forms)
    return Case("scan_counts/E%d_%s" % (E, kind), calls, cut=5, forms=BIG_FORMS if E > 4 * SCAN_BLOCK else ALL_FORMS)


SCAN_CASES = [(E, kind) for E in (SCAN_BLOCK, SCAN_BLOCK + 1, 16 * SCAN_BLOCK, 16 * SCAN_BLOCK + 1) for kind in ("U1", "UE", "between")]


def scan_deep():
    """2048 * 2048 + 1 entries: device_scan's block sums themselves need more than one block.  Only side, label and
    frame are given; the dump alone is compared (vectorised reference)"""
    E = SCAN_DEEP_E
    i = np.arange(E, dtype=np.int64)
    b = (i * 2654435761) % 3000001                  # about 1.4 entries per bucket, scattered
    cells = np.stack([2 * (b // 16384), 2 * ((b // 128) % 128), 2 * (b % 128)], 1)
    frame = (i // 8000).astype(np.uint32)
    return Case("scan_deep", [(cells + DELTA, np.tile([3, 1, 2], (E, 1)), frame, True)], forms=("one_call",), census=False)


# ---- 5. partition_counts -----------------------------------------------------------------------------------------
PART_SIZES = (1, 63, 64, 65, 127, 128, 129, 200)
SUB_POINTS = np.array([[0.0, -0.3, -0.4], [0.0, -0.3, 0.0], [0.0, -0.3, 0.4], [0.0, 0.2, -0.4], [0.0, 0.2, 0.0], [0.0, 0.2, 0.4]])


def _bucket_entries(size, spread):
    """(offset inside the cell, frame) of a bucket's entries.  "one": one sub-cell, frames round robin; "all": frame f < 6
    keeps to sub-cell f, frame 6 is a run longer than RUN_MAX (the overflow slice); "overflow": one frame's run alone.
    (At these sides two entries of one frame in different sub-cells always lie within the run rule's limit, so a frame
    keeps to one sub-cell unless it is meant for the overflow slice.)"""
    if spread == "one" or size < RUN_MAX + 1:
        return [(DELTA, k % 6) for k in range(size)]
    if spread == "overflow":
        return [(SUB_POINTS[k % 6] + [0.25, 0, 0], 6) for k in range(size)]
    rest = size - (RUN_MAX + 1)
    return [(SUB_POINTS[k % 6] + [0.25, 0, 0], k % 6) for k in range(rest)] + [(SUB_POINTS[k % 6] + [0.25, 0, 0], 6) for k in range(RUN_MAX + 1)]


def _partition_case(name, buckets, **kw):
    """buckets: [(cell, size, spread)], inserted frame by frame (frames 0 .. 6)"""
    rows = []
    for b, (cell, size, spread) in enumerate(buckets):
        for k, (d, f) in enumerate(_bucket_entries(size, spread)):
            rows.append((f, b, k, cell[0] + d[0], cell[1] + d[1], cell[2] + d[2]))
    rows.sort(key=lambda r: (r[0], r[1], r[2]))
    a = np.array(rows)
    calls = per_frame_calls(a[:, 3:6], np.tile([4, 5, 6], (len(a), 1)), a[:, 0].astype(np.uint32))
    return Case(name, calls, cut=len(calls) - 1, **kw)


def partition_counts():
    buckets = []
    for si, size in enumerate(PART_SIZES):
        for pi, spread in enumerate(("one", "all", "overflow")):
            if size == 1 and spread != "one":
                continue
            buckets.append((np.array([120 + 4 * si, 120 + 4 * pi, 120]), size, spread))
    return _partition_case("partition_counts/sizes", buckets)


def partition_many(n_waves=WAVES_MI355X):
    """2 * n_waves buckets, so that every wave of slice_partition_kernel takes a second one: singletons but for sized
    buckets first, last and either side of the stride boundary"""
    U = 2 * n_waves
    sized = {0: (65, "all"), n_waves - 1: (200, "all"), n_waves: (64, "one"), U - 1: (129, "all")}
    buckets = [(np.array([2 * b, 120, 120]), ) + sized.get(b, (1, "one")) for b in range(U)]
    return _partition_case("partition_counts/many_buckets", buckets)


def slice_spread(case):
    """{bucket key: (size, set of slices its entries take)} as slice_assign_kernel decides (sub_cell and run_limit of
    _select_edges): 6 is the overflow slice"""
    keys, off, ids = case.structure()
    out = {}
    for u in range(len(keys)):
        idx = ids[off[u]:off[u + 1]]
        slices = set()
        for f in np.unique(case.frame[idx]):
            run = idx[case.frame[idx] == f]
            subs = [se.sub_cell(case.side[g]) for g in run]
            close = len(run) > RUN_MAX or any(
                subs[a] != subs[b] and not (se.norm3(case.side[run[a]] - case.side[run[b]]) > se.run_limit(ROUGH, case.side[run[a]], case.side[run[b]]))
                for a in range(len(run)) for b in range(a + 1, len(run)))
            slices |= {6} if close else set(subs)
        out[tuple(keys[u])] = (len(idx), slices)
    return out


# ---- 6. hash_counts ----------------------------------------------------------------------------------------------
HASH_LABEL = (5, 6, 7)


def _hash_grid(n=400000):
    """candidate keys on even cells (x, y even, z = 200) with their home slot in a table of 1024"""
    i = np.arange(n, dtype=np.int64)
    cells = np.stack([2 * (i % 700) + 200, 2 * (i // 700) + 200, np.full(n, 200)], 1)
    home = hash_key(pack_key(label_code(HASH_LABEL), cells[:, 0], cells[:, 1], cells[:, 2])) & np.uint64(HASH_MIN - 1)
    return cells, home.astype(np.int64)


def _hash_case(name, cells, extra=(), **kw):
    E = len(cells)
    frame = spread_frames(E, 4)
    calls = per_frame_calls(cells + DELTA, np.tile(HASH_LABEL, (E, 1)), frame)
    return Case(name, calls, cut=3, extra=extra, **kw)


def hash_counts():
    cells, home = _hash_grid()
    rng = np.random.default_rng(11)
    out = []
    for U in (511, 512, 513, 1024, 1025):
        out.append(_hash_case("hash_counts/U%d" % U, cells[rng.permutation(20000)[:U]]))
    # 512 buckets, 44 of them with one home slot; an absent key whose home lies inside their chain
    target = 300
    same = np.flatnonzero(home == target)[:44]
    others = np.flatnonzero((home < target - 100) | (home > target + 200))
    pick = np.concatenate([same, others[rng.permutation(len(others))[:512 - len(same)]]])
    absent = np.setdiff1d(np.flatnonzero(home == target + 5), pick)[0]
    out.append(_hash_case("hash_counts/chain", cells[pick[rng.permutation(len(pick))]],
                          extra=[(cells[absent] + DELTA, np.array(HASH_LABEL))]))
    # a chain that starts in the last three slots and wraps to slot 0
    last = np.flatnonzero(home >= HASH_MIN - 3)[:9]
    mid = np.flatnonzero((home > 100) & (home < 900))
    pick = np.concatenate([last, mid[rng.permutation(len(mid))[:191]]])
    out.append(_hash_case("hash_counts/wrap", cells[pick[rng.permutation(len(pick))]]))
    return out


def hash_slots(case):
    """(home slot of every bucket key, the set of slots linear probing occupies) in build_segment's table: used by the
    reach assertions only.  The occupied set does not depend on the insertion order"""
    keys = case.structure()[0]
    cap = HASH_MIN
    while cap < 2 * len(keys):
        cap *= 2
    home = (hash_key(pack_key(keys[:, 3], keys[:, 0], keys[:, 1], keys[:, 2])) & np.uint64(cap - 1)).astype(np.int64)
    used, wrapped = set(), 0
    for h in home.tolist():
        s = h
        while s in used:
            s = (s + 1) % cap
            wrapped += s == 0
        used.add(s)
    return home, used, cap, wrapped


# ---- 7. id_bits --------------------------------------------------------------------------------------------------
def id_bits():
    out = []
    for n in (8192, 8193):
        rng = np.random.default_rng(n)
        cells, labs = key_pool(rng, 600)
        sizes, pick = [120, n], rng.integers(0, 600, 120 + n)
        frame = np.repeat([0, 1], sizes).astype(np.uint32)
        out.append(Case("id_bits/frame_of_%d" % n, per_frame_calls(cells[pick] + DELTA, labs[pick], frame), cut=1))
    for name, hi in (("span_600000", 600000), ("span_2p20m2", (1 << 20) - 3), ("span_2p20m1_refused", (1 << 20) - 2)):
        rng = np.random.default_rng(hi)
        cells, labs = key_pool(rng, 300)
        pick = rng.integers(0, 300, 4096 + 100)
        frame = np.repeat([0, hi], [4096, 100]).astype(np.uint32)
        out.append(Case("id_bits/" + name, per_frame_calls(cells[pick] + DELTA, labs[pick], frame), cut=1,
                        cfg=dict(max_frame_n=hi + 10)))
    return out


# ---- 8. frame_order ----------------------------------------------------------------------------------------------
def frame_order(E):
    """frame ids out of insertion order: descending, one call with two ids, a frame split by another's (A, B, A), gaps"""
    rng = np.random.default_rng(E)
    cells, labs = key_pool(rng, E // 12)
    pick = rng.integers(0, E // 12, E)
    sizes = [E // 6] * 5
    sizes.append(E - sum(sizes))
    ids = [900, 41, 40, 3, 40, 17]                                   # A = 40, B = 3
    frame = np.repeat(ids, sizes).astype(np.uint32)
    side, lab = cells[pick] + DELTA, labs[pick]
    b = np.cumsum([0] + sizes)
    calls = [(side[b[0]:b[1]], lab[b[0]:b[1]], frame[b[0]:b[1]]), (side[b[1]:b[3]], lab[b[1]:b[3]], frame[b[1]:b[3]])]
    calls += [(side[b[k]:b[k + 1]], lab[b[k]:b[k + 1]], frame[b[k]:b[k + 1]]) for k in (3, 4, 5)]
    return Case("frame_order/E%d" % E, calls, cut=4)


# ---- 9. cold_store -----------------------------------------------------------------------------------------------
def block_switch_sizes():
    n = BLOCK_MAX // 136
    while desc_block_total(n + 1) <= BLOCK_MAX:
        n += 1
    while desc_block_total(n) > BLOCK_MAX:
        n -= 1
    return n, n + 1


def cold_store():
    out = []
    rng = np.random.default_rng(5)
    cells, labs = key_pool(rng, 300)
    sizes = [1, 1, 1, 2, 4092, 10]                                   # the calls' first entries: 0, 1, 2, 3, 5, 4097
    pick = rng.integers(0, 300, sum(sizes))
    frame = np.repeat(np.arange(len(sizes)), sizes).astype(np.uint32)
    out.append(Case("cold_store/offsets", per_frame_calls(cells[pick] + DELTA, labs[pick], frame), cut=4))
    sizes = [5, 7, 5]
    pick = rng.integers(0, 4, 17)
    b = np.cumsum([0] + sizes)
    calls = [(cells[pick[b[k]:b[k + 1]]] + DELTA, labs[pick[b[k]:b[k + 1]]], np.full(sizes[k], k), k == 1) for k in range(3)]
    out.append(Case("cold_store/null_fields", calls, cut=2))
    lo, hi = block_switch_sizes()
    pick = rng.integers(0, 300, lo + hi)
    frame = np.repeat([0, 1], [lo, hi]).astype(np.uint32)
    out.append(Case("cold_store/block_switch", per_frame_calls(cells[pick] + DELTA, labs[pick], frame), cut=1))
    return out


# ---- 10. degenerate ----------------------------------------------------------------------------------------------
def degenerate():
    out = [Case("degenerate/empty", [], forms=("one_call", "per_frame", "view"))]
    out.append(Case("degenerate/one_entry", [([[4.125, 6.125, 8.125]], [1, 2, 3], [0])]))
    # sides in (-0.5, 0.5) go to cell 0 ((int) truncates towards zero), beside cells 0 reached from above
    s = np.array([[0.25, 600.125, 800.125], [-0.3, 600.125, 800.125], [-0.49, 600.2, 800.3], [-0.0, 600.125, 800.0],
                  [0.49, 600.125, 800.125], [600.125, -0.3, 800.125], [600.125, 0.3, 800.125], [600.125, 800.125, -0.45],
                  [600.125, 800.125, 0.45], [-0.2, -0.2, 200.125], [0.2, 0.2, 200.125], [-0.25, 600.125, 800.125]])
    out.append(Case("degenerate/cell_zero", per_frame_calls(s, np.tile([1, 2, 3], (len(s), 1)), spread_frames(len(s), 3)), cut=2))
    return out


# ---- every small workload ----------------------------------------------------------------------------------------
_CASES = None


def cases(n_waves=WAVES_MI355X):
    """every workload but scan_deep, by name"""
    global _CASES
    if _CASES is None or _CASES[0] != n_waves:
        cs = [sort_counts(E) for E in SORT_E] + digit_skip() + [scan_counts(E, k) for E, k in SCAN_CASES]
        cs += [partition_counts(), partition_many(n_waves)] + hash_counts() + id_bits()
        cs += [frame_order(RS_TILE), frame_order(RS_TILE + 1)] + cold_store() + degenerate()
        _CASES = (n_waves, {c.name: c for c in cs})
    return _CASES[1]


REFUSED = ("id_bits/span_2p20m1_refused",)
