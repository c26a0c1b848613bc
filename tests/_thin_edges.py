"""Inputs at the structural edges of sgtd_thin_clouds (thin_kernels.hip.h, thin_run of sgtd_accel.hip) and a numpy
restatement of the device pipeline whose wrong versions (mutants) the inputs have to tell apart.  Plain helper module of
tests/test_thin_edges.py (CPU: every input reaches the count or boundary it exists for, the pipeline restated equals the
rule restated, every mutant is caught) and tests/test_gpu_thin_edges.py (GPU: the call equals tests/_thin_ref.py on every
input, bit for bit, in every form of the call).

The rule is tests/_thin_ref.py's and stays the oracle; nothing here predicts an output but `deep`, whose closed form
test_thin_edges.py compares with the oracle at a reduced size.

Constants restated from the sources (test_thin_edges.py asserts them against the text):
  RS_ROUND 256, RS_TILE 4096   SGTD_RS_THREADS, SGTD_RS_THREADS x SGTD_RS_ROUNDS   table_kernels.hip.h:123-125
  DIGIT 8 bits                 radix_scatter_kernel, `(u32)(k >> shift) & 255u`   table_kernels.hip.h:178
  WAVE 64                      SGTD_WAVE   common.hip.h
  SCAN_BLOCK 2048              SGTD_SCAN_THREADS x SGTD_SCAN_ITEMS   table_kernels.hip.h:21-22
  THIN_BLOCK 256               `__launch_bounds__(256)`, `blockIdx.x * 256`   thin_kernels.hip.h:36-38, 62-63, 69-71, 90-91, 107-109
  MAX_CLOUDS 1 << 16           SGTD_REG_MAX_CLOUDS   include/sgtd_accel.h:1231
  MAX_CELL 1 << 20             SGTD_THIN_MAX_CELL   include/sgtd_accel.h:1567
  CELL_BITS 21                 SGTD_THIN_CELL_BITS   thin_kernels.hip.h:22
  key                          cx << 42 | cy << 21 | cz, every coordinate offset by MAX_CELL   thin_kernels.hip.h:52-53
  DROP_KEY 2^63 - 1            SGTD_THIN_DROP_KEY   thin_kernels.hip.h:23 (dropped points carry the cloud n_clouds)
"""
import numpy as np

import _thin_ref as tr

RS_ROUND, RS_TILE, DIGIT, WAVE, SCAN_BLOCK, THIN_BLOCK = 256, 4096, 8, 64, 2048, 256
MAX_CLOUDS, MAX_CELL, CELL_BITS = 1 << 16, 1 << 20, 21
DROP_KEY = (1 << 63) - 1
RECIP_LEAF = 49.0 / 512.0        # 49 * (1 / 49) < 1 in f64: k * leaf * (1 / leaf) falls below k for some k
DEEP_P = (SCAN_BLOCK * SCAN_BLOCK - 1, SCAN_BLOCK * SCAN_BLOCK)      # the scans run over P + 1 words


def key_bits(v):
    """key_bits of sgtd_accel.hip: the bits the cloud sort takes for n_clouds clouds"""
    b = 0
    while v:
        b += 1
        v >>= 1
    return max(b, 1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want):
    return (np.array_equal(got["pt_off"], want["pt_off"]) and np.array_equal(got["n_dropped"], want["n_dropped"])
            and got["points"].shape == want["points"].shape and np.array_equal(bits(got["points"]), bits(want["points"])))


# ---- the device pipeline restated --------------------------------------------------------------------------------
SKIP_PASS = tuple("skip_pass_%d" % d for d in range(8))
MUTANTS = ("trunc", "div_f32", "recip", "inclusive", "out_as_nonfinite", "acc_f32", "sum_to_f32", "pairwise", "key_order",
           "heads_no_cloud", "cloud_bits_short") + SKIP_PASS + ("cloud_sort_tiles", "off_from_flags", "live_short", "col4_first")


def point_keys(points, pt_off, leaf, trunc=False, div_f32=False, recip=False, inclusive=False):
    """thin_keys_kernel -> (key u64, cloud i64 with n_clouds for a dropped point, non-finite mask, out-of-range mask)"""
    p = np.asarray(points, np.float32)
    off = np.asarray(pt_off, np.int64).reshape(-1)
    S, n = off.size - 1, int(off[-1])
    p = p[:n]
    wide = p[:, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        if div_f32:
            q = (p[:, :3] / np.float32(leaf)).astype(np.float64)
        elif recip:
            q = wide * (1.0 / np.float64(leaf))
        else:
            q = wide / np.float64(leaf)
        cell = np.trunc(q) if trunc else np.floor(q)
        finite = np.isfinite(wide).all(axis=1)
        hi = (cell <= float(MAX_CELL)) if inclusive else (cell < float(MAX_CELL))
        inside = ((cell >= -float(MAX_CELL)) & hi).all(axis=1)
    live = finite & inside
    cloud = np.searchsorted(off[1:], np.arange(n), side="right").astype(np.int64)      # the last s with off[s] <= i
    key = np.full(n, DROP_KEY, np.uint64)
    u = (cell[live] + float(MAX_CELL)).astype(np.int64).astype(np.uint64)
    key[live] = (u[:, 0] << np.uint64(2 * CELL_BITS)) | (u[:, 1] << np.uint64(CELL_BITS)) | u[:, 2]
    cl = np.where(live, cloud, S)
    return key, cl, cloud, ~finite, finite & ~inside


def _radix_pass(digit, swap_tiles=False):
    """the permutation of one stable 8-bit pass; swap_tiles: inside a digit the first two tiles' elements change places"""
    if not swap_tiles or len(digit) <= RS_TILE:
        return np.argsort(digit, kind="stable")
    pos = np.arange(len(digit))
    tile = pos // RS_TILE
    tile = np.where(tile < 2, tile ^ 1, tile)
    return np.lexsort((pos, tile, digit))


def _pairwise(v):
    while len(v) > 1:
        h = len(v) // 2
        s = v[0:2 * h:2] + v[1:2 * h:2]
        v = np.concatenate([s, v[2 * h:]]) if len(v) % 2 else s
    return v[0]


def thin_model(points, pt_off, leaf, trunc=False, div_f32=False, recip=False, inclusive=False, out_as_nonfinite=False,
               acc_f32=False, sum_to_f32=False, pairwise=False, key_order=False, heads_no_cloud=False, cloud_bits_short=False,
               skip_pass=None, cloud_sort_tiles=False, off_from_flags=False, live_short=False, col4_first=False):
    """thin_run's passes one by one: keys, the stable sort by the 63 cell bits and then by the cloud's low bits (8 bits a
    pass), heads, the two exclusive scans over n + 1 words, cstart, a walk per run.  Every keyword is one wrong version"""
    p = np.ascontiguousarray(points, np.float32)
    off = np.asarray(pt_off, np.int64).reshape(-1)
    S, n, stride = off.size - 1, int(off[-1]), p.shape[1]
    key, cl, cloud, bad, out = point_keys(p, off, leaf, trunc, div_f32, recip, inclusive)
    if out_as_nonfinite:
        bad, out = bad | out, np.zeros(n, bool)
    dropped = np.stack([np.bincount(cloud[bad], minlength=S)[:S], np.bincount(cloud[out], minlength=S)[:S]], 1).astype(np.int32)
    if n == 0:
        return {"points": np.zeros((0, stride), np.float32), "pt_off": np.zeros(S + 1, np.int64), "n_dropped": dropped.reshape(S, 2)}
    # the two sorts
    order = np.arange(n)
    for d in range(8):
        if skip_pass == d:
            continue
        order = order[_radix_pass(((key[order] >> np.uint64(DIGIT * d)) & np.uint64(255)).astype(np.int64))]
    nbits = key_bits(S - 1) if cloud_bits_short else key_bits(S)
    ck = cl[order] & ((1 << nbits) - 1)
    for shift in range(0, nbits, DIGIT):
        sel = _radix_pass((ck >> shift) & 255, cloud_sort_tiles)
        order, ck = order[sel], ck[sel]
    # heads: a flag per position, a flag at the point the position holds; the live count
    ko, co = key[order], cl[order]
    live = co < S
    head = live.copy()
    head[1:] &= (ko[1:] != ko[:-1]) if heads_no_cloud else ((co[1:] != co[:-1]) | (ko[1:] != ko[:-1]))
    ends = np.flatnonzero(live & np.concatenate([~live[1:], [True]]))
    count = int(ends.max()) + 1 if len(ends) else 0
    if live_short and count and n > RS_TILE and not live[(n - 1) // RS_TILE * RS_TILE:].any():
        count -= 1
    flags = np.concatenate([head, [False]]).astype(np.int64)
    first = np.zeros(n + 1, np.int64)
    first[order[head]] = 1
    excl = np.cumsum(flags) - flags
    first_excl = np.cumsum(first) - first
    K = int(excl[n])
    cstart = np.zeros(K + 1, np.int64)
    cstart[K] = count
    at = np.flatnonzero(head)
    cstart[excl[at]] = at
    out_off = (excl if off_from_flags else first_excl)[off].astype(np.int64)
    # the sums: cell c walks positions cstart[c] .. cstart[c + 1] in order
    lens = np.maximum(cstart[1:] - cstart[:-1], 0)
    vals = p.astype(np.float32 if acc_f32 else np.float64)[order]
    sums = np.zeros((K, stride), vals.dtype)
    with np.errstate(all="ignore"):
        if pairwise:
            for c in range(K):
                if lens[c]:
                    sums[c] = _pairwise(vals[cstart[c]:cstart[c] + lens[c]])
        else:
            by_len = np.argsort(-lens, kind="stable")
            asc = lens[by_len][::-1]
            for k in range(int(lens.max()) if K else 0):
                who = by_len[:K - int(np.searchsorted(asc, k, side="right"))]      # the cells longer than k
                sums[who] += vals[cstart[who] + k]
        s64 = sums.astype(np.float32).astype(np.float64) if sum_to_f32 else sums.astype(np.float64)
        mean = (s64 / lens.astype(np.float64)[:, None]).astype(np.float32)
    head_pt = order[cstart[:K]]
    if col4_first and stride == 4:
        mean[:, 3] = p[head_pt, 3]
    res = np.zeros((K, stride), np.float32)
    res[np.arange(K) if key_order else first_excl[head_pt]] = mean
    return {"points": res, "pt_off": out_off, "n_dropped": dropped}


def mutant(name):
    """the keyword arguments of thin_model for a name of MUTANTS"""
    return {"skip_pass": int(name[-1])} if name.startswith("skip_pass_") else {name: True}


# ---- a case ------------------------------------------------------------------------------------------------------
class Case:
    """gen() -> (points, pt_off, leaf, stride); reach(points, pt_off, leaf, stride) -> True where the input reaches the
    count or boundary the case exists for, from the input alone.  The input and the oracle's output are made once"""

    def __init__(self, name, gen, reach, catches):
        self.name, self._gen, self._reach, self.catches = name, gen, reach, tuple(catches)
        self._in = self._want = None

    def input(self):
        if self._in is None:
            pts, off, leaf, stride = self._gen()
            pts = np.ascontiguousarray(pts, np.float32).reshape(-1, stride)
            pts.setflags(write=False)
            self._in = (pts, np.asarray(off, np.int64), float(leaf), stride)
        return self._in

    def reaches(self):
        return bool(self._reach(*self.input()))

    def want(self):
        if self._want is None:
            pts, off, leaf, _ = self.input()
            self._want = tr.thin(pts, off, leaf)
        return self._want

    def has_out_of_range(self):
        pts, off, leaf, _ = self.input()
        return bool(point_keys(pts, off, leaf)[4].any())


def _pack(clouds, stride=3):
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    full = [np.asarray(c, np.float32).reshape(-1, stride) for c in clouds if len(c)]
    return (np.concatenate(full) if full else np.zeros((0, stride), np.float32)), off


def _scattered(rng, n, leaf, lo=(-11, -9, -3), per_cell=3):
    """n points over about n / per_cell cells, the points of a cell scattered over the whole index range; some
    coordinates negative"""
    C = max(1, n // per_cell)
    cid = rng.integers(0, C, n)
    cell = np.stack([cid % 23 + lo[0], (cid // 23) % 19 + lo[1], cid // 437 + lo[2]], 1)
    return ((cell + rng.uniform(0.1, 0.9, (n, 3))) * leaf).astype(np.float32)


def _dropped(n, first=0):
    """n points that are dropped, of both kinds in turn (leaf 1.0): NaN, +inf, -inf; far out, cell 2^20 exactly, cell
    -2^20 - 1"""
    rows = np.array([[0.5, np.nan, 0.5], [3e6, 0.5, 0.5], [np.inf, 0.5, 0.5], [float(MAX_CELL), 0.5, 0.5], [0.5, 0.5, -np.inf],
                     [0.5, -float(MAX_CELL) - 1.0, 0.5]], np.float32)
    return rows[(np.arange(n) + first) % len(rows)]


def _spans(key, live, bounds, n):
    """every bound below n has a cell with a point before it and a point at or behind it"""
    idx = np.flatnonzero(live)
    _, inv = np.unique(key[idx], return_inverse=True)
    lo = np.full(inv.max() + 1, n)
    hi = np.zeros(inv.max() + 1, np.int64)
    np.minimum.at(lo, inv, idx)
    np.maximum.at(hi, inv, idx)
    return all(((lo < b) & (hi >= b)).any() for b in bounds if b < n)


# ---- 1. count-N --------------------------------------------------------------------------------------------------
COUNT_N = (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)
COUNT_LEAF = 0.1


def _count_gen(N):
    def gen():
        rng = np.random.default_rng(1000 + N)
        pts = _scattered(rng, N, COUNT_LEAF)
        g = rng.integers(0, N, N // 10)      # on the faces of a leaf that is no f32: the division's rounding decides the cell
        pts[g, 0] = (rng.integers(-11, 12, len(g)) * 0.1).astype(np.float32)
        return pts, [0, N], COUNT_LEAF, 3
    return gen


def _count_reach(N):
    def reach(pts, off, leaf, stride):
        key, cl, _, bad, out = point_keys(pts, off, leaf)
        cells = len(np.unique(key))
        ok = len(pts) == N and off.tolist() == [0, N] and not bad.any() and not out.any()
        if N >= WAVE - 1:
            ok = ok and 2.0 <= N / cells <= 4.5 and (pts[:, :3] < 0).any()
            ok = ok and _spans(key, np.ones(N, bool), (WAVE, RS_ROUND, SCAN_BLOCK, RS_TILE, 2 * RS_TILE), N)
        return ok
    return reach


# ---- 2. digit-d --------------------------------------------------------------------------------------------------
DIGIT_PAIRS = 300
DIGIT_BASE = (0x0B3A5C << 42) | (0x0C5A3B << 21) | 0x0D2B4E


def digit_bit(d):
    return 62 if d == 7 else DIGIT * d + 7


def _cell_point(k, frac):
    u = np.array([(k >> 42) & 0x1FFFFF, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF], np.float64)
    return u - MAX_CELL + frac      # leaf 1.0; |cell| <= 2^20 and a quarter: exact in f32


def _digit_gen(d):
    def gen():
        rng = np.random.default_rng(2000 + d)
        hi, lo = DIGIT_BASE | (1 << digit_bit(d)), DIGIT_BASE & ~(1 << digit_bit(d))
        others = [int(x) for x in rng.integers(0, 1 << 62, 5)]
        rows = []
        for k in range(DIGIT_PAIRS):
            rows.append(_cell_point(hi, 0.25 * rng.integers(1, 4, 3)))
            rows.append(_cell_point(lo, 0.25 * rng.integers(1, 4, 3)))
            if k % 7 == 3:
                rows.append(_cell_point(others[k % 5], 0.25 * rng.integers(1, 4, 3)))
        return np.array(rows), [0, len(rows)], 1.0, 3
    return gen


def _digit_reach(d):
    def reach(pts, off, leaf, stride):
        key = point_keys(pts, off, leaf)[0]
        assert np.array_equal(pts.astype(np.float64) * 4, np.round(pts.astype(np.float64) * 4))
        u, cnt = np.unique(key, return_counts=True)
        a, b = sorted(int(x) for x in u[np.argsort(-cnt, kind="stable")[:2]])
        x = a ^ b
        two = key[(key == np.uint64(a)) | (key == np.uint64(b))]
        turns = int((two[1:] != two[:-1]).sum())
        return x != 0 and x >> (DIGIT * d) << (DIGIT * d) == x and x >> (DIGIT * d) < 256 and int(two[0]) == b and turns >= 2 * DIGIT_PAIRS - 1 \
            and len(u) > 2 and np.abs(pts).max() > (MAX_CELL / 2 if d == 7 else 0)
    return reach


# ---- 3. cloud-digit-b, clouds-S ----------------------------------------------------------------------------------
CLOUD_DIGIT = {0: (5, 2, 1), 1: (600, 257, 1), 2: (MAX_CLOUDS, None, 0)}      # n_clouds, the two clouds that alternate
CLOUD_PAIRS = 300


def _cloud_digit_gen(b):
    def gen():
        S, hi, lo = CLOUD_DIGIT[b]
        rng = np.random.default_rng(3000 + b)
        clouds = [np.zeros((0, 3))] * S
        z = np.arange(2 * CLOUD_PAIRS, dtype=np.float64)
        if hi is None:      # the dropped points carry the cloud S: they meet cloud 0 in the corner cell, whose key they share
            corner = np.full((CLOUD_PAIRS, 3), MAX_CELL - 0.5)
            mix = np.empty((2 * CLOUD_PAIRS, 3))
            mix[0::2], mix[1::2] = [np.nan, 0.5, 0.5], corner      # (not finite only: the case goes to the host function too)
            clouds[0] = mix
            clouds[1000] = rng.uniform(-5, 5, (40, 3))
            clouds[S - 1] = rng.uniform(-5, 5, (3, 3))
        else:
            clouds[hi] = np.stack([z[0::2] * 0 + 0.5, z[0::2] * 0 + 0.5, z[0::2] + 0.5], 1)
            clouds[lo] = np.stack([z[1::2] * 0 + 0.5, z[1::2] * 0 + 0.5, z[1::2] + 0.5], 1)
            for s in range(S):
                if s not in (hi, lo) and s % 4 != 3:
                    clouds[s] = rng.uniform(-5, 5, (1 + s % 2, 3))
            clouds[S - 1] = np.concatenate([rng.uniform(-5, 5, (3, 3)), _dropped(4)])
        pts, off = _pack(clouds)
        return pts, off, 1.0, 3
    return gen


def _cloud_digit_reach(b):
    def reach(pts, off, leaf, stride):
        key, cl = point_keys(pts, off, leaf)[:2]
        seq = cl[np.argsort(key, kind="stable")]      # the clouds of the positions the cloud sort meets
        x = seq[1:] ^ seq[:-1]
        turn = (x != 0) & ((x >> (DIGIT * b)) << (DIGIT * b) == x) & ((x >> (DIGIT * b)) < 256)
        at = np.flatnonzero(turn)
        return off.size - 1 == CLOUD_DIGIT[b][0] and len(at) >= 2 * CLOUD_PAIRS - 1 and seq[at[0]] > seq[at[0] + 1] \
            and key_bits(off.size - 1) > DIGIT * b
    return reach


CLOUDS_S = (255, 256, 257, 65535, 65536)
CLOUDS_BASE = np.array([[0.3, 0.3, 0.3], [5.3, -2.2, 1.1]])


def _clouds_gen(S):
    def gen():
        rng = np.random.default_rng(4000 + S)
        drops = sorted({0, S // 5, S // 2, (3 * S) // 4, S - 1})
        clouds = []
        for s in range(S):
            if s % 3 == 0:
                c = CLOUDS_BASE[:1 + (s % 6 == 0)]      # the coordinates of cloud 0
            elif s % 7 in (1, 2):
                c = np.zeros((0, 3))
            else:
                c = rng.uniform(-50, 50, (1, 3))
            if s in drops:
                k = drops.index(s)
                c = c if len(c) else rng.uniform(-50, 50, (1, 3))
                c = np.concatenate([_dropped(2, k), c, _dropped(3, k + 2)])
            clouds.append(c)
        pts, off = _pack(clouds)
        return pts, off, 1.0, 3
    return gen


def _clouds_meet(key, cl, S):
    """two clouds with no live point of another between them: the last cell of one is the first cell of the other"""
    live = cl < S
    order = np.lexsort((key[live], cl[live]))
    k, c = key[live][order], cl[live][order]
    return bool(((c[1:] != c[:-1]) & (k[1:] == k[:-1])).any())


def _clouds_reach(S):
    def reach(pts, off, leaf, stride):
        key, cl, cloud, bad, out = point_keys(pts, off, leaf)
        sizes = np.diff(off)
        ok = off.size - 1 == S and (sizes == 0).sum() > S // 8 and np.median(sizes) in (1, 2) and _clouds_meet(key, cl, S)
        for s in (0, S - 1):
            ok = ok and bad[cloud == s].any() and out[cloud == s].any() and (cl == s).any()
        ok = ok and len(np.unique(cloud[bad | out])) >= 4
        if S in (256, 65536):
            ok = ok and key_bits(S) == key_bits(S - 1) + 1 and S % 256 == 0
        return ok and off[-1] <= 70000
    return reach


# ---- 4. empties, boundary ----------------------------------------------------------------------------------------
def _empties_gen(kind):
    def gen():
        rng = np.random.default_rng(5000)
        a, b = _scattered(rng, 200, 0.5), _scattered(rng, 150, 0.5)
        none = [np.zeros((0, 3))]
        clouds = none * 300 + [a] + none * 300 + [b] + none * 300 if kind == "300" else none * (MAX_CLOUDS - 1) + [a]
        pts, off = _pack(clouds)
        return pts, off, 0.5, 3
    return gen


def _empties_reach(kind):
    def reach(pts, off, leaf, stride):
        full = np.flatnonzero(np.diff(off)).tolist()
        if kind == "300":
            return full == [300, 601] and off.size - 1 == 902
        return full == [MAX_CLOUDS - 1] and off.size - 1 == MAX_CLOUDS
    return reach


BOUNDARY_AT = (RS_TILE, SCAN_BLOCK)
BOUNDARY_SHARED = 5


def _boundary_gen(B):
    def gen():
        rng = np.random.default_rng(6000 + B)
        leaf = RECIP_LEAF
        a = _scattered(rng, B, leaf, lo=(-24, -9, -3))       # x cells -24 .. -2
        b = _scattered(rng, B // 2 + 77, leaf, lo=(2, -9, -3))      # x cells 2 .. 24
        g = rng.integers(0, B - BOUNDARY_SHARED, B // 10)      # y exactly k * leaf: k * leaf / leaf = k, k * leaf * (1 / leaf) may fall short
        a[g, 1] = (rng.integers(1, 10, len(g)) * leaf).astype(np.float32)
        shared = ((rng.uniform(0.1, 0.9, (2 * BOUNDARY_SHARED, 3))) * leaf).astype(np.float32)      # cell (0, 0, 0): the last of a, the first of b
        a[B - BOUNDARY_SHARED:], b[:BOUNDARY_SHARED] = shared[:BOUNDARY_SHARED], shared[BOUNDARY_SHARED:]
        return np.concatenate([a, b]), [0, B, B + len(b)], leaf, 3
    return gen


def _boundary_reach(B):
    def reach(pts, off, leaf, stride):
        key, cl = point_keys(pts, off, leaf)[:2]
        rk = point_keys(pts, off, leaf, recip=True)[0]
        m = key[B - 1]
        return off[1] == B and off.size == 3 and (key[B - BOUNDARY_SHARED:B + BOUNDARY_SHARED] == m).all() and key[:B].max() == m \
            and key[B:].min() == m and (key == m).sum() == 2 * BOUNDARY_SHARED and (rk != key).any() and off[2] > B + RS_ROUND
    return reach


# ---- 5. drops ----------------------------------------------------------------------------------------------------
def _corner_gen():
    rng = np.random.default_rng(7100)
    plain = rng.uniform(-40, 40, (RS_TILE - 200, 3))
    mix = np.empty((400, 3))
    mix[0::2], mix[1::2] = _dropped(200), MAX_CELL - 0.5      # dropped points and the corner cell's in turn: one key
    return _pack([plain[:2000], np.concatenate([plain[2000:], mix])])


DROPS = {
    "all-1": lambda: _pack([_dropped(300)]),
    "all-3": lambda: _pack([_dropped(100), _dropped(150, 1), _dropped(50, 2)]),
    "first": lambda: _pack([np.concatenate([_dropped(1), np.random.default_rng(7001).uniform(-9, 9, (499, 3))])]),
    "last-live": lambda: _pack([np.concatenate([_dropped(700), [[0.5, -1.5, 2.5]]])]),
    "live-4096-then": lambda: _pack([np.concatenate([np.random.default_rng(7002).uniform(-6, 6, (RS_TILE, 3)), _dropped(RS_TILE)])]),
    "live-8192-then": lambda: _pack([np.random.default_rng(7003).uniform(-7, 7, (3000, 3)),
                                     np.concatenate([np.random.default_rng(7004).uniform(-7, 7, (2 * RS_TILE - 3000, 3)), _dropped(RS_TILE)])]),
    "then-live-4096": lambda: _pack([np.concatenate([_dropped(RS_TILE), np.random.default_rng(7005).uniform(-6, 6, (RS_TILE, 3))])]),
    "then-live-8192": lambda: _pack([_dropped(1000), np.concatenate([_dropped(RS_TILE - 1000, 4), np.random.default_rng(7006).uniform(-7, 7, (5000, 3))]),
                                     np.random.default_rng(7007).uniform(-7, 7, (2 * RS_TILE - 5000, 3))]),
    "corner": _corner_gen,
}


def _drops_reach(kind):
    def reach(pts, off, leaf, stride):
        key, cl, cloud, bad, out = point_keys(pts, off, leaf)
        S, n = off.size - 1, len(pts)
        live = cl < S
        both = bad.any() and out.any()
        if kind in ("all-1", "all-3"):
            return both and not live.any() and S == int(kind[-1]) and (np.diff(off) > 0).all()
        if kind == "first":
            return not live[0] and live[1:].all()
        if kind == "last-live":
            return live[-1] and not live[:-1].any() and both
        if kind.startswith("live-"):
            L = int(kind.split("-")[1])
            return n == L + RS_TILE and live[:L].all() and not live[L:].any() and both and L % RS_TILE == 0
        if kind.startswith("then-live-"):
            L = int(kind.split("-")[2])
            return n == L + RS_TILE and live[RS_TILE:].all() and not live[:RS_TILE].any() and both
        # corner: the positions that hold the key of all ones lie on both sides of a tile boundary, live and dropped on each
        order = np.argsort(key, kind="stable")
        top = np.flatnonzero(key[order] == np.uint64(DROP_KEY))
        lv = live[order][top]
        left, right = top < RS_TILE, top >= RS_TILE
        in_cloud = set(cloud[order][top].tolist())
        return lv[left].any() and (~lv[left]).any() and lv[right].any() and (~lv[right]).any() and in_cloud == {S - 1} and S == 2
    return reach


# ---- 6. long-cell-N ----------------------------------------------------------------------------------------------
LONG_N = (RS_TILE + 1, 2 * RS_TILE + 1, 3 * RS_TILE + 1)
LONG_LEAF, LONG_EVERY = 1024.0, 53
BIG = float(1 << 60)      # the f64 sum near BIG * m keeps multiples of 256, 512 or 1024 only: what a small value adds depends on where it is added
PERTURBATIONS = ("swap_4095_4096", "swap_tiles", "swap_rounds", "reverse_wave", "rotate_one", "swap_64_apart", "swap_256_apart")


def perturbation(name, n):
    """a permutation of the long cell's run (its points in index order) that a sum in another order would make"""
    q = np.arange(n)
    if name == "swap_4095_4096":
        q[[RS_TILE - 1, RS_TILE]] = q[[RS_TILE, RS_TILE - 1]]
    elif name == "swap_tiles":
        q = np.concatenate([q[RS_TILE:2 * RS_TILE], q[:RS_TILE], q[2 * RS_TILE:]])      # (the second tile may be short)
    elif name == "swap_rounds":
        q[2 * RS_ROUND:4 * RS_ROUND] = np.concatenate([q[3 * RS_ROUND:4 * RS_ROUND], q[2 * RS_ROUND:3 * RS_ROUND]])
    elif name == "reverse_wave":
        q[5 * WAVE:6 * WAVE] = q[5 * WAVE:6 * WAVE][::-1].copy()
    elif name == "rotate_one":
        q = np.roll(q, 1)
    elif name == "swap_64_apart":
        q[[1000, 1000 + WAVE]] = q[[1000 + WAVE, 1000]]
    elif name == "swap_256_apart":
        q[[3000, 3000 + RS_ROUND]] = q[[3000 + RS_ROUND, 3000]]
    else:
        raise KeyError(name)
    return q


def long_run(pts):
    """the indices of the long cell's points"""
    return np.flatnonzero(pts[:, 0] < LONG_LEAF)


def perturbed(pts, name):
    run = long_run(pts)
    out = np.array(pts)
    out[run] = pts[run[perturbation(name, len(run))]]
    return out


def _witness(rng, n):
    """n f32-exact values whose f64 sum in this order is a small integer and in most other orders another one: the
    running sum moves among BIG * 1 .. 7, where it keeps multiples of 256, 512 or 1024, small values are added on the way
    and the last values take the big part away"""
    w = rng.integers(1, 1000, n).astype(np.float64)
    m = 0
    for k in range(n - 8):
        if k == 0 or rng.random() < 0.3:
            step = int(rng.integers(-3, 4)) if k else 3
            step = step if 1 <= m + step <= 7 else -step
            if step and 1 <= m + step <= 7:
                w[k] = BIG * step
                m += step
    for k in range(n - 8, n - 1):
        take = min(m, 1)
        w[k], m = (-BIG * take, m - take) if take else (w[k], m)
    assert m == 0
    return w


def _long_gen(N):
    def gen():
        total = N
        while total - total // (LONG_EVERY + 1) < N:
            total += 1
        for seed in range(200):
            rng = np.random.default_rng(8000 + N + 100000 * seed)
            pts = np.empty((total, 4))
            pts[:, :3] = rng.uniform(1.0, 1000.0, (total, 3))
            pts[:, 3] = rng.integers(1, 1000, total)
            small = np.arange(total) % (LONG_EVERY + 1) == LONG_EVERY
            assert total - int(small.sum()) == N
            pts[small, 0] += LONG_LEAF      # the second cell: one step along x, the higher key
            run = np.flatnonzero(~small)
            w = _witness(rng, N)
            pts[run, 3] = w
            pts = pts.astype(np.float32)
            mean = (lambda v: np.float32(np.add.accumulate(v)[-1] / np.float64(N)).view(np.uint32))
            base = mean(w)
            if all(mean(w[perturbation(p, N)]) != base for p in PERTURBATIONS) and abs(np.add.accumulate(w)[-1]) < 1e8:
                return pts, [0, total], LONG_LEAF, 4
        raise AssertionError("no seed makes every perturbation of long-cell-%d change the sum" % N)
    return gen


def _long_reach(N):
    def reach(pts, off, leaf, stride):
        key = point_keys(pts, off, leaf)[0]
        u, cnt = np.unique(key, return_counts=True)
        run = long_run(pts)
        w = pts[run, 3].astype(np.float64)
        total = np.add.accumulate(w)[-1]
        return stride == 4 and len(u) == 2 and cnt[0] == N and u[1] > u[0] and 0 < cnt[1] < N // 40 and len(run) == N \
            and np.abs(w).max() >= BIG and total == np.round(total) and abs(total) < 1e8 and off.tolist() == [0, len(pts)] \
            and (np.diff(np.flatnonzero(key == u[1])) > 1).all()
    return reach


# ---- 7. deep -----------------------------------------------------------------------------------------------------
DEEP_PER_CELL = 4


def deep(P, scan_block=SCAN_BLOCK, tile=RS_TILE):
    """P points in three clouds, DEEP_PER_CELL points in a cell before the clouds split it and a cell's points a quarter of the batch apart;
    every `tile + 3`-th point is not finite and every `scan_block + 5`-th out of range.  Coordinates are multiples of
    1/32, so every sum is exact in f64 whatever its order, and the expected output is a closed form: -> (points, pt_off,
    leaf, 3), the dict the call must return"""
    leaf = 0.5
    C = (P + DEEP_PER_CELL - 1) // DEEP_PER_CELL
    i = np.arange(P, dtype=np.int64)
    c = i % C
    cell = np.stack([c % 211 - 105, (c // 211) % 199 - 99, c // (211 * 199) - 12], 1).astype(np.float64)
    frac = np.stack([(i * 7) % 16, (i * 5 + 3) % 16, (i * 3 + 1) % 16], 1) / 16.0 + 1.0 / 32.0
    pts = ((cell + frac) * leaf).astype(np.float32)
    bad = i % (tile + 3) == 7
    out = (i % (scan_block + 5) == 11) & ~bad
    pts[bad, 1] = np.nan
    pts[out, 0] = 3e6
    off = np.array([0, P // 3 + 1, P // 3 + 1 + scan_block, P], np.int64) if P > 3 * scan_block + 3 else np.array([0, P], np.int64)
    S = off.size - 1
    cloud = np.searchsorted(off[1:], i, side="right")
    live = ~(bad | out)
    g = cloud[live] * C + c[live]
    u, first, inv, cnt = np.unique(g, return_index=True, return_inverse=True, return_counts=True)
    wide = pts[live].astype(np.float64)
    sums = np.stack([np.bincount(inv, weights=wide[:, a], minlength=len(u)) for a in range(3)], 1)      # exact: the order is free
    mean = (sums / cnt.astype(np.float64)[:, None]).astype(np.float32)
    rows = mean[np.argsort(first, kind="stable")]      # by smallest point index; the clouds lie back to back
    out_off = np.searchsorted(u // C, np.arange(S + 1), side="left").astype(np.int64)
    dropped = np.stack([np.bincount(cloud[bad], minlength=S), np.bincount(cloud[out], minlength=S)], 1).astype(np.int32)
    return (pts, off, leaf, 3), {"points": rows, "pt_off": out_off, "n_dropped": dropped}


def deep_reaches(P, scan_block=SCAN_BLOCK):
    """the scans over P + 1 words: at scan_block^2 + 1 words there are scan_block + 1 block sums, which need a second
    level, and word P stands alone in the last block"""
    blocks = (P + 1 + scan_block - 1) // scan_block
    return blocks == scan_block + 1 and P % scan_block == 0 if P == scan_block * scan_block else blocks == scan_block and P == scan_block * scan_block - 1


# ---- the cases and what each must catch --------------------------------------------------------------------------
_RULE = ("trunc", "div_f32", "acc_f32", "sum_to_f32", "key_order")
_DROP = ("inclusive", "out_as_nonfinite")


def _all_cases():
    cs = [Case("count-%d" % N, _count_gen(N), _count_reach(N), () if N == 1 else _RULE[2:] if N < 255 else _RULE + (("cloud_sort_tiles",) if N > RS_TILE else ()))
          for N in COUNT_N]
    cs += [Case("digit-%d" % d, _digit_gen(d), _digit_reach(d), ("skip_pass_%d" % d,)) for d in range(8)]
    cs += [Case("cloud-digit-%d" % b, _cloud_digit_gen(b), _cloud_digit_reach(b), ("key_order",) if b < 2 else ("cloud_bits_short",)) for b in range(3)]
    cs += [Case("clouds-%d" % S, _clouds_gen(S), _clouds_reach(S),
                _DROP + ("heads_no_cloud", "off_from_flags") + (("cloud_bits_short",) if S in (256, 65536) else ())) for S in CLOUDS_S]
    cs += [Case("empties-300", _empties_gen("300"), _empties_reach("300"), ("trunc", "key_order")),
           Case("empties-max", _empties_gen("max"), _empties_reach("max"), ("trunc", "key_order"))]
    cs += [Case("boundary-%d" % B, _boundary_gen(B), _boundary_reach(B), ("recip", "heads_no_cloud")) for B in BOUNDARY_AT]
    drops = {"all-1": _DROP, "all-3": _DROP, "first": ("trunc",), "last-live": _DROP, "live-4096-then": _DROP + ("live_short",),
             "live-8192-then": _DROP + ("live_short",), "then-live-4096": _DROP, "then-live-8192": _DROP + ("off_from_flags",),
             "corner": _DROP + ("cloud_sort_tiles", "cloud_bits_short")}
    cs += [Case("drops-" + k, (lambda k=k: DROPS[k]() + (1.0, 3)), _drops_reach(k), drops[k]) for k in DROPS]
    cs += [Case("long-cell-%d" % N, _long_gen(N), _long_reach(N), ("pairwise", "col4_first", "acc_f32", "cloud_sort_tiles")) for N in LONG_N]
    return {c.name: c for c in cs}


_CASES = None


def cases():
    """every case but deep, by name"""
    global _CASES
    if _CASES is None:
        _CASES = _all_cases()
    return _CASES


def caught_by():
    """mutant -> the cases that must catch it"""
    out = {m: [] for m in MUTANTS}
    for c in cases().values():
        for m in c.catches:
            out[m].append(c.name)
    return out


# the cases that run in every form of the call (test_gpu_thin_edges.py), one of each family
EVERY_FORM = ("count-4097", "digit-7", "cloud-digit-1", "clouds-256", "empties-300", "boundary-4096", "drops-all-3", "drops-live-8192-then",
              "drops-corner", "long-cell-8193")
# one handle, call after call: stale words behind n, a change of stride, K = 0 between runs.  (name, stride; None: an empty batch)
SEQUENCE = (("count-8193", 3), ("count-63", 3), ("drops-all-3", 3), ("count-4097", 3), ("long-cell-4097", 4), (None, 3), ("count-8193", 3))
