"""Workloads at the edges of the batch ordering (sgtd_amd/csrc/order_kernels.hip.h: the one-sweep radix passes over the home
keys and the fused group index), built on tests/_select_edges.py's Workload, and a plain restatement of what the ordering
computes.  Helper module of tests/test_order_edges.py (CPU: every workload reaches its edge) and
tests/test_gpu_order_edges.py (GPU: both forms of the ordering equal the oracle and each other on them).

A case is one table and ONE candidate_selector call of exactly n descriptors, handed in in a shuffled slot order.  Every
`step`-th descriptor is also a table entry (the same sides: a match at distance 0), dealt over NF frames, so that a
descriptor resolved with another home cell's rows, or swept in another pass, changes P, P_swept, M, the votes or the lists.
T and G, the tiles of the sort passes and of the group index, come from the library (sgtd_order_tiles).
"""
import ctypes as C
import re

import numpy as np

import _select_edges as se

ROUGH = 0.03
CBITS, SUB_BITS = 6, 2            # the default config (max_len 50 at resolution 1): 12 + 3 * 6 + 2 = 32 key bits
CMASK = (1 << CBITS) - 1
WIDE_SUB_BITS = 4                 # SGTD_HOME_SUB_BITS=4: 34 key bits, the launch train
NF = 5
LABELS = ((2, 3, 1), (2, 3, 2), (2, 4, 1))      # ascending label codes
FRAC = np.array([0.3, 0.3, 0.3])


def tiles():
    """(T, G) of the library"""
    from sgtd_amd import _lib
    a, b = C.c_int(0), C.c_int(0)
    _lib.lib().sgtd_order_tiles(C.byref(a), C.byref(b))
    return a.value, b.value


# ---- the restatement -----------------------------------------------------------------------------------------------
def home_coord(s):
    """home_coord of probe_kernels.hip.h: (int)side, the all-ones marker where it does not fit or side - 1 truncates below 0"""
    return CMASK if se.c_int(float(s) - 1.0) < 0 else min(se.c_int(s), CMASK)


def home_key(side, label, sub_bits=SUB_BITS):
    x, y, z = (home_coord(v) for v in side)
    ny, nz = 1 << (sub_bits >> 1), 1 << (sub_bits - (sub_bits >> 1))
    f1, f2 = side[1] - se.c_int(side[1]), side[2] - se.c_int(side[2])
    sub = min(max(se.c_int(f1 * ny), 0), ny - 1) * nz + min(max(se.c_int(f2 * nz), 0), nz - 1)
    return ((((se.label_code(label) << CBITS | x) << CBITS | y) << CBITS | z) << sub_bits) | sub


def model(side, label, sub_bits=SUB_BITS):
    """the ordering of a descriptor set: keys, the stable order, the heads (group_heads_kernel's rule), gid, group_first"""
    keys = np.array([home_key(s, l, sub_bits) for s, l in zip(side, label)], np.uint64)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    cell = ks >> np.uint64(sub_bits)
    marker = np.zeros(len(ks), bool)
    for k in range(3):
        marker |= ((cell >> np.uint64(k * CBITS)) & np.uint64(CMASK)) == CMASK
    heads = np.ones(len(ks), bool)
    heads[1:] = (cell[1:] != cell[:-1]) | marker[1:]
    gid = np.cumsum(heads) - 1
    return dict(keys=keys, order=order, sorted=ks, heads=heads, marker=marker, gid=gid, group_first=np.flatnonzero(heads),
                n_groups=int(heads.sum()))


# ---- descriptor sets, in SORTED order (the cases shuffle them) ---------------------------------------------------------
def cell_side(c, frac=FRAC):
    """the c-th of 60^3 home cells, coordinates 1 .. 60 (no marker), ascending in the key"""
    return np.array([1 + (c // 3600) % 60, 1 + (c // 60) % 60, 1 + c % 60], np.float64) + frac


def groups(sizes, first_cell=0, label=LABELS[0], rng=None):
    """consecutive home cells with the given numbers of descriptors, at different places inside the cell"""
    side = []
    for c, n in enumerate(sizes):
        for i in range(n):
            frac = FRAC if rng is None else 0.02 + 0.96 * rng.random(3)
            side.append(cell_side(first_cell + c, frac))
    return np.array(side).reshape(-1, 3), np.tile(np.asarray(label, np.int32), (len(side), 1))


def sizes_to(total, rng, hi=9):
    out = []
    while sum(out) < total:
        out.append(min(int(rng.integers(1, hi + 1)), total - sum(out)))
    return out


def mixed(n, seed=7):
    rng = np.random.default_rng(seed)
    return groups(sizes_to(n, rng), rng=rng)


def one_cell(n):
    """one home cell and one sub-cell class: every key is the same, one digit bucket in every pass"""
    rng = np.random.default_rng(11)
    side = cell_side(20 * 3600 + 20 * 60 + 20, np.zeros(3)) + 0.02 + 0.46 * rng.random((n, 3))
    return side, np.tile(np.asarray(LABELS[0], np.int32), (n, 1))


def own_cells(n):
    return groups([1] * n)


def boundary(T, G, b):
    """a group boundary at sorted positions G + b and T + b; the groups around them straddle nothing else on purpose"""
    rng = np.random.default_rng(13)
    sizes, at = [], 0
    for stop in sorted({G + b, T + b}):
        k, rem = divmod(stop - at, 7)
        sizes += [7] * k + ([rem] if rem else [])
        at = stop
    sizes += [6, 3, 9, 5]
    return groups(sizes, rng=rng)


MARKER_SIDES = np.array([[70.3, 5.3, 6.3], [70.3, 5.3, 6.3], [5.3, 0.0, 6.3], [5.3, 0.0, 6.3], [5.3, 6.3, 1e-17], [5.3, 6.3, 1e-17],
                         [70.3, 5.3, 6.3], [64.2, 70.1, 6.3]])


def markers(T, G):
    """descriptors whose key carries the all-ones marker, with equal keys, adjacent, across the group tile's boundary (sorted
    positions G - 3 .. G + 4, behind fillers of the same label code) and the sort tile's (T - 3 .. T + 4, a higher code)"""
    m = len(MARKER_SIDES)
    lo, hi = sorted({G, T})[0], sorted({G, T})[-1]
    s0, l0 = groups(sizes_to(lo - 3, np.random.default_rng(17)), label=LABELS[0])
    parts = [(s0, l0), (MARKER_SIDES, np.tile(np.asarray(LABELS[0], np.int32), (m, 1)))]
    if hi > lo:
        s1, l1 = groups(sizes_to(hi - 3 - (lo - 3 + m), np.random.default_rng(19)), label=LABELS[1])
        parts += [(s1, l1), (MARKER_SIDES, np.tile(np.asarray(LABELS[1], np.int32), (m, 1)))]
    s2, l2 = groups([4, 1, 6], label=LABELS[2])
    parts.append((s2, l2))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def top_digit(n):
    """keys that differ only in their top digit (the label code's upper eight bits): one cell, 64 codes, many equal keys"""
    side = np.tile(cell_side(7 * 3600 + 7 * 60 + 7), (n, 1))
    label = np.array([[1 + (i % 64) // 8, 1 + (i % 64) % 8, 5] for i in range(n)], np.int32)
    o = np.argsort([se.label_code(l) for l in label], kind="stable")
    return side[o], label[o]


def low_digit(n):
    """keys that differ only in their lowest digit (six bits of the third cell coordinate, the two sub-cell bits)"""
    side = np.array([[9.3, 9.3 + 0.5 * ((i >> 1) & 1), 1 + (i >> 2) % 60 + 0.3 + 0.5 * (i & 1)] for i in range(n)])
    label = np.tile(np.asarray(LABELS[0], np.int32), (n, 1))
    o = np.argsort([home_key(s, l) for s, l in zip(side, label)], kind="stable")
    return side[o], label[o]


# ---- cases -----------------------------------------------------------------------------------------------------------
COUNTS = ("1", "T-1", "T", "T+1", "3T+1", "G-1", "G", "G+1", "3G+1")      # live descriptors, in the library's tiles
CASES = tuple("count " + c for c in COUNTS) + ("one cell", "own cells", "boundary -1", "boundary 0", "boundary 1", "markers", "top digit",
                                                "low digit")


def count_of(sym, T, G):
    m = re.fullmatch(r"(\d*)([TG])?([+-]1)?", sym)
    return int(m.group(1) or 1) * {"T": T, "G": G, None: 1}[m.group(2)] + int(m.group(3) or 0)


def deep(T, G):
    """the case with a look-back at least three tiles deep in both kernels"""
    return "count 3T+1" if T >= G else "count 3G+1"


def descriptors(name, T, G):
    """(side, label) of a case in sorted order"""
    big = 3 * G + 1 if G < T else T + G + 1
    if name.startswith("count "):
        return mixed(count_of(name.split()[1], T, G))
    if name.startswith("boundary "):
        return boundary(T, G, int(name.split()[1]))
    return {"one cell": lambda: one_cell(big), "own cells": lambda: own_cells(big), "markers": lambda: markers(T, G),
            "top digit": lambda: top_digit(T + 5), "low digit": lambda: low_digit(T + 5)}[name]()


_CASES = {}


def case(name, T, G):
    """-> Workload with one query set of exactly n descriptors (no BOOST descriptor) in shuffled slot order, n"""
    if (name, T, G) not in _CASES:
        side, label = descriptors(name, T, G)
        n = len(side)
        wl = se.Workload(ROUGH, stamped=True)
        step = max(1, n // 1500) if name != "one cell" else max(1, n // 10)
        pick = np.arange(0, n, step)
        frames = wl.frames(NF)
        for f in range(NF):
            m = pick[f::NF]
            # (a frame without a picked descriptor still gets an entry, far from every query: frame ids stay consecutive)
            es = side[m] if len(m) else np.array([[40000.0, 40000.0, 40000.0]])
            el = label[m] if len(m) else np.asarray([LABELS[0]], np.int32)
            wl.add(es, el, frames[f], boost=False)
        perm = np.random.default_rng(23).permutation(n)
        wl.tags.setdefault(name, []).append(len(wl.sets))
        wl.sets.append((side[perm], label[perm].astype(np.int32), name))
        _CASES[(name, T, G)] = (wl, n)
    return _CASES[(name, T, G)]


def query_descs(wl, mod, frame=se.QUERY_FRAME):
    side, label, _ = wl.sets[0]
    return wl.descs(mod, side, label, np.full(len(side), frame, np.uint32))


_ANSWERS = {}


def expected(oracle, name, T, G, frame=se.QUERY_FRAME):
    """the oracle's answer of a case (computed once): ov._answer's fields and P"""
    import _overflow_edges as ov
    key = (name, T, G, frame)
    if key not in _ANSWERS:
        wl, n = case(name, T, G)
        o = oracle.OracleManager(rough_dis_threshold=ROUGH)
        wl.load(o, oracle)
        ans = ov._answer(o, o.select(query_descs(wl, oracle, frame)), n, with_rough=False, with_entries=False)
        ans["P"] = int(o.counters()["P"])
        _ANSWERS[key] = ans
    return _ANSWERS[key]


# ---- keypoint batches (frames, loop): descriptors are built on the device, the frames' sizes are ragged ------------------
RAGGED = (120, 0, 0, 120, 9, 120, 0)      # keypoints per query frame: frames without a descriptor between full ones


def ragged_world(synth):
    """(map, xyz, label, kp_off) of a query batch whose descriptor slots are several times its descriptors"""
    m = synth.make_map(24, 120, stream=5)
    qs = synth.make_queries(m, len(RAGGED), stream=5)
    xyz = np.concatenate([qs.xyz[i][:k] for i, k in enumerate(RAGGED)]).astype(np.float32)
    label = np.concatenate([qs.label[i][:k] for i, k in enumerate(RAGGED)])
    off = np.concatenate([[0], np.cumsum(RAGGED)]).astype(np.int64)
    return m, xyz, label, off
