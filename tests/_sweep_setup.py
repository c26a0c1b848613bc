"""Workloads at the edges of the sweep's per-pass set-up (probe_sorted_kernel / sweep_pass of probe_kernels.hip.h): what a
wavefront does once per pass — taking the header's derived constants (ngap, -hi2), checking the room of its columns'
record streams, locating the visit list's ranges — and the group tails of the test loop.  Plain helper module of
tests/test_sweep_setup.py (CPU: with the oracle alone every family reaches its edge) and tests/test_gpu_sweep_setup.py
(GPU: every form of the sweep equals the oracle on them).

Families (descriptor workloads on tests/_select_edges.py's Workload, one frame per AddSTDescs call so that a tail segment
can take the second half):
  widths   1 .. 9 query descriptors per home cell: passes of R = 1, 2, 3, 4 descriptors and 4 + k as a pass of four and a
           ragged one; the descriptors sit at different corners and faces of the cell, so the 27-cell gates of a pass's
           columns differ per range (the penalties that carry -hi2)
  lengths  visit lists of exactly 1, 63, 64, 65, 255, 256, 257, 4095, 4096 and 4097 entries (one bucket, every entry in the
           query's own sub-cell, no other bucket of the label code near): group tails of one and two words, the 64-word
           window and its rebuild at position 4096
  band     _select_edges.shell: entries at the threshold to within ulps ... 1e-1 either side, and _overflow_edges.queue_case:
           a known number of records that the f32 pre-test cannot decide (the undecided queue, fed by the header's ngap)
  room     the first gate set (45 lists of about a thousand records): under SGTD_REC_SLAB=512 / SGTD_REC_RATE=1 nearly every
           pass takes a fresh slab and the lists move
"""
import numpy as np

import _overflow_edges as ov
import _select_edges as se

ROUGH = ov.ROUGH
LENGTHS = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
LEN_FRAMES = 6                       # the entries of every length are dealt over six frames
LEN_CELL = np.array([3.0, 4.0, 5.0])
LEN_Q = LEN_CELL + np.array([0.1, -0.2, -0.3])
WIDTH_LABEL = (2, 1, 1)
# where in its home cell a descriptor sits (fractions of the cell per side): corners, faces and the middle
WIDTH_SPOTS = np.array([[0.05, 0.5, 0.5], [0.95, 0.95, 0.5], [0.5, 0.5, 0.5], [0.05, 0.05, 0.95], [0.95, 0.5, 0.05],
                        [0.5, 0.95, 0.95], [0.3, 0.05, 0.3], [0.7, 0.7, 0.95], [0.05, 0.95, 0.05]])
ROOM_ENV = {"SGTD_REC_SLAB": 512, "SGTD_REC_RATE": 1}
QUEUE_ENV = {"SGTD_REC_CAP": ov.QUEUE_REC_CAP, "SGTD_AMB_MIN": 1}


def len_label(i):
    return (3, 1 + i, 1)


def gate_mask(s):
    """the 27 cells of voxel_round whose centre lies within 1.5 of the side (STDesc.cpp:327-342), as a bit mask"""
    m, c = 0, 0
    for x in (-1, 0, 1):
        for y in (-1, 0, 1):
            for z in (-1, 0, 1):
                p = (se.c_int(s[0] + x), se.c_int(s[1] + y), se.c_int(s[2] + z))
                d = [float(s[k]) - (float(p[k]) + 0.5) for k in range(3)]
                if np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) < 1.5:
                    m |= 1 << c
                c += 1
    return m


def widths(wl):
    rng = np.random.default_rng(41)
    items = []
    for k in range(1, 10):
        home = np.array([10.0 + 3 * k, 20.0, 30.0])
        q = home + WIDTH_SPOTS[:k]
        ents = home - 1.4 + 3.8 * rng.random((80, 3))
        items.append((q, [ents[:40], ents[40:]]))
    se._pack(wl, items, WIDTH_LABEL, "widths")


def width_homes(side):
    """descriptors per home cell ((int) of every side) of a query set's sides (the BOOST descriptor left out)"""
    cells = {}
    for s in np.asarray(side, np.float64)[:-1]:
        cells.setdefault(tuple(se.c_int(v) for v in s), []).append(s)
    return cells


def main_workload():
    """widths, band (shell) and room (gate) on one stamped table with the BOOST entries"""
    wl = se.Workload(ROUGH, stamped=True)
    widths(wl)
    se.shell(wl)
    se.gate(wl)
    return wl


def length_entries(i, n):
    rng = np.random.default_rng(100 + i)
    return LEN_CELL + np.stack([-0.4 + 0.8 * rng.random(n), -0.45 + 0.4 * rng.random(n), -0.45 + 0.25 * rng.random(n)], 1)


def lengths_workload():
    """a table without BOOST entries: per length a label code of its own, one bucket, the query in the entries' sub-cell"""
    wl = se.Workload(ROUGH, stamped=True)
    ents = [length_entries(i, n) for i, n in enumerate(LENGTHS)]
    for f in range(LEN_FRAMES):
        side = np.concatenate([e[f::LEN_FRAMES] for e in ents])
        label = np.concatenate([np.tile(len_label(i), (len(e[f::LEN_FRAMES]), 1)) for i, e in enumerate(ents)])
        wl.add(side, label.astype(np.int32), wl.frames(1), boost=False)
    for i in range(len(LENGTHS)):
        wl.query([LEN_Q], len_label(i), "lengths")
    return wl, ents


def query_descs(wl, mod, k, frame=se.QUERY_FRAME):
    side, label, _ = wl.sets[k]
    return wl.descs(mod, side, label, np.full(len(side), frame, np.uint32))


# ---- the oracle's answers, once per workload and stamping ------------------------------------------------------------
_CACHE = {}


def _answers(oracle, wl, sets, frames):
    o = oracle.OracleManager(**ov.sel_config())
    wl.load(o, oracle)
    return {k: ov._answer(o, o.select(query_descs(wl, oracle, k, frames[k])), len(wl.sets[k][0])) for k in sets}


def held_frame(ans):
    """the table frame a FRAMES query is stamped with: the plain answer's first candidate (its entries then do not count)"""
    return int(ans["cand_frame"][0]) if len(ans["cand_frame"]) else 0


def expected(oracle, name, held=False):
    """(workload, {set: the oracle's answer}, {set: the frame id the queries carry}).  name: main, lengths or a queue_case
    size; held: the queries carry the id of a frame the table holds"""
    key = (name, held)
    if key not in _CACHE:
        if held:
            wl, plain, _ = expected(oracle, name)
            frames = {k: held_frame(a) for k, a in plain.items()}
        else:
            wl = main_workload() if name == "main" else lengths_workload()[0] if name == "lengths" else ov.queue_case(name)[0]
            sets = range(len(wl.sets))
            if name == "main":       # (every widths set, the shell sets at the threshold to within ulps, the first gate set)
                sets = wl.tags["widths"] + wl.tags["shell"][:2] + wl.tags["gate"][:1]
            frames = {k: se.QUERY_FRAME for k in sets}
        _CACHE[key] = (wl, _answers(oracle, wl, list(frames), frames), frames)
    return _CACHE[key]
