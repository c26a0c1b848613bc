"""Workloads at the edges of the work buffers a query batch runs on (match records, the planner's pass pool, GroupRows, the
undecided queue, the candidate-pair buffer), the hooks that start those buffers small and the comparison each capacity
test makes.  Plain helper module of tests/test_overflow_edges.py (CPU: with the oracle alone every workload reaches its
edge) and tests/test_gpu_overflow_edges.py (GPU: every output of a batch that outgrew a buffer and was re-run by
sgtd_sync equals the oracle, in every form a batch takes).

The workloads are the existing ones: descriptor cases of tests/_select_edges.py (families shell, runs, gate and homes on one
stamped table: one frame per AddSTDescs call, ids 0, 1, 2, ...: what a tail segment and a multi-device handle take) and of
tests/_record_edges.py (stale: three queries in a row on one handle), and small synthetic keypoint maps.
"""
import numpy as np

import _record_edges as rec
import _select_edges as se

# ---- the hooks (sgtd_create in sgtd_amd/csrc/sgtd_accel.hip; every one is read once per handle) -------------------
# name -> (floor, the expression of sgtd_create that applies it)
HOOKS = {
    "SGTD_REC_CAP": (1024, 'getenv("SGTD_REC_CAP")) { e->rec_cap = (size_t)std::max(1024ll, atoll(o))'),
    "SGTD_POOL_UNITS": (64, 'getenv("SGTD_POOL_UNITS")) e->pool_units = (size_t)std::max(64ll, atoll(o))'),
    "SGTD_GROUP_CAP": (1, 'getenv("SGTD_GROUP_CAP")) e->group_cap_hook = (size_t)std::max(1ll, atoll(o))'),
    "SGTD_PAIR_CAP": (64, 'getenv("SGTD_PAIR_CAP")) { e->pair_cap = (size_t)std::max(64ll, atoll(o))'),
    "SGTD_AMB_MIN": (1, 'getenv("SGTD_AMB_MIN")) e->amb_min = (size_t)std::max(1ll, atoll(o))'),
}
AMB_MIN_DEFAULT = 65536      # sgtd_engine::amb_min
AMB_PER_REC = 64             # rec_alloc: the queue holds max(amb_min, rec_cap / 64) entries
MAX_ATTEMPTS = 12            # sync_batch: launches of one batch before SGTD_ERR_CAPACITY

# the comparison of every capacity test: (file under sgtd_amd/csrc, the text of the line)
GUARDS = {
    "pairs_one_query": ("probe_kernels.hip.h", "if (acc > pair_cap) overflow[1] = 1;"),                    # block_scan_kernel
    "pairs_batch": ("probe_kernels.hip.h", "if (wrapped || carry > pair_cap) overflow[1] = 1;"),          # query_base_kernel
    "group_rows": ("probe_kernels.hip.h", "if (n_groups > (long long)rows_cap) {"),                       # group_resolve_kernel
    "records": ("probe_kernels.hip.h", "if (got + take <= (u64)B.rec_cap) { nxt = (u32)got; end = (u32)got + take; }"),   # new_slab
    "make_room": ("probe_kernels.hip.h", "if (end - nxt < need_g) { fits = false; if (lane == 0) B.overflow()[0] = 1; return; }"),
    "queue": ("probe_kernels.hip.h", "if (qa < B.amb_cap) B.amb_queue[qa] = make_uint2(at, pv.word(PH_SLOT, k));"),
    "queue_size": ("sgtd_accel.hip", "CHK(ensure(e, e->amb_queue, std::max<size_t>(e->amb_min, e->rec_cap / 64) * sizeof(uint2)));"),
    "attempts": ("sgtd_accel.hip", "for (int attempt = 0; attempt < 12; attempt++) {"),
}


def source_lines(root):
    """{guard or hook name: line number} of every text above in the engine's sources under `root` (the repository); a text
    that is gone or no longer unique raises"""
    import os
    out, cache = {}, {}
    items = [(k, "sgtd_accel.hip", v[1]) for k, v in HOOKS.items()] + [(k, f, t) for k, (f, t) in GUARDS.items()]
    for name, fn, text in items:
        if fn not in cache:
            with open(os.path.join(root, "sgtd_amd", "csrc", fn)) as fh:
                cache[fn] = fh.read().split("\n")
        hits = [i + 1 for i, line in enumerate(cache[fn]) if text in line]
        if len(hits) != 1:
            raise AssertionError("%s: %d lines of %s hold %r" % (name, len(hits), fn, text))
        out[name] = hits[0]
    return out


def pairs_overflow(total, cap):
    """block_scan_kernel / query_base_kernel: the batch's candidate pairs against the pair buffer: T pairs fit a buffer of T"""
    return total > cap


def groups_overflow(n_groups, cap):
    """group_resolve_kernel: G home cells fit G GroupRows"""
    return n_groups > cap


def queue_overflow(n_queued, cap):
    """the sweep's undecided queue: entry qa is stored while qa < cap, so n entries fit a queue of n"""
    return n_queued > cap


def records_must_overflow(n_matches, cap):
    """new_slab: M records cannot fit a buffer of fewer than M (a buffer of M or more may still overflow: slabs strand
    room, and which wave sweeps what varies from run to run)"""
    return cap < n_matches


def queue_entries(rec_cap, amb_min=AMB_MIN_DEFAULT):
    return max(amb_min, rec_cap // AMB_PER_REC)


# ---- the f32 pre-test's band (f32_bounds in sgtd_amd/csrc/common.hip.h: `const double m = 2.0 * A + 16.0 * u * thr + 1e-12;`)
# A record goes to the undecided queue when its f32 squared distance is neither below (thr - m)^2 nor above (thr + m)^2,
# m = 2 A + 16 u thr + 1e-12 with u = 2^-24 and A = u |(4 |q_k| + 16)_k| >= 4 u |q| / sqrt(3) = 4 u thr / (rough sqrt(3)).  The f32
# distance is within A + 2 u d of the true one (the same comment), so a match with thr (1 - 1e-6) <= d < thr is queued
# whenever A + 14 u thr > 1e-6 thr — for rough <= 0.03: A >= 4.5e-6 thr.
NEAR_REL = 1e-6


def near_threshold(rough_list, qside, rough):
    """of the oracle's rough matches (OracleManager.rough_matches): those within NEAR_REL relative of the threshold"""
    thr = se.norm3(qside[rough_list["q_idx"]]) * rough
    return np.abs(rough_list["dis"] / thr - 1.0) <= NEAR_REL


# ---- home cells (home_keys_kernel / group_heads_kernel of probe_kernels.hip.h) ------------------------------------
SHIPPED_CBITS = 6            # sgtd_accel.hip: the smallest cbits with 2^cbits >= (int)(descriptor_max_len / std_side_resolution) + 3


def home_groups(side, label, cbits=SHIPPED_CBITS):
    """the number of GroupRows a batch of descriptors takes: distinct (label code, (int)side) — a coordinate at or beyond
    the marker 2^cbits - 1, or one whose side - 1 truncates below 0, makes a group of the descriptor's own"""
    cmask = (1 << cbits) - 1
    keys, alone = set(), 0
    for s, l in zip(np.asarray(side, np.float64), np.asarray(label)):
        c = [cmask if se.c_int(v - 1.0) < 0 else min(se.c_int(v), cmask) for v in s]
        if cmask in c:
            alone += 1
        else:
            keys.add((se.label_code(l),) + tuple(c))
    return len(keys) + alone


HOMES_CELLS = 9              # _select_edges.homes: k = 1 .. 9 descriptors in home cell (10 + 3 k, 20, 30) each
HOMES_G = HOMES_CELLS + 1    # ... and the query set's BOOST descriptor in a cell (and label code) of its own


# ---- descriptor workloads ------------------------------------------------------------------------------------------
ROUGH = 0.03
SEL_FAMILIES = ("shell", "runs", "gate", "homes")


def sel_workload():
    """the shell, runs, gate and homes families of tests/_select_edges.py on one stamped table"""
    wl = se.Workload(ROUGH, stamped=True)
    for fam in SEL_FAMILIES:
        getattr(se, fam)(wl)
    return wl


def sel_config():
    return dict(rough_dis_threshold=ROUGH)


def tail_split(wl):
    """AddSTDescs calls before the first query of the tail form (the rest is appended after it: a tail segment)"""
    return len(wl.adds) // 2


def stale_case():
    """tests/_record_edges.py's stale case: query 0 has 40 candidates with lists of 60 .. 99 records, query 1 no candidate,
    query 2 three candidates — three candidate_selector calls in a row on one handle"""
    return rec.stale()[0]


def stale_long_case():
    """stale's first query with every list ten records longer: 40 candidates with lists of 70 .. 109 records, so that the
    list of the highest candidate alone (the shortest: 70 pairs) is still above SGTD_PAIR_CAP's floor"""
    c = rec.Case("stale_long", "stale")
    a, b = c.keys(110), c.keys(8)
    for f in range(40):
        c.entries(a[:70 + f], f)
        c.entries(b[:(f % 5)], f)
        c.end_call()
    c.query(a)
    return c


def shards_of_frames(frames, n_shards, block=64):
    """the shard of every frame id on a multi-device handle (multi_impl.hip.h shard_of: blocks of SGTD_SHARD_BLOCK = 64
    frames dealt round robin)"""
    return (np.asarray(frames, np.int64) // block) % n_shards


# ---- keypoint workloads --------------------------------------------------------------------------------------------
FRAME_MAP = dict(n_frames=60, n_kp=160, stream=77)
FRAME_QUERIES = 6
LOOP_MAP = dict(n_frames=40, n_kp=120, stream=78)
LOOP_SESSION = 40


def frame_world(synth):
    """a map of 60 frames of 160 keypoints and 6 query frames that re-observe map frames"""
    m = synth.make_map(FRAME_MAP["n_frames"], FRAME_MAP["n_kp"], stream=FRAME_MAP["stream"])
    return m, synth.make_queries(m, FRAME_QUERIES, stream=FRAME_MAP["stream"])


def loop_world(synth):
    """a map of 40 frames of 120 keypoints and a session of 40 frames that re-observe map frames (some the same one: a
    later session frame then finds the earlier among its candidates)"""
    m = synth.make_map(LOOP_MAP["n_frames"], LOOP_MAP["n_kp"], stream=LOOP_MAP["stream"])
    return m, synth.make_queries(m, LOOP_SESSION, stream=LOOP_MAP["stream"])


def pose12(pose):
    """synth's (x, y, yaw) poses as rows of the row-major 3x4 [R | t]"""
    p = np.asarray(pose, np.float64)
    c, s = np.cos(p[:, 2]), np.sin(p[:, 2])
    z, o = np.zeros(len(p)), np.ones(len(p))
    return np.stack([c, -s, z, p[:, 0], s, c, z, p[:, 1], z, z, o, z], 1)


def prior_frames(pose, center, radius, margin=1e-3):
    """the map frames a position prior (center (x, y), radius) allows; no frame lies within `margin` of the circle (the
    engine keeps the poses in f32)"""
    d = np.hypot(pose[:, 0] - center[0], pose[:, 1] - center[1])
    assert np.all(np.abs(d - radius) > margin)
    return np.nonzero(d < radius)[0]


def bisect_step(overflows, lo, hi):
    """the smallest cap in (lo, hi] for which overflows(cap) is False, given overflows(lo) and not overflows(hi); returns
    (step, {cap: overflowed} of every cap tried)"""
    tried = {lo: bool(overflows(lo)), hi: bool(overflows(hi))}
    assert tried[lo] and not tried[hi], tried
    while hi - lo > 1:
        mid = (lo + hi) // 2
        tried[mid] = bool(overflows(mid))
        if tried[mid]:
            lo = mid
        else:
            hi = mid
    return hi, tried


def is_step(tried, step):
    """every tried cap below the step overflowed, none at or above it did"""
    return all(ov == (cap < step) for cap, ov in tried.items())


# ---- the oracle's answers, once per workload -------------------------------------------------------------------------
FIELDS = ("side", "label", "frame")
_CACHE = {}


def _answer(o, sel, n_desc, with_rough=True, with_entries=True):
    """a select of the oracle with what else a batch reports: the vote vector, M (rough matches), T (candidate pairs), D
    (query descriptors), the lists' table entries and the rough list"""
    sel.update(votes=o.votes(), M=o.counters()["M"], T=int(sel["cand_off"][-1]), D=int(n_desc))
    if with_entries:
        ent = o.fetch_entries(sel["db_entry"])
        sel["entries"] = {f: getattr(ent, f).copy() for f in FIELDS}
    if with_rough:
        sel["rough"] = o.rough_matches()
    return sel


def sel_expected(oracle):
    """(workload, the oracle's answer per query set) of sel_workload()"""
    if "sel" not in _CACHE:
        wl = sel_workload()
        o = oracle.OracleManager(**sel_config())
        wl.load(o, oracle)
        _CACHE["sel"] = (wl, [_answer(o, o.select(wl.query_descs(oracle, k)), len(wl.sets[k][0])) for k in range(len(wl.sets))])
    return _CACHE["sel"]


def stale_expected(oracle):
    if "stale" not in _CACHE:
        c = stale_case()
        o = oracle.OracleManager(**c.config())
        c.load(o, oracle)
        _CACHE["stale"] = (c, [_answer(o, o.select(c.query_descs(oracle, k)), len(c.queries[k])) for k in range(len(c.queries))])
    return _CACHE["stale"]


def stale_long_expected(oracle):
    if "stale_long" not in _CACHE:
        c = stale_long_case()
        o = oracle.OracleManager(**c.config())
        c.load(o, oracle)
        _CACHE["stale_long"] = (c, o, [_answer(o, o.select(c.query_descs(oracle, 0)), len(c.queries[0]))])
    return _CACHE["stale_long"]


def shard_expected(oracle, n_shards=3):
    """per shard of a multi-device handle over sel_workload(): the answers of a table that holds the shard's frames alone
    (what the shard's own handle computes: its pair total decides whether IT overflows)"""
    if "shards" not in _CACHE:
        wl, _ = sel_expected(oracle)
        out = []
        for s in range(n_shards):
            o = oracle.OracleManager(**sel_config())
            for side, label, frame in wl.adds:
                if shards_of_frames(frame[:1], n_shards)[0] == s:
                    o.add(wl.descs(oracle, side, label, frame))
            out.append([_answer(o, o.select(wl.query_descs(oracle, k)), len(wl.sets[k][0]), with_rough=False) for k in range(len(wl.sets))])
        _CACHE["shards"] = out
    return _CACHE["shards"]


def _frame_descs(oracle, m, first=0):
    """the descriptors of every frame of a synthetic map, stamped first, first + 1, ..."""
    ob = oracle.OracleManager()
    out = []
    for f in range(m.xyz.shape[0]):
        ob.set_current_frame_id(first + f)
        out.append(ob.build(m.xyz[f], m.label[f]))
    return out


def frames_answers(oracle, descs, qs, allowed=None, **cfg):
    """the oracle's answer per query frame of qs on a table of the frames `allowed` (None: all) of descs, and the map from
    the full table's entry ids to that table's (-1: an entry of a frame that is not allowed)"""
    n = np.array([d.n for d in descs], np.int64)
    keep = np.ones(len(descs), bool) if allowed is None else np.isin(np.arange(len(descs)), allowed)
    o = oracle.OracleManager(**cfg)
    for f in np.nonzero(keep)[0]:
        o.add(descs[f])
    emap = np.where(np.repeat(keep, n), np.cumsum(np.repeat(keep, n)) - 1, -1)
    out = []
    for q in range(qs.xyz.shape[0]):
        o.set_current_frame_id(len(descs))
        nd = o.build(qs.xyz[q], qs.label[q], export=False)
        out.append(_answer(o, o.select(), nd, with_rough=(q == 0)))
    return out, emap


FILTER_PRIOR_RADIUS = 16.5


def frame_expected(oracle, synth):
    """dict(map, queries, descs, answers, filtered=(allowed frames, answers, entry map), prior=(center, radius, allowed
    frames, answers, entry map)) of frame_world(): the filter drops the frames of query 0's first and last candidate"""
    if "frame" not in _CACHE:
        m, qs = frame_world(synth)
        descs = _frame_descs(oracle, m)
        ans, _ = frames_answers(oracle, descs, qs)
        cf = ans[0]["cand_frame"]
        allowed = np.setdiff1d(np.arange(m.xyz.shape[0]), [int(cf[0]), int(cf[-1])])
        f_ans, f_map = frames_answers(oracle, descs, qs, allowed)
        center = (float(qs.pose[0, 0]), float(qs.pose[0, 1]))
        near = prior_frames(m.pose, center, FILTER_PRIOR_RADIUS)
        p_ans, p_map = frames_answers(oracle, descs, qs, near)
        _CACHE["frame"] = dict(map=m, queries=qs, descs=descs, answers=ans, filtered=(allowed, f_ans, f_map),
                               prior=(center, FILTER_PRIOR_RADIUS, near, p_ans, p_map))
    return _CACHE["frame"]


def loop_expected(oracle, synth, skip):
    """(map, session, the oracle's sequential loop over the session) of loop_world(): session frame i has the id
    n_map + i and is searched against the frames with an id below n_map + i - skip (sgtd_loop_frames' bound: with skip > 0
    the first session frames do not see the map's last frames either)"""
    key = ("loop", skip)
    if key not in _CACHE:
        m, ses = loop_world(synth)
        n_map = m.xyz.shape[0]
        o = oracle.OracleManager()
        frames = _frame_descs(oracle, m) + _frame_descs(oracle, ses, first=n_map)
        sels, added = [], 0
        for i in range(ses.xyz.shape[0]):
            while added < n_map + i - skip:
                o.add(frames[added])
                added += 1
            d = frames[n_map + i]
            sels.append(_answer(o, o.select(d), d.n, with_rough=False, with_entries=False))      # (millions of pairs: the ids alone)
        _CACHE[key] = (m, ses, sels)
    return _CACHE[key]


# ---- the undecided queue at exactly its capacity ----------------------------------------------------------------------
QUEUE_REC_CAP = 8192                         # with SGTD_AMB_MIN = 1: a queue of 128 entries
QUEUE_Q = np.array([5.05, 6.05, 7.05])       # (every entry within its threshold of 0.317 lies in its own cell: one probe each)
QUEUE_LABEL = (1, 9, 1)
QUEUE_REL = 1e-9


def band_rel(q, rough):
    """m / thr of f32_bounds (common.hip.h) for a query side q: the half width of the f32 pre-test's band, relative"""
    u = 2.0 ** -24
    thr = float(se.norm3(q)) * rough
    a = u * (4.0 * np.abs(np.asarray(q, np.float64)) + 16.0)
    return (2.0 * float(np.sqrt((a * a).sum())) + 16.0 * u * thr + 1e-12) / thr


def queue_case(n_band):
    """one query descriptor and n_band table entries at its threshold to within QUEUE_REL relative, on either side and at
    it (_select_edges.LADDER up to 1e-9, along _select_edges.DIRS), each in a frame of its own with the BOOST entries: the
    f32 pre-test cannot decide any of them, so the sweep queues exactly n_band records (the BOOST entries sit at distance 0)
    -> (workload, the entries' sides)"""
    wl = se.Workload(ROUGH, stamped=True)
    thr = float(se.norm3(QUEUE_Q)) * ROUGH
    ds = [d for d in se.LADDER if abs(d) <= QUEUE_REL]
    ents = []
    for j in range(n_band):
        e = QUEUE_Q + se.DIRS[j % len(se.DIRS)] * (thr * (1.0 + ds[(j // len(se.DIRS)) % len(ds)]))
        ents.append(e)
        wl.add([e], QUEUE_LABEL, wl.frames(1))
    wl.query([QUEUE_Q], QUEUE_LABEL, "queue")
    return wl, np.array(ents)


def queue_expected(oracle, n_band):
    key = ("queue", n_band)
    if key not in _CACHE:
        wl, ents = queue_case(n_band)
        o = oracle.OracleManager(**sel_config())
        wl.load(o, oracle)
        _CACHE[key] = (wl, ents, _answer(o, o.select(wl.query_descs(oracle, 0)), len(wl.sets[0][0])))
    return _CACHE[key]


# ---- caps that depend on the workloads (tests/test_overflow_edges.py shows that they lie where they should) ----------
MULTI_PAIR_CAP = 16384       # between the smallest and the largest shard's pair total of the first gate set
AMB_SETS = (0, 1)            # the first two shell sets: thousands / hundreds of matches at the threshold to within ulps
AMB_REC_CAP = {0: 131072, 1: 32768}     # per set: a record buffer many times its matches, a 64th of which is fewer queue entries than
                                        # it has matches at the threshold
