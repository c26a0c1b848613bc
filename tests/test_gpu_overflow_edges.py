"""Work-buffer overflow and the re-run of sgtd_sync (sync_batch in sgtd_accel.hip) at their edges in every form, against the
oracle bit for bit.  Workloads and the restated hooks and comparisons: tests/_overflow_edges.py (tests/test_overflow_edges.py
shows without a GPU that every cap set here lies where it should).

Every hook is read once per handle in sgtd_create: it is set before the handle is created and deleted right after.  Every
case asserts stats()["overflowed"] and the movement of reruns_total / rewrites_total (which repair ran), that
batches_total moved by 1 + the re-runs and overflow_launches_total by the launches that raised a flag, and that the same
batch enqueued again on the grown buffers raises nothing and gives the same answer.  After every repair: candidates, votes,
pair_off, every match list's (q_idx, db_entry) and its entries, the full vote vector, last_M, last_D, last_cand_pairs, and
last of all result_rough (the diagnostic sweep re-runs the batch once more, on the same handle).

  causes   candidate pairs (SGTD_PAIR_CAP = T, T - 1, 64: one query in the automatic mode and SGTD_SELECT_MODE 1 and 2, a
           batch in the same three, deferred lists finished with a keep mask); GroupRows (SGTD_GROUP_CAP = G, G - 1, 1 on the
           homes set, with and without a tail segment; the step found by bisection on a keypoint batch); the pass pool
           (SGTD_POOL_UNITS = 64 and the step by bisection); match records (SGTD_REC_CAP = 1024, M / 2, M, 2 M, 4 M, 16 M, and
           1024 with SGTD_REC_RATE = 1); the undecided queue (SGTD_AMB_MIN = 1: a queue of rec_cap / 64 entries)
  forms    candidate_selector, query_frames, search_frame (lists_only or not, ordinary and page-locked arrays), a batch
           enqueued with fetch=False and read only through verify / refine_poses / overlap / align_keypoints, a frame filter
           and a position prior, loop_frames, a view beside its owner's batch, a three-shard handle of which one shard
           overflows, the export of the exchange path, two batches back to back (both under the pair and the record cause)

The refit, the overlap and the alignment of the handle that never overflowed are compared on one query with their numpy
restatements (tests/_refine_ref.py, _overlap_ref.py, _align_ref.py).  Not proven here: that a kernel behind a raised flag
touches nothing — the re-run overwrites whatever it wrote, so only a fault would show a missing guard.

The deferred form counts no flagged launch: the flag is raised by the list pass of sgtd_finish_lists, which is no launch of
the batch's pipeline (include/sgtd_accel.h: overflow_launches_total counts launches).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _overflow_edges as ov  # noqa: E402
import _record_edges as rec  # noqa: E402

pytestmark = pytest.mark.gpu

TOTALS = ("batches_total", "overflow_launches_total", "reruns_total", "rewrites_total")
MODES = {"auto": {}, "mode1": {"SGTD_SELECT_MODE": "1"}, "mode2": {"SGTD_SELECT_MODE": "2"}}
_CLEAN = {}


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from sgtd_amd import manager, synth
    oracle.build_library()
    return oracle, manager, synth


# ---- handles and counters ------------------------------------------------------------------------------------------
def _new(manager, monkeypatch, env, **kw):
    """a handle created under the hooks `env`, which are gone again when it returns"""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return manager.STDescManager(**kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _totals(g):
    st = g.stats()
    return {k: st[k] for k in TOTALS}


def _check_repair(g, before, kind, tag, flagged=None, group=False):
    """the flag and the counters' movement since `before` for a batch that was waited for.  kind: none (nothing raised),
    rewrite (the list pass alone ran again), rerun (the whole batch ran again), records (the flag only has to agree with
    the re-runs).  flagged: launches that raised a flag, where they are not the re-runs (rewrite: 1).  group: a
    multi-device handle, whose batches_total is one shard's while the other counters are sums"""
    st = g.stats()
    d = {k: int(st[k] - before[k]) for k in TOTALS}
    msg = "%s: overflowed %d, %s" % (tag, st["overflowed"], d)
    assert d["reruns_total"] < ov.MAX_ATTEMPTS - 1, msg            # (it converged: no SGTD_ERR_CAPACITY, and not at the last try)
    if not group:
        assert d["batches_total"] == 1 + d["reruns_total"], msg
    if kind == "none":
        assert st["overflowed"] == 0 and d["reruns_total"] == 0 and d["rewrites_total"] == 0, msg
        want = 0
    elif kind == "rewrite":
        assert st["overflowed"] == 1 and d["rewrites_total"] == 1 and d["reruns_total"] == 0, msg
        want = 1
    elif kind == "rerun":
        assert st["overflowed"] == 1 and d["reruns_total"] >= 1 and d["rewrites_total"] == 0, msg
        want = d["reruns_total"]
    else:
        assert kind == "records"
        assert st["overflowed"] == (1 if d["reruns_total"] else 0) and d["rewrites_total"] == 0, msg
        want = d["reruns_total"]
    assert d["overflow_launches_total"] == (want if flagged is None else flagged), msg
    return d


def _kind_of_pairs(total, cap):
    return "rewrite" if ov.pairs_overflow(total, max(cap, ov.HOOKS["SGTD_PAIR_CAP"][0])) else "none"


# ---- comparisons with the oracle -----------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_votes(g, q, exp, tag):
    lo, v = g.result_votes(q)
    want = exp["votes"]
    n = min(len(v), len(want) - lo)
    np.testing.assert_array_equal(v[:n].astype(np.float64), want[lo:lo + n], err_msg=tag)
    assert v[n:].sum() == 0 and want[:lo].sum() == 0 and want[lo + n:].sum() == 0, tag


def _check_query(g, res, q, exp, tag, emap=None, multi=False):
    nc = len(exp["cand_frame"])
    assert int(res.n_cand[q]) == nc, tag
    np.testing.assert_array_equal(res.cand_frame[q, :nc], exp["cand_frame"], err_msg=tag)
    np.testing.assert_array_equal(res.cand_votes[q, :nc], exp["cand_votes"], err_msg=tag)
    np.testing.assert_array_equal(res.pair_off[q, :nc + 1], exp["cand_off"], err_msg=tag)
    assert np.all(res.pair_off[q, nc:] == exp["cand_off"][-1]), tag
    qi, de = g.result_pairs(q, res)
    np.testing.assert_array_equal(qi, exp["q_idx"], err_msg=tag)
    if not multi:       # (a multi-device handle's entry ids are the shards' own: the same entries)
        np.testing.assert_array_equal(de if emap is None else emap[de], exp["db_entry"], err_msg=tag)
    if "entries" in exp:
        got = g.fetch_entries(de)
        for f in ov.FIELDS:
            np.testing.assert_array_equal(getattr(got, f), exp["entries"][f], err_msg=tag + " " + f)


def _check_stats(g, answers, tag):
    st = g.stats()
    assert st["last_M"] == sum(a["M"] for a in answers), tag
    assert st["last_cand_pairs"] == sum(a["T"] for a in answers), tag
    assert st["last_D"] == sum(a["D"] for a in answers) and st["last_queries"] == len(answers), tag


def _check_batch(g, answers, tag, emap=None, multi=False, votes=True):
    """every output of the batch that was last enqueued on g (waited for here) against the oracle's answers"""
    res = g.results()
    for q, exp in enumerate(answers):
        t = "%s query %d" % (tag, q)
        _check_query(g, res, q, exp, t, emap, multi)
        if votes:
            _check_votes(g, q, exp, t)
    _check_stats(g, answers, tag)
    return res


def _check_rough(g, q, exp, tag, emap=None):
    """result_rough: the diagnostic sweep re-runs the batch on the same handle (once more through the same buffers)"""
    got, want = g.result_rough(q), exp["rough"]
    for key in ("q_idx", "cell", "frame"):
        np.testing.assert_array_equal(got[key], want[key], err_msg="%s rough %s" % (tag, key))
    np.testing.assert_array_equal(got["db_entry"] if emap is None else emap[got["db_entry"]], want["db_entry"], err_msg=tag + " rough entry")
    np.testing.assert_array_equal(_bits(got["dis"]), _bits(want["dis"]), err_msg=tag + " rough dis")


def _twice(g, enqueue, answers, kind, tag, flagged=None, rough=True, fixed_records=False, **kw):
    """the batch under the hook (the repair `kind`), the same batch again on the grown buffers (nothing raised, the same
    answer), then the rough list of query 0.  fixed_records: the handle's record buffer was set by SGTD_REC_CAP — if the
    first run fitted it, nothing has grown, and the second run reserves room by the rate the first one measured (measured:
    the shell set's second run takes 139 296 records of a buffer of 131 072 that held its first): there the second run's
    flag only has to agree with its counters"""
    before = _totals(g)
    enqueue()
    _check_batch(g, answers, tag, **kw)
    d = _check_repair(g, before, kind, tag, flagged=flagged, group=kw.get("multi", False))
    second = "records" if fixed_records and d["reruns_total"] == 0 and d["rewrites_total"] == 0 else "none"
    before = _totals(g)
    enqueue()
    _check_batch(g, answers, tag + " again", **kw)
    _check_repair(g, before, second, tag + " again", group=kw.get("multi", False))
    if rough and not kw.get("multi"):
        _check_rough(g, 0, answers[0], tag, kw.get("emap"))
    return d


# ---- workloads on handles ------------------------------------------------------------------------------------------
def _sel_handle(manager, monkeypatch, env, oracle, tail=False, devices=None):
    wl, ex = ov.sel_expected(oracle)
    kw = dict(ov.sel_config())
    if devices:
        kw["devices"] = devices
    g = _new(manager, monkeypatch, env, **kw)
    if tail:
        h = ov.tail_split(wl)
        wl.load(g, manager, 0, h)
        g.finalize()                                   # (the table is built: what follows goes to a tail segment)
        wl.load(g, manager, h, None)
    else:
        wl.load(g, manager)
    return g, wl, ex


def _stale_handle(manager, monkeypatch, env, oracle):
    c, ex = ov.stale_expected(oracle)
    g = _new(manager, monkeypatch, env, **c.config())
    c.load(g, manager)
    return g, c, ex


def _frame_handle(manager, monkeypatch, env, fe, keypoints=False, poses=False):
    g = _new(manager, monkeypatch, env)
    m = fe["map"]
    g.add_frames(m.xyz, m.label, keep_keypoints=keypoints)
    if poses:
        g.set_frame_poses(np.arange(m.xyz.shape[0]), ov.pose12(m.pose))
    return g


def _one_query_cases(oracle):
    """(name, handle maker, query descriptors maker, the oracle's answer) of the one-query cases: the homes set and stale's
    first query"""
    wl, ex = ov.sel_expected(oracle)
    k = wl.tags["homes"][0]
    c, sx = ov.stale_expected(oracle)
    return {
        "homes": (lambda ma, mp, env: _sel_handle(ma, mp, env, oracle)[0], lambda ma: wl.query_descs(ma, k), ex[k]),
        "stale": (lambda ma, mp, env: _stale_handle(ma, mp, env, oracle)[0], lambda ma: c.query_descs(ma, 0), sx[0]),
    }


# ---- cause 1: candidate pairs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", ["homes", "stale"])
def test_pair_cap_one_query(mods, monkeypatch, case, mode):
    """block_scan_kernel's own check (one query in the block form: the automatic mode and SGTD_SELECT_MODE 1) and
    launch_lists' query_base_kernel (SGTD_SELECT_MODE 2): T pairs fit a buffer of T, T - 1 and 64 re-run the write pass alone"""
    oracle, manager, _ = mods
    make, query, exp = _one_query_cases(oracle)[case]
    T = exp["T"]
    for cap in (T, T - 1, 64):
        g = make(manager, monkeypatch, dict(MODES[mode], SGTD_PAIR_CAP=cap))
        q = query(manager)
        _twice(g, lambda: g.query_descs(q), [exp], _kind_of_pairs(T, cap), "%s/%s/pair_cap %d of %d" % (case, mode, cap, T))
        assert g.stats()["select_form"] in ((2,) if mode == "mode2" else (0,))
        g.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_pair_cap_batch(mods, monkeypatch, mode):
    """query_base_kernel over a batch: the block passes (automatic mode, SGTD_SELECT_MODE 1) and launch_lists (2)"""
    oracle, manager, synth = mods
    fe = ov.frame_expected(oracle, synth)
    qs, ans = fe["queries"], fe["answers"]
    T = sum(a["T"] for a in ans)
    for cap in (T, T - 1, 64):
        g = _frame_handle(manager, monkeypatch, dict(MODES[mode], SGTD_PAIR_CAP=cap), fe)
        _twice(g, lambda: g.query_frames(qs.xyz, qs.label, fetch=False), ans, _kind_of_pairs(T, cap),
               "batch/%s/pair_cap %d of %d" % (mode, cap, T))
        g.close()


def _keep_tensor(mask):
    import torch
    return torch.tensor([mask - (1 << 64) if mask >= (1 << 63) else mask], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("name", ["all", "none", "bit0", "highest", "alternating"])
def test_pair_cap_deferred_lists_keep_their_mask(mods, monkeypatch, name):
    """set_deferred_lists + finish_lists(keep) into a pair buffer of T, T - 1 and 64, T the total of the KEPT lists: the list
    pass that sgtd_sync runs again (rerun_write) writes the masked lists, the losers' lists stay empty"""
    oracle, manager, _ = mods
    c, ent, sx = ov.stale_long_expected(oracle)      # (the highest candidate's list alone is above the hook's floor)
    mask = rec.keep_masks(len(sx[0]["cand_frame"]))[name]
    exp = rec.masked(sx[0], mask)
    got = ent.fetch_entries(exp["db_entry"])
    exp = dict(exp, T=int(exp["cand_off"][-1]), entries={f: getattr(got, f).copy() for f in ov.FIELDS})
    T = exp["T"]
    for cap in (T, T - 1, 64):
        g = _new(manager, monkeypatch, {"SGTD_SELECT_MODE": "2", "SGTD_PAIR_CAP": max(cap, 0)}, **c.config())
        c.load(g, manager)
        g.set_deferred_lists(True)
        keep = _keep_tensor(mask)
        q = c.query_descs(manager, 0)

        def enqueue():
            g.query_descs(q)
            g.finish_lists(keep)
        kind = _kind_of_pairs(T, cap)
        assert name == "none" or kind == ("none" if cap == T else "rewrite")
        _twice(g, enqueue, [exp], kind, "deferred/%s/pair_cap %d of %d" % (name, cap, T), flagged=0, rough=False)
        assert g.stats()["select_form"] == 2
        if kind == "none" and name != "all":
            # the lists of all candidates once more into the buffer that held the kept ones: T_all pairs, a rewrite
            before = _totals(g)
            g.finish_lists(None)
            _check_batch(g, [sx[0]], "deferred/%s/unmasked" % name)
            st = g.stats()
            assert st["rewrites_total"] - before["rewrites_total"] == (1 if sx[0]["T"] > max(cap, 64) else 0)
        g.close()


# ---- cause 2: GroupRows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", [False, True])
def test_group_cap_on_the_homes_set(mods, monkeypatch, tail):
    """G = 10 home cells by construction: G GroupRows hold them, G - 1 and 1 re-run the batch; with a tail segment a row
    takes two slots"""
    oracle, manager, _ = mods
    G = ov.HOMES_G
    for cap in (G, G - 1, 1):
        g, wl, ex = _sel_handle(manager, monkeypatch, {"SGTD_GROUP_CAP": cap}, oracle, tail=tail)
        k = wl.tags["homes"][0]
        q = wl.query_descs(manager, k)
        _twice(g, lambda: g.query_descs(q), [ex[k]], "rerun" if ov.groups_overflow(G, cap) else "none",
               "homes/tail %d/group_cap %d of %d" % (tail, cap, G))
        assert (g.stats()["tail_entries"] > 0) == tail
        g.close()


def _batch_overflows(manager, monkeypatch, fe, env, tag):
    """one fresh handle, one batch under `env`: parity, and whether it overflowed"""
    qs, ans = fe["queries"], fe["answers"]
    g = _frame_handle(manager, monkeypatch, env, fe)
    before = _totals(g)
    g.query_frames(qs.xyz, qs.label, fetch=False)
    _check_batch(g, ans, tag, votes=False)
    d = _check_repair(g, before, "records", tag)
    g.close()
    return d["reruns_total"] > 0


def _step(manager, monkeypatch, fe, hook, lo, hi):
    return ov.bisect_step(lambda cap: _batch_overflows(manager, monkeypatch, fe, {hook: cap}, "%s %d" % (hook, cap)), lo, hi)


def test_group_cap_step_on_a_keypoint_batch(mods, monkeypatch):
    """the smallest SGTD_GROUP_CAP that does not overflow, by bisection over fresh handles: parity on both sides of the step
    (every handle is compared), every tried cap below it overflows and none at or above it, and a second search finds the
    same value"""
    oracle, manager, synth = mods
    fe = ov.frame_expected(oracle, synth)
    hi = sum(a["D"] for a in fe["answers"])          # (no more home cells than descriptors)
    step, tried = _step(manager, monkeypatch, fe, "SGTD_GROUP_CAP", 1, hi)
    step2, tried2 = _step(manager, monkeypatch, fe, "SGTD_GROUP_CAP", 1, hi)
    print("GroupRows: the %d-descriptor batch of frame_world() needs %d (second search: %d)" % (hi, step, step2))
    assert ov.is_step(tried, step) and ov.is_step(tried2, step2), (step, tried, step2, tried2)
    assert step == step2 and 1 < step <= hi, "GroupRows needed: %d, then %d" % (step, step2)


def test_pool_units_step_on_a_keypoint_batch(mods, monkeypatch):
    """SGTD_POOL_UNITS = 64 re-runs the batch; the smallest value that does not, by bisection (the pool's cursor keeps
    counting past the capacity, so the need is a sum over the passes and the same in every run)"""
    oracle, manager, synth = mods
    fe = ov.frame_expected(oracle, synth)
    qs, ans = fe["queries"], fe["answers"]
    g = _frame_handle(manager, monkeypatch, {"SGTD_POOL_UNITS": 64}, fe)
    _twice(g, lambda: g.query_frames(qs.xyz, qs.label, fetch=False), ans, "rerun", "batch/pool_units 64")
    g.close()
    hi = 1 << 21
    step, tried = _step(manager, monkeypatch, fe, "SGTD_POOL_UNITS", 64, hi)
    step2, tried2 = _step(manager, monkeypatch, fe, "SGTD_POOL_UNITS", 64, hi)
    print("pass pool: the batch of frame_world() needs %d units (second search: %d)" % (step, step2))
    assert ov.is_step(tried, step) and ov.is_step(tried2, step2), (step, tried, step2, tried2)
    assert step == step2, "pass pool units needed: %d, then %d" % (step, step2)


# ---- cause 4: match records ----------------------------------------------------------------------------------------
def _ladder(M):
    return [1024, M // 2, M, 2 * M, 4 * M, 16 * M]


@pytest.mark.parametrize("rung", range(6))
def test_rec_cap_ladder_batch(mods, monkeypatch, rung):
    oracle, manager, synth = mods
    fe = ov.frame_expected(oracle, synth)
    qs, ans = fe["queries"], fe["answers"]
    M = sum(a["M"] for a in ans)
    cap = _ladder(M)[rung]
    g = _frame_handle(manager, monkeypatch, {"SGTD_REC_CAP": cap}, fe)
    _twice(g, lambda: g.query_frames(qs.xyz, qs.label, fetch=False), ans, "rerun" if ov.records_must_overflow(M, cap) else "records",
           "batch/rec_cap %d of %d" % (cap, M), fixed_records=True)
    g.close()


def test_rec_cap_ladder_one_query(mods, monkeypatch):
    oracle, manager, _ = mods
    c, sx = ov.stale_expected(oracle)
    M = sx[0]["M"]
    for cap in _ladder(M):
        g, _, _ = _stale_handle(manager, monkeypatch, {"SGTD_REC_CAP": cap}, oracle)
        q = c.query_descs(manager, 0)
        _twice(g, lambda: g.query_descs(q), [sx[0]], "rerun" if ov.records_must_overflow(M, cap) else "records",
               "stale/rec_cap %d of %d" % (cap, M), fixed_records=True)
        g.close()


def test_rec_cap_with_lists_that_move(mods, monkeypatch):
    """SGTD_REC_RATE = 1: every list gets the smallest room and moves as it grows, into a buffer that overflows in the same
    sweep (make_room's own exit): the keypoint batch, and the first gate set, whose 45 lists of a thousand records each
    outgrow any first room (a record buffer of 1024, and one that holds the first rooms but not the moves)"""
    oracle, manager, synth = mods
    fe = ov.frame_expected(oracle, synth)
    qs, ans = fe["queries"], fe["answers"]
    g = _frame_handle(manager, monkeypatch, {"SGTD_REC_CAP": 1024, "SGTD_REC_RATE": 1}, fe)
    _twice(g, lambda: g.query_frames(qs.xyz, qs.label, fetch=False), ans, "rerun", "batch/rec_cap 1024/rec_rate 1", fixed_records=True)
    g.close()
    wl, ex = ov.sel_expected(oracle)
    k = wl.tags["gate"][0]
    assert ex[k]["M"] > 512 * ex[k]["D"]
    for cap in (1024, 32768):
        g, _, _ = _sel_handle(manager, monkeypatch, {"SGTD_REC_CAP": cap, "SGTD_REC_RATE": 1}, oracle)
        q = wl.query_descs(manager, k)
        _twice(g, lambda: g.query_descs(q), [ex[k]], "rerun", "gate/rec_cap %d/rec_rate 1" % cap, fixed_records=True)
        assert g.stats()["list_moves_total"] > 0
        g.close()


# ---- cause 5: the undecided queue ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ov.AMB_SETS)
def test_undecided_queue_grows_with_the_record_buffer(mods, monkeypatch, k):
    """SGTD_AMB_MIN = 1: the queue holds rec_cap / 64 entries.  A record buffer that holds the shell set's records several
    times over is not re-run under the default floor and is re-run under the hook, because the queue cannot hold the
    matches at the threshold; the re-run grows the queue with the record buffer and converges"""
    oracle, manager, _ = mods
    for env, kind in (({"SGTD_REC_CAP": ov.AMB_REC_CAP[k]}, "none"),
                      ({"SGTD_REC_CAP": ov.AMB_REC_CAP[k], "SGTD_AMB_MIN": 1}, "rerun"),
                      ({"SGTD_REC_CAP": 1024, "SGTD_AMB_MIN": 1}, "rerun")):
        g, wl, ex = _sel_handle(manager, monkeypatch, env, oracle)
        q = wl.query_descs(manager, k)
        _twice(g, lambda: g.query_descs(q), [ex[k]], kind, "shell set %d/%s" % (k, env), fixed_records=True)
        g.close()


def test_undecided_queue_at_exactly_its_capacity(mods, monkeypatch):
    """`qa < B.amb_cap`: 128 undecided records fit the queue of QUEUE_REC_CAP / 64 = 128 entries (no re-run, and every one of
    them is decided: the answer is the oracle's), 129 do not (a re-run); under the default floor neither re-runs"""
    oracle, manager, _ = mods
    cap = ov.queue_entries(ov.QUEUE_REC_CAP, 1)
    for n, hook, kind in ((cap, 1, "none"), (cap + 1, 1, "rerun"), (cap + 1, None, "none")):
        wl, _, exp = ov.queue_expected(oracle, n)
        env = {"SGTD_REC_CAP": ov.QUEUE_REC_CAP}
        if hook:
            env["SGTD_AMB_MIN"] = hook
        g = _new(manager, monkeypatch, env, **ov.sel_config())
        wl.load(g, manager)
        q = wl.query_descs(manager, 0)
        _twice(g, lambda: g.query_descs(q), [exp], kind, "queue of %d, %d undecided, hook %s" % (cap, n, hook), fixed_records=True)
        g.close()


@pytest.mark.parametrize("family", ["gate", "runs"])
def test_small_queue_on_gate_and_runs(mods, monkeypatch, family):
    """the gate and runs sets under SGTD_AMB_MIN = 1: none of their matches is within 1e-6 of the threshold (the CPU test),
    so whether the small queue overflows is left open: the flag agrees with the re-runs, and the answer is the oracle's"""
    oracle, manager, _ = mods
    wl, ex = ov.sel_expected(oracle)
    for k in wl.tags[family][:2]:
        g, _, _ = _sel_handle(manager, monkeypatch, {"SGTD_REC_CAP": 4 * ex[k]["M"], "SGTD_AMB_MIN": 1}, oracle)
        q = wl.query_descs(manager, k)
        _twice(g, lambda: g.query_descs(q), [ex[k]], "records", "%s set %d" % (family, k), fixed_records=True)
        g.close()


# ---- forms -----------------------------------------------------------------------------------------------------------
def _cause_env(cause, T):
    return {"pairs": {"SGTD_PAIR_CAP": T - 1}, "records": {"SGTD_REC_CAP": 1024}, "groups": {"SGTD_GROUP_CAP": 1}}[cause]


CAUSE_KIND = {"pairs": "rewrite", "records": "rerun", "groups": "rerun"}
FRAME_KEYS = ("cand_frame", "cand_votes", "pair_off", "score", "rot", "t", "inlier_off", "inlier_q_idx")


@pytest.mark.parametrize("page_locked", [False, True])
@pytest.mark.parametrize("lists_only", [False, True])
@pytest.mark.parametrize("cause", ["pairs", "records"])
def test_search_frame(mods, monkeypatch, cause, lists_only, page_locked):
    """sgtd_search_frame on a batch that is repaired inside the call: lists_only against the oracle, the verified form
    against the same call on a handle that never overflowed"""
    oracle, manager, _ = mods
    c, sx = ov.stale_expected(oracle)
    exp = sx[0]
    q = c.query_descs(manager, 0)
    key = ("search_frame", lists_only)
    if key not in _CLEAN:
        h, _, _ = _stale_handle(manager, monkeypatch, {}, oracle)
        _CLEAN[key] = h.search_frame(q, capacity=exp["T"], lists_only=lists_only)
        assert h.stats()["overflowed"] == 0
        h.close()
    want = _CLEAN[key]
    g, _, _ = _stale_handle(manager, monkeypatch, _cause_env(cause, exp["T"]), oracle)
    for again in (False, True):
        tag = "search_frame/%s/lists_only %d/page_locked %d/again %d" % (cause, lists_only, page_locked, again)
        before = _totals(g)
        out = g.search_frame(q, capacity=exp["T"], lists_only=lists_only, page_locked=page_locked)
        _check_repair(g, before, "none" if again else CAUSE_KIND[cause], tag)
        assert out["status"] == 0 and out["n_cand"] == want["n_cand"] == len(exp["cand_frame"]) and out["n_inliers"] == want["n_inliers"], tag
        for kk in FRAME_KEYS:
            np.testing.assert_array_equal(_bits(out[kk]) if out[kk].dtype == np.float64 else out[kk], _bits(want[kk]) if want[kk].dtype == np.float64 else want[kk],
                                          err_msg=tag + " " + kk)
        for f in ov.FIELDS:
            np.testing.assert_array_equal(getattr(out["entries"], f), getattr(want["entries"], f), err_msg=tag + " " + f)
        nc = out["n_cand"]
        np.testing.assert_array_equal(out["cand_frame"][:nc], exp["cand_frame"], err_msg=tag)
        np.testing.assert_array_equal(out["pair_off"][:nc + 1], exp["cand_off"], err_msg=tag)
        if lists_only:
            np.testing.assert_array_equal(out["inlier_q_idx"], exp["q_idx"], err_msg=tag)
            for f in ov.FIELDS:
                np.testing.assert_array_equal(getattr(out["entries"], f), exp["entries"][f], err_msg=tag + " " + f)
        _check_votes(g, 0, exp, tag)
        _check_stats(g, [exp], tag)
    g.close()


RADIUS, ALIGN_ITER = 1.0, 5


def _stage_results(g, stage, answers):
    """everything `stage` reports for every query of the batch that is pending on g, read through it alone"""
    out = []
    g.verify()
    if stage == "refine":
        g.refine_poses(2)
    elif stage == "overlap":
        g.overlap(RADIUS)
    elif stage == "align":
        g.align_keypoints(RADIUS, iterations=ALIGN_ITER)
    if stage == "verify":
        out.append(g.search_loop())
    for q, a in enumerate(answers):
        if stage == "verify":
            out.append(g.result_verify(q))
            off, qi, ent = g.result_inlier_entries(q, a["T"])
            out.append((off, qi) + tuple(getattr(ent, f) for f in ov.FIELDS))
        elif stage == "refine":
            r = g.result_refined(q)
            out.append(tuple(r[k] for k in sorted(r)))
        elif stage == "overlap":
            r = g.result_overlap(q)
            out.append(tuple(r[k] for k in sorted(r)))
        else:
            r = g.result_aligned(q)
            out.append(tuple(r[k] for k in sorted(r)))
    return out


def _same(a, b, tag):
    assert len(a) == len(b), tag
    for i, (x, y) in enumerate(zip(a, b)):
        for j, (u, v) in enumerate(zip(x, y)):
            u, v = np.asarray(u), np.asarray(v)
            assert u.dtype == v.dtype and u.shape == v.shape, (tag, i, j)
            if u.dtype.kind == "f":      # (bit for bit, NaN included)
                np.testing.assert_array_equal(u.view(np.uint64 if u.dtype == np.float64 else np.uint32),
                                              v.view(np.uint64 if v.dtype == np.float64 else np.uint32), err_msg="%s %d %d" % (tag, i, j))
            else:
                np.testing.assert_array_equal(u, v, err_msg="%s %d %d" % (tag, i, j))


def _check_stage_reference(h, stage, fe):
    """the stage's results for query 0 on the handle that never overflowed against the stage's numpy restatement
    (tests/_refine_ref.py, _overlap_ref.py, _align_ref.py), fed as tests/test_gpu_refine.py, test_gpu_overlap.py and
    test_gpu_align.py feed them: verify()'s poses, the batch's pairs, inliers and entries, the query's and the candidate
    frames' keypoints"""
    m, qs = fe["map"], fe["queries"]
    res = h.results()
    cn = h.config_setting_["candidate_num"]

    def frame_kp(f):
        return m.xyz[f], m.label[f]
    if stage == "refine":
        import test_gpu_refine as t_refine
        exp, _ = t_refine._expected(h, res, 0, 2)
        stats = t_refine._stats()
        t_refine._compare(h.result_refined(0), exp, cn, "clean", stats)
        assert stats["verified"] > 0
    elif stage == "overlap":
        import test_gpu_overlap as t_overlap
        tally = []
        t_overlap._check_query(h, res, 0, RADIUS, False, qs.xyz[0], qs.label[0], frame_kp, "clean", tally)
        assert tally and sum(e["n_hit_query"] for e in tally) > 0
    elif stage == "align":
        import test_gpu_align as t_align
        tally = {}
        t_align._check_query(h, int(res.n_cand[0]), res.cand_frame[0], 0, RADIUS, ALIGN_ITER, False, qs.xyz[0], qs.label[0],
                             frame_kp, "clean", tally)
        assert tally["verified"] > 0 and tally["compared"] > 0


@pytest.mark.parametrize("stage", ["verify", "refine", "overlap", "align"])
@pytest.mark.parametrize("cause", ["pairs", "records"])
def test_stages_behind_a_repaired_batch(mods, monkeypatch, cause, stage):
    """a batch enqueued with fetch=False and read only through the stage: the stage waits for the batch, which repairs it,
    and then reports what it reports on a handle that never overflowed — whose results for one query in turn equal the
    oracle's verification and the numpy restatements of the refit, the overlap and the alignment"""
    oracle, manager, synth = mods
    fe = ov.frame_expected(oracle, synth)
    qs, ans = fe["queries"], fe["answers"]
    if stage not in _CLEAN:
        h = _frame_handle(manager, monkeypatch, {}, fe, keypoints=True)
        h.query_frames(qs.xyz, qs.label, fetch=False)
        _CLEAN[stage] = _stage_results(h, stage, ans)
        assert h.stats()["overflowed"] == 0
        _check_stage_reference(h, stage, fe)
        if stage == "verify":
            o = oracle.OracleManager()
            for d in fe["descs"]:
                o.add(d)
            o.set_current_frame_id(len(fe["descs"]))
            o.build(qs.xyz[0], qs.label[0], export=False)
            r = o.select()
            score, rot, t = _CLEAN[stage][1]
            for k in range(len(r["cand_frame"])):
                s, o_t, o_rot, _ = o.verify(k, int(r["cand_off"][k + 1] - r["cand_off"][k]))
                assert score[k] == s and (s < 0 or (np.array_equal(t[k], o_t) and np.array_equal(rot[k], o_rot))), k
        h.close()
    T = sum(a["T"] for a in ans)
    g = _frame_handle(manager, monkeypatch, _cause_env(cause, T), fe, keypoints=True)
    tag = "%s behind %s" % (stage, cause)
    before = _totals(g)
    g.query_frames(qs.xyz, qs.label, fetch=False)
    _same(_stage_results(g, stage, ans), _CLEAN[stage], tag)
    _check_repair(g, before, CAUSE_KIND[cause], tag)
    before = _totals(g)
    g.query_frames(qs.xyz, qs.label, fetch=False)
    _same(_stage_results(g, stage, ans), _CLEAN[stage], tag + " again")
    _check_repair(g, before, "none", tag + " again")
    _check_batch(g, ans, tag)
    g.close()


@pytest.mark.parametrize("mode", ["auto", "mode2"])
@pytest.mark.parametrize("what", ["filter", "prior"])
@pytest.mark.parametrize("cause", ["pairs", "records"])
def test_filter_and_prior_survive_the_rerun(mods, monkeypatch, cause, what, mode):
    """a batch keeps the rows it was enqueued with, re-runs included: the repaired batch is the filtered answer (the filter
    is cleared again before the batch is waited for)"""
    oracle, manager, synth = mods
    fe = ov.frame_expected(oracle, synth)
    qs = fe["queries"]
    if what == "filter":
        allowed, ans, emap = fe["filtered"]
    else:
        center, radius, allowed, ans, emap = fe["prior"]
    T = sum(a["T"] for a in ans)
    g = _frame_handle(manager, monkeypatch, dict(MODES[mode], **_cause_env(cause, T)), fe, poses=what == "prior")

    def enqueue():
        if what == "filter":
            g.query_frames(qs.xyz, qs.label, fetch=False, allowed=allowed)
        else:
            g.query_frames(qs.xyz, qs.label, fetch=False, prior=(center, radius))
    _twice(g, enqueue, ans, CAUSE_KIND[cause], "%s/%s/%s" % (what, cause, mode), emap=emap)
    g.close()


@pytest.mark.parametrize("skip", [0, 2])
@pytest.mark.parametrize("cause", ["pairs", "records", "groups"])
def test_loop_frames(mods, monkeypatch, cause, skip):
    """sgtd_loop_frames in one chunk: the re-run builds the session's frames again but adds them once — the results are the
    oracle's sequential loop, and the frame counter, the frames and the entries are those of a handle that never overflowed"""
    oracle, manager, synth = mods
    m, ses, sels = ov.loop_expected(oracle, synth, skip)
    n = ses.xyz.shape[0]
    key = ("loop", skip)
    if key not in _CLEAN:
        h = manager.STDescManager()
        h.add_frames(m.xyz, m.label)
        h.loop_frames(ses.xyz, ses.label, skip_near=skip, batch=n)
        st = h.stats()
        assert st["overflowed"] == 0
        _CLEAN[key] = (h.current_frame_id_, st["n_frames"], st["n_entries"])
        h.close()
    T = sum(s["T"] for s in sels)
    g = _new(manager, monkeypatch, _cause_env(cause, T))
    g.add_frames(m.xyz, m.label)
    tag = "loop/%s/skip %d" % (cause, skip)
    before = _totals(g)
    g.loop_frames(ses.xyz, ses.label, skip_near=skip, batch=n, fetch=False)
    _check_batch(g, sels, tag, votes=False)
    _check_repair(g, before, CAUSE_KIND[cause], tag)
    for q in (0, n // 2, n - 1):
        _check_votes(g, q, sels[q], tag)
    st = g.stats()
    assert (g.current_frame_id_, st["n_frames"], st["n_entries"]) == _CLEAN[key], tag
    g.close()


@pytest.mark.parametrize("cause", ["pairs", "records"])
def test_view_under_the_hook_beside_its_owners_batch(mods, monkeypatch, cause):
    """a view created under the hook on an owner created without it, the owner's own batch in flight: the view's batch is
    repaired in the view's buffers, both answers are right and the owner has seen no overflow"""
    import torch
    oracle, manager, synth = mods
    fe = ov.frame_expected(oracle, synth)
    qs, ans = fe["queries"], fe["answers"]
    T = sum(a["T"] for a in ans)
    own = _frame_handle(manager, monkeypatch, {}, fe)
    own.finalize()
    view = _new(manager, monkeypatch, _cause_env(cause, T))
    stream = torch.cuda.Stream()
    view.set_stream(stream.cuda_stream)
    view.attach_table(own)
    rx, rl = np.ascontiguousarray(qs.xyz[::-1]), np.ascontiguousarray(qs.label[::-1])
    for again in (False, True):
        tag = "view/%s/again %d" % (cause, again)
        b_own, b_view = _totals(own), _totals(view)
        own.query_frames(rx, rl, fetch=False)                       # the owner's batch: the queries in reverse order
        view.query_frames(qs.xyz, qs.label, fetch=False)
        _check_batch(view, ans, tag)
        _check_repair(view, b_view, "none" if again else CAUSE_KIND[cause], tag)
        _check_batch(own, ans[::-1], tag + " owner")
        _check_repair(own, b_own, "none", tag + " owner")
    view.close()
    own.close()


def test_some_shards_of_a_multi_device_handle_rewrite(mods, monkeypatch):
    """devices=[0, 0, 0] with SGTD_PAIR_CAP between the shards' pair totals of the gate set: one shard rewrites, the others
    do not; the group's flag is the OR of the shards' and its counters their sums (batches_total: one shard's)"""
    oracle, manager, _ = mods
    g, wl, ex = _sel_handle(manager, monkeypatch, {"SGTD_PAIR_CAP": ov.MULTI_PAIR_CAP}, oracle, devices=[0, 0, 0])
    shards = ov.shard_expected(oracle)
    # a set no shard overflows on first: the flag is not stuck
    k0 = wl.tags["homes"][0]
    assert not any(ov.pairs_overflow(s[k0]["T"], ov.MULTI_PAIR_CAP) for s in shards)
    q0 = wl.query_descs(manager, k0)
    before = _totals(g)
    g.query_descs(q0)
    _check_batch(g, [ex[k0]], "multi/homes", multi=True)
    _check_repair(g, before, "none", "multi/homes", group=True)
    k = wl.tags["gate"][0]
    q = wl.query_descs(manager, k)
    n_over = sum(ov.pairs_overflow(s[k]["T"], ov.MULTI_PAIR_CAP) for s in shards)
    assert n_over == 1
    d = _twice(g, lambda: g.query_descs(q), [ex[k]], "rewrite", "multi/gate", flagged=n_over, multi=True)
    assert d["rewrites_total"] == n_over and d["batches_total"] == 1
    g.close()
    # every shard that holds records re-runs under SGTD_REC_CAP: the sums of the shards' counters
    g, wl, ex = _sel_handle(manager, monkeypatch, {"SGTD_REC_CAP": 1024}, oracle, devices=[0, 0, 0])
    d = _twice(g, lambda: g.query_descs(q), [ex[k]], "rerun", "multi/gate/records", multi=True)
    assert d["reruns_total"] >= 2
    g.close()


@pytest.mark.parametrize("cause", ["pairs", "records"])
def test_exchange_path_exports_the_flag_and_then_the_final_table(mods, monkeypatch, cause):
    """set_candidate_export + set_deferred_lists on a shard that overflows.  records: before sgtd_sync the packed table
    carries the flag and merge_candidates_dev reports it; after it the table is final and its serial has moved.  pairs: the
    export reads the batch's flag alone (export_candidates_kernel's `dead`), which the pair buffer never raises — the
    table is final when it is exported, the flag comes from the list pass of finish_lists, and the repair is a rewrite
    that exports nothing again"""
    import torch
    oracle, manager, synth = mods
    fe = ov.frame_expected(oracle, synth)
    qs, ans = fe["queries"], fe["answers"]
    nq = len(ans)
    T = sum(a["T"] for a in ans)
    g = _frame_handle(manager, monkeypatch, dict(_cause_env(cause, T), SGTD_SELECT_MODE="2"), fe)
    cn = g.config_setting_["candidate_num"]
    dev = torch.device("cuda", 0)
    packed = torch.zeros(2 * nq * cn + 4, dtype=torch.int32, device=dev)
    g.set_candidate_export(packed)
    g.set_deferred_lists(True)

    def merged():
        of = torch.empty((nq, cn), dtype=torch.int32, device=dev)
        ov_, osrc = torch.empty_like(of), torch.empty_like(of)
        on = torch.empty(nq, dtype=torch.int32, device=dev)
        keep = torch.empty(nq, dtype=torch.int64, device=dev)
        flags = torch.zeros(4, dtype=torch.int32, device=dev)
        g.merge_candidates_dev(0, packed.clone(), 1, 0, nq, of, ov_, on, osrc, keep, flags)
        torch.cuda.synchronize()
        return of.cpu().numpy(), ov_.cpu().numpy(), on.cpu().numpy(), keep, int(flags[0])

    def final(of, ovt, on):
        for q, a in enumerate(ans):
            nc = len(a["cand_frame"])
            assert int(on[q]) == nc
            np.testing.assert_array_equal(of[q, :nc], a["cand_frame"])
            np.testing.assert_array_equal(ovt[q, :nc], a["cand_votes"])
    before = _totals(g)
    g.query_frames(qs.xyz, qs.label, fetch=False)
    torch.cuda.synchronize()
    tail = packed[2 * nq * cn:].cpu().numpy()
    assert tail[0] == (1 if cause == "records" else 0) and tail[1] == nq and tail[2] == cn, tail
    serial = int(tail[3])
    if cause == "records":
        assert merged()[4] == 1
        g.sync()
        _check_repair(g, before, "rerun", "exchange")
        torch.cuda.synchronize()
        tail = packed[2 * nq * cn:].cpu().numpy()
        assert tail[0] == 0 and int(tail[3]) > serial, (tail, serial)
    of, ovt, on, keep, flag = merged()
    assert flag == 0
    final(of, ovt, on)
    g.finish_lists(keep)                              # (one table: every candidate is a winner)
    _check_batch(g, ans, "exchange/" + cause)
    if cause == "pairs":
        _check_repair(g, before, "rewrite", "exchange/pairs", flagged=0)
        torch.cuda.synchronize()
        tail = packed[2 * nq * cn:].cpu().numpy()
        assert tail[0] == 0 and int(tail[3]) == serial, (tail, serial)
    g.set_candidate_export(None)
    g.close()


@pytest.mark.parametrize("cause", ["pairs", "records"])
def test_two_batches_back_to_back_count_the_first_flag(mods, monkeypatch, cause):
    """batch A overflows and is never waited for; batch B is enqueued behind it: B's answer is right and
    overflow_launches_total has counted A's flag (the only trace of A's overflow, as include/sgtd_accel.h says).  records:
    B (the queries in reverse order) meets the same small buffer and is re-run.  pairs: B is the first half of the queries,
    whose pairs fit the buffer that A's did not: nothing is rewritten, for A or for B"""
    oracle, manager, synth = mods
    fe = ov.frame_expected(oracle, synth)
    qs, ans = fe["queries"], fe["answers"]
    T = sum(a["T"] for a in ans)
    g = _frame_handle(manager, monkeypatch, _cause_env(cause, T), fe)
    before = _totals(g)
    g.query_frames(qs.xyz, qs.label, fetch=False)                                                    # A
    if cause == "records":
        g.query_frames(np.ascontiguousarray(qs.xyz[::-1]), np.ascontiguousarray(qs.label[::-1]), fetch=False)   # B
        _check_batch(g, ans[::-1], "back to back")
    else:
        h = len(ans) // 2
        assert sum(a["T"] for a in ans[:h]) < T - 1
        g.query_frames(np.ascontiguousarray(qs.xyz[:h]), np.ascontiguousarray(qs.label[:h]), fetch=False)       # B
        _check_batch(g, ans[:h], "back to back")
    st = g.stats()
    d = {k: int(st[k] - before[k]) for k in TOTALS}
    if cause == "records":
        assert st["overflowed"] == 1 and d["reruns_total"] >= 1 and d["rewrites_total"] == 0, d
        assert d["batches_total"] == 2 + d["reruns_total"] and d["overflow_launches_total"] == 1 + d["reruns_total"], d
    else:
        assert st["overflowed"] == 0 and d == dict(batches_total=2, overflow_launches_total=1, reruns_total=0, rewrites_total=0), d
    g.close()
