"""The sweep's per-pass set-up at its edges in every form, against the oracle: candidates, their votes, pair_off, every match
list's (q_idx, db_entry) in order, the vote vector, P and M — exact equality, no tolerance.  Workloads: tests/_sweep_setup.py
(tests/test_sweep_setup.py shows that they reach their edges).

  families  widths (passes of 1 .. 4 descriptors and 4 + k, gates that differ per column), lengths (visit lists of 1 .. 4097
            entries), band (the undecided queue, fed by the header's ngap), room (SGTD_REC_SLAB=512 / SGTD_REC_RATE=1: a
            fresh slab for nearly every pass, lists that move; the same under a SGTD_REC_CAP that overflows and is re-run)
  forms     plain: one table segment; tail: the second half of the frames appended after finalize; frames: the queries
            carry the id of a frame the table holds (the sweep's FRAMES variant); loop: sgtd_loop_frames (the BOUND
            variant) — a loop batch is built from keypoints on the device, so its passes cannot be shaped descriptor by
            descriptor: it runs the keypoint session of tests/_overflow_edges.py under the default and the room hooks
  The WIDE variant needs a table above 4 GB: it is covered by compilation and the existing cfg4 tests only.

Run as a script (`python tests/test_gpu_sweep_setup.py small0`) it checks widths and lengths with SGTD_SMALL_ORDER=0 (read
once per process), under which a one-frame call takes the batch's general ordering.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _overflow_edges as ov  # noqa: E402
import _sweep_setup as ss  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = ("plain", "tail", "frames")
TOTALS = ("batches_total", "reruns_total", "rewrites_total", "list_moves_total")


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from sgtd_amd import manager, synth
    oracle.build_library()
    return oracle, manager, synth


def _new(manager, monkeypatch, env, **kw):
    """a handle created under the hooks `env` (each is read once per handle, in sgtd_create)"""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        return manager.STDescManager(**kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _handle(mods, monkeypatch, name, form, env):
    oracle, manager, _ = mods
    wl, ans, frames = ss.expected(oracle, name, held=form == "frames")
    g = _new(manager, monkeypatch, env, **ov.sel_config())
    if form == "tail":
        h = len(wl.adds) // 2
        wl.load(g, manager, 0, h)
        g.finalize()                                   # (the table is built: what follows goes to a tail segment)
        wl.load(g, manager, h, None)
    else:
        wl.load(g, manager)
    return g, wl, ans, frames


def _check(g, exp, tag, q=0, res=None):
    res = g.results() if res is None else res
    nc = len(exp["cand_frame"])
    assert int(res.n_cand[q]) == nc, tag
    np.testing.assert_array_equal(res.cand_frame[q, :nc], exp["cand_frame"], err_msg=tag)
    np.testing.assert_array_equal(res.cand_votes[q, :nc], exp["cand_votes"], err_msg=tag)
    np.testing.assert_array_equal(res.pair_off[q, :nc + 1], exp["cand_off"], err_msg=tag)
    qi, de = g.result_pairs(q, res)
    np.testing.assert_array_equal(qi, exp["q_idx"], err_msg=tag)
    np.testing.assert_array_equal(de, exp["db_entry"], err_msg=tag)
    lo, v = g.result_votes(q)
    want = exp["votes"]
    n = min(len(v), len(want) - lo)
    np.testing.assert_array_equal(v[:n].astype(np.float64), want[lo:lo + n], err_msg=tag)
    assert v[n:].sum() == 0 and want[:lo].sum() == 0 and want[lo + n:].sum() == 0, tag
    return res


TAIL_BATCHES = 4      # a handle merges its tail segment into the table at its fifth batch on it (settle_tail)


def _run_sets(mods, monkeypatch, name, form, sets=None, env={}):
    """every set of the workload through one handle (tail: a fresh one every TAIL_BATCHES sets, so that each set meets a
    tail segment); -> (the handles' counters' movement, the last handle's stats)"""
    _, manager, _ = mods
    g, d, st = None, {k: 0 for k in TOTALS}, None

    def done():
        for k in TOTALS:
            d[k] += int(g.stats()[k] - before[k])
        g.close()

    wl, ans, frames = None, ss.expected(mods[0], name, held=form == "frames")[1], None
    for i, k in enumerate(ans if sets is None else sets):
        if g is None or (form == "tail" and i % TAIL_BATCHES == 0):
            if g is not None:
                done()
            g, wl, ans, frames = _handle(mods, monkeypatch, name, form, env)
            before = {t: g.stats()[t] for t in TOTALS}
        tag = "%s/%s/set %d %s" % (name, form, k, env)
        g.query_descs(ss.query_descs(wl, manager, k, frames[k]))
        _check(g, ans[k], tag)
        st = g.stats()
        assert st["last_M"] == ans[k]["M"] and st["last_D"] == ans[k]["D"], tag
        assert st["last_cand_pairs"] == ans[k]["T"], tag
        if name == "lengths":      # (the BOOST descriptor's cell has no bucket on this table: the set's one pass is the list)
            assert st["last_P"] == ss.LENGTHS[k] and st["last_P_swept"] == ss.LENGTHS[k], (tag, st["last_P"], st["last_P_swept"])
        if form == "tail":
            assert st["tail_entries"] > 0, tag
    done()
    return d, st


@pytest.mark.parametrize("form", FORMS)
def test_pass_widths(mods, monkeypatch, form):
    oracle = mods[0]
    wl = ss.expected(oracle, "main")[0]
    _run_sets(mods, monkeypatch, "main", form, wl.tags["widths"])


@pytest.mark.parametrize("form", FORMS)
def test_visit_list_lengths(mods, monkeypatch, form):
    _run_sets(mods, monkeypatch, "lengths", form)


@pytest.mark.parametrize("form", FORMS)
def test_undecided_band(mods, monkeypatch, form):
    """the shell sets (matches at the threshold to within ulps) under the default buffers, and a queue one entry too small
    for the records the f32 pre-test cannot decide: the re-run shows that the queue was fed, the answer that every queued
    record was decided exactly"""
    oracle = mods[0]
    wl = ss.expected(oracle, "main")[0]
    _run_sets(mods, monkeypatch, "main", form, wl.tags["shell"][:2])
    cap = ov.queue_entries(ov.QUEUE_REC_CAP, 1)
    n = cap + 2 if form == "frames" else cap + 1       # (frames: the entry of the frame the query carries is not a record)
    d, st = _run_sets(mods, monkeypatch, n, form, env=ss.QUEUE_ENV)
    assert d["reruns_total"] >= 1 and st["overflowed"] == 1, d
    d, st = _run_sets(mods, monkeypatch, n, form, env={"SGTD_REC_CAP": ov.QUEUE_REC_CAP})      # the default floor: it fits
    assert d["reruns_total"] == 0 and st["overflowed"] == 0, d


@pytest.mark.parametrize("form", FORMS)
def test_room(mods, monkeypatch, form):
    oracle = mods[0]
    wl, ans, _ = ss.expected(oracle, "main", held=form == "frames")
    k = wl.tags["gate"][0]
    d, st = _run_sets(mods, monkeypatch, "main", form, [k] + wl.tags["widths"], env=ss.ROOM_ENV)
    assert d["list_moves_total"] > 0, d
    # ... and a record buffer of half the set's matches: the sweep overflows (new_slab or make_room) and sgtd_sync re-runs it
    cap = max(ov.HOOKS["SGTD_REC_CAP"][0], ans[k]["M"] // 2)
    assert ov.records_must_overflow(ans[k]["M"], cap)
    d, st = _run_sets(mods, monkeypatch, "main", form, [k], env=dict(ss.ROOM_ENV, SGTD_REC_CAP=cap))
    assert d["reruns_total"] >= 1 and d["reruns_total"] < ov.MAX_ATTEMPTS - 1 and st["overflowed"] == 1, d
    assert d["list_moves_total"] > 0, d


@pytest.mark.parametrize("room", [False, True])
def test_loop_batch(mods, monkeypatch, room):
    """sgtd_loop_frames in one chunk (BOUND): the oracle's sequential loop, under the default hooks and the room hooks"""
    oracle, manager, synth = mods
    m, ses, sels = ov.loop_expected(oracle, synth, 0)
    n = ses.xyz.shape[0]
    g = _new(manager, monkeypatch, ss.ROOM_ENV if room else {})
    g.add_frames(m.xyz, m.label)
    g.loop_frames(ses.xyz, ses.label, skip_near=0, batch=n, fetch=False)
    res = g.results()
    for q in range(n):
        _check(g, sels[q], "loop/room %s/frame %d" % (room, q), q=q, res=res)
    st = g.stats()
    assert st["last_M"] == sum(s["M"] for s in sels)
    g.close()


def test_small_order_off_in_a_process_of_its_own():
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "small0"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, SGTD_SMALL_ORDER="0"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "small0 ok" in p.stdout


class _Env:
    """monkeypatch's two calls, for the script"""

    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k):
        del os.environ[k]


if __name__ == "__main__":
    if sys.argv[1:] == ["small0"]:
        assert os.environ.get("SGTD_SMALL_ORDER") == "0"
        from oracle import oracle
        from sgtd_amd import manager, synth
        oracle.build_library()
        ms = (oracle, manager, synth)
        for form in FORMS:
            _run_sets(ms, _Env(), "main", form, ss.expected(oracle, "main")[0].tags["widths"])
            _run_sets(ms, _Env(), "lengths", form)
        print("small0 ok")
