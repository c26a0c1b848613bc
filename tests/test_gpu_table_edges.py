"""The hash-table build (build_idmap, build_segment, copy_in of sgtd_accel.hip; table_kernels.hip.h) at its structural
edges, in every form in which a table comes to exist, against the oracle.  Workloads: tests/_table_edges.py.

  forms   one_call (one AddSTDescs); per_frame (one call per frame, one finalize); tail (finalize and query, then append);
          tail_moved (SGTD_TAIL_MAX large: no room reserved, the tail's build moves the layout); tail_merged (SGTD_TAIL_MAX
          1: the append merges); aged_tail (four unchanged batches merge the tail); loaded (save_table, load_table into a
          fresh handle, append); removed (decoy frames interleaved, then remove_frames); multi (a three-shard handle on
          one GPU: queries only); view (attach_table: queries through the view, the dump through the owner)
  checks  stats (n_entries, n_buckets, tail_entries), then the census — one query descriptor per bucket: result_rough
          (q_idx, cell, db_entry, frame, dis), result_votes, the candidates with their votes and result_pairs (at most
          44 frames) — then fetch_entries of every insertion index (seven fields, bit patterns), then table_dump (keys,
          bucket offsets, entry ids).  The dump sorts a bucket's ids and result_rough orders a descriptor's matches by
          (cell, entry id) itself, so the order inside a bucket (the sort's stability, the slice partition) is what the
          candidates' match lists (result_pairs) show.  All comparisons are exact.

Run as a script (`python tests/test_gpu_table_edges.py noblock`) it checks the cold_store workloads with
SGTD_COPY_IN_BLOCK=0.
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

import _select_edges as se  # noqa: E402
import _table_edges as te  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("side", "angle", "center", "vertex", "label", "frame", "node_id")
ROUGH_MAX = 4096          # result_rough orders every descriptor's matches by selection (quadratic): one descriptor's 32 768 matches take minutes
TAIL_ENV = {"tail_moved": "1000000", "tail_merged": "1"}
COMBOS = [(n, f) for n, c in te.cases().items() if n not in te.REFUSED for f in c.forms]

_EXPECT = {}


def _oracle_for(c):
    from oracle import oracle
    oracle.build_library()
    o = oracle.OracleManager(**{k: v for k, v in c.cfg.items() if k in oracle.DEFAULTS})
    for lo, hi in c.call_bounds():
        o.add(c.descs(oracle, lo, hi))
    return oracle, o


def expected(c):
    """the oracle's dump and its answer to every census of workload c, once"""
    if c.name not in _EXPECT:
        oracle, o = _oracle_for(c)
        out = dict(dump=o.table_dump(), census=[])
        for k in range(len(c.census())):
            sel = o.select(c.query_descs(oracle, k))
            sel.update(votes=o.votes(), M=o.counters()["M"], rough=o.rough_matches())
            ent = o.fetch_entries(sel["db_entry"])
            sel["entries"] = {f: getattr(ent, f).copy() for f in ("side", "label", "frame")}
            out["census"].append(sel)
        _EXPECT[c.name] = out
    return _EXPECT[c.name]


def the_case(name):
    """the workload; partition_counts/many_buckets sized for this device's launch of slice_partition_kernel"""
    c = te.cases()[name]
    if name == "partition_counts/many_buckets":
        import torch
        waves = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4
        if waves != te.WAVES_MI355X:
            c = te.partition_many(waves)
            c.name += "/%d" % waves
    return c


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _add(g, mod, c, bounds):
    for lo, hi in bounds:
        g.AddSTDescs(c.descs(mod, lo, hi, null_bare=True))


def _check_votes(g, exp, tag):
    lo, v = g.result_votes(0)
    ov = exp["votes"]
    n = max(min(len(v), len(ov) - lo), 0)
    np.testing.assert_array_equal(v[:n].astype(np.float64), ov[lo:lo + n], err_msg=tag)
    assert v[n:].sum() == 0 and ov[:lo].sum() == 0 and ov[lo + n:].sum() == 0, tag
    assert g.stats()["last_M"] == exp["M"], tag


def check_census(g, mod, c, exp, tag, multi=False):
    """every census of c through handle g against the oracle's answers"""
    for k, sel in enumerate(exp["census"]):
        t = "%s census %d" % (tag, k)
        g.query_descs(c.query_descs(mod, k))
        res = g.results()
        _check_votes(g, sel, t)
        if not multi and np.bincount(sel["rough"]["q_idx"], minlength=1).max() <= ROUGH_MAX:
            got, want = g.result_rough(0), sel["rough"]
            for key in ("q_idx", "cell", "db_entry", "frame"):
                np.testing.assert_array_equal(got[key], want[key], err_msg="%s rough %s" % (t, key))
            np.testing.assert_array_equal(_bits(got["dis"]), _bits(want["dis"]), err_msg=t + " rough dis")
        if c.n_frames() > se.MAX_SET:
            continue
        nc = int(res.n_cand[0])
        assert nc == len(sel["cand_frame"]), t
        np.testing.assert_array_equal(res.cand_frame[0, :nc], sel["cand_frame"], err_msg=t)
        np.testing.assert_array_equal(res.cand_votes[0, :nc], sel["cand_votes"], err_msg=t)
        np.testing.assert_array_equal(res.pair_off[0, :nc + 1], sel["cand_off"], err_msg=t)
        qi, de = g.result_pairs(0, res)
        np.testing.assert_array_equal(qi, sel["q_idx"], err_msg=t)
        if multi:                                        # (the entry ids are the shards' own: the same entries)
            ent = g.fetch_entries(de)
            for f in ("side", "label", "frame"):
                np.testing.assert_array_equal(getattr(ent, f), sel["entries"][f], err_msg="%s %s" % (t, f))
        else:
            np.testing.assert_array_equal(de, sel["db_entry"], err_msg=t)


def check_entries(g, c, tag):
    """fetch_entries of every insertion index: all seven fields as bit patterns"""
    if c.E == 0:
        return
    got = g.fetch_entries(np.arange(c.E, dtype=np.int64))
    want = dict(side=c.side, label=c.label, frame=c.frame, **c.optional())
    for f in FIELDS:
        a, b = getattr(got, f), want[f]
        assert a.dtype == b.dtype, (tag, f)
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="%s entries %s" % (tag, f))


def check_dump(g, c, exp, tag):
    keys, off, ids = g.table_dump()
    for a, b, what in zip((keys, off, ids), exp["dump"], ("keys", "bucket_off", "entry ids")):
        np.testing.assert_array_equal(a, b, err_msg="%s dump %s" % (tag, what))
    st = g.stats()
    assert (st["n_entries"], st["n_buckets"], st["tail_entries"]) == (c.E, len(exp["dump"][0]), 0), tag


def check_all(g, mod, c, tag, tail=0, owner=None):
    exp = expected(c)
    st = g.stats()
    assert st["n_entries"] == c.E, tag
    check_census(g, mod, c, exp, tag)
    st = g.stats()
    assert st["tail_entries"] == tail, (tag, st["tail_entries"], tail)
    if tail == 0 and exp["census"]:
        assert st["n_buckets"] == len(exp["dump"][0]), tag
    check_entries(g, c, tag)
    check_dump(owner or g, c, exp, tag)
    if tail:                                             # (the dump merged the tail: the merged table answers the same)
        check_census(g, mod, c, exp, tag + " after the dump")


def _decoys(c, mod, k, n):
    """decoy frame k: n copies of the workload's entries (their buckets) under a frame id above the workload's"""
    d = mod.Descs(n)
    at = (np.arange(n) * 7 + k) % c.E
    d.side[:], d.label[:], d.frame[:] = c.side[at], c.label[at], c.free_frames()[k]
    return d


def run_form(name, form, tmp_path=None):
    from sgtd_amd import manager
    c = the_case(name)
    tag = "%s/%s" % (c.name, form)
    cut = c.cut_entry()
    made = []

    def new(**kw):
        g = manager.STDescManager(**dict(c.cfg, **kw))
        made.append(g)
        return g

    owner, tail = None, 0
    if form == "one_call":
        g = new()
        _add(g, manager, c, [(0, c.E)] if c.E else [])
    elif form == "per_frame":
        g = new()
        _add(g, manager, c, c.run_bounds())
        g.finalize()
    elif form in ("tail", "tail_moved", "tail_merged", "aged_tail"):
        g = new()                                        # (SGTD_TAIL_MAX is read when the handle is created)
        _add(g, manager, c, c.run_bounds(0, cut))
        g.finalize()
        g.query_descs(c.query_descs(manager, 0))         # the table is built and has answered: what follows is appended
        g.results()
        assert g.stats()["tail_entries"] == 0, tag
        _add(g, manager, c, c.run_bounds(cut, c.E))
        tail = c.expected_tail(int(TAIL_ENV[form]) if form in TAIL_ENV else None)
        if form == "aged_tail":
            exp = expected(c)
            g.query_descs(c.query_descs(manager, 0))
            g.results()
            assert g.stats()["tail_entries"] == tail, tag
            for _ in range(4):                           # SGTD_TAIL_BATCHES unchanged batches: the next one merges
                check_census(g, manager, c, dict(exp, census=exp["census"][:1]), tag + " ageing")
            tail = 0
    elif form == "loaded":
        first = new()
        _add(first, manager, c, c.run_bounds(0, cut))
        first.finalize()
        path = os.path.join(str(tmp_path), "edges.tbl")
        first.save_table(path)
        g = new()
        g.load_table(path)
        g.finalize()                                     # the loaded table is built; the append then tails or rebuilds like any other
        assert g.stats()["tail_entries"] == 0, tag
        _add(g, manager, c, c.run_bounds(cut, c.E))
        tail = c.expected_tail()
    elif form == "removed":
        g = new()
        runs = c.run_bounds()
        mid = len(runs) // 2
        g.AddSTDescs(_decoys(c, manager, 0, 37))
        _add(g, manager, c, runs[:mid])
        g.AddSTDescs(_decoys(c, manager, 1, 64))
        g.finalize()                                     # (a built table, then more, then the removal)
        _add(g, manager, c, runs[mid:])
        g.AddSTDescs(_decoys(c, manager, 2, 1))
        assert g.remove_frames(c.free_frames()) == 37 + 64 + 1, tag
    elif form == "multi":
        g = manager.STDescManager(devices=[0, 0, 0], **c.cfg)
        made.append(g)
        _add(g, manager, c, c.run_bounds())
        check_census(g, manager, c, expected(c), tag, multi=True)
        g.close()
        return
    elif form == "view":
        owner = new()
        _add(owner, manager, c, c.run_bounds())
        owner.finalize()
        g = new()
        g.attach_table(owner)
    else:
        raise AssertionError(form)
    check_all(g, manager, c, tag, tail=tail, owner=owner)
    for h in reversed(made):
        h.close()


@pytest.mark.parametrize("name, form", COMBOS, ids=["%s-%s" % nf for nf in COMBOS])
def test_every_form_equals_the_oracle(name, form, monkeypatch, tmp_path):
    if form in TAIL_ENV:
        monkeypatch.setenv("SGTD_TAIL_MAX", TAIL_ENV[form])
    run_form(name, form, tmp_path)


@pytest.mark.parametrize("form", ["one_call", "per_frame"])
def test_span_past_the_entry_id_is_refused(form):
    """12 rank bits and a frame span of 2^20 - 1: SGTD_ERR_UNSUPPORTED with the "entry id" message, never an answer (one
    frame id less is answered: id_bits/span_2p20m2)"""
    from sgtd_amd import manager
    c = te.cases()[te.REFUSED[0]]
    g = manager.STDescManager(**c.cfg)
    _add(g, manager, c, [(0, c.E)] if form == "one_call" else c.run_bounds())
    with pytest.raises(manager.SgtdError) as ei:
        g.candidate_selector(c.query_descs(manager, 0))
    assert ei.value.status == -6 and "entry id" in str(ei.value)
    g.close()


def test_scan_deep_dump():
    """2048 * 2048 + 1 entries in one call: device_scan's second recursion (the head flags' block sums need two blocks);
    side, label and frame only; the dump against the vectorised restatement"""
    from sgtd_amd import manager
    c = te.scan_deep()
    g = manager.STDescManager(**c.cfg)
    _add(g, manager, c, [(0, c.E)])
    keys, off, ids = g.table_dump()
    for a, b, what in zip((keys, off, ids), c.structure(), ("keys", "bucket_off", "entry ids")):
        np.testing.assert_array_equal(a, b, err_msg="scan_deep " + what)
    st = g.stats()
    assert (st["n_entries"], st["n_buckets"], st["tail_entries"]) == (c.E, len(keys), 0)
    g.close()


def test_copy_in_block_off_in_a_process_of_its_own():
    """SGTD_COPY_IN_BLOCK=0 (read once per process): every field of every call is copied on its own"""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "noblock"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, SGTD_COPY_IN_BLOCK="0"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "noblock ok" in p.stdout


@pytest.mark.parametrize("total", [te.REMOVE_TILE - 1, te.REMOVE_TILE, te.REMOVE_TILE + 1])
@pytest.mark.parametrize("which", ["first", "last", "every_other"])
def test_removal_at_the_tile_boundary(total, which):
    """a table of 1023 / 1024 / 1025 entries (the removal's tiles hold 1024) loses its first frame, its last, or every other
    one: what is left equals the oracle's table of the kept frames"""
    from sgtd_amd import manager
    full = te.pooled("removal/E%d" % total, total, 900 + total, n_frames=8, per_key=9)
    frames = sorted(set(full.frame.tolist()))
    gone = {"first": frames[:1], "last": frames[-1:], "every_other": frames[::2]}[which]
    keep = ~np.isin(full.frame, gone)
    c = te.Case("removal/E%d_%s" % (total, which), te.per_frame_calls(full.side[keep], full.label[keep], full.frame[keep]))
    g = manager.STDescManager(**c.cfg)
    for lo, hi in full.run_bounds():
        g.AddSTDescs(_one(manager, full.side[lo:hi], full.label[lo:hi], full.frame[lo:hi]))
    g.finalize()
    assert g.stats()["n_entries"] == total
    assert g.remove_frames(gone) == int((~keep).sum())
    exp = expected(c)
    check_census(g, manager, c, exp, c.name)
    got = g.fetch_entries(np.arange(c.E, dtype=np.int64))
    for f in ("side", "label", "frame"):
        np.testing.assert_array_equal(_bits(getattr(got, f)), _bits(getattr(c, f)), err_msg=f)
    check_dump(g, c, exp, c.name)
    g.close()


def _one(mod, side, label, frame):
    d = mod.Descs(len(side))
    d.side[:], d.label[:], d.frame[:] = side, label, frame
    return d


def test_empty_emptied_and_refilled():
    """an empty table answers nothing; a table emptied by remove_frames answers nothing and, refilled, like a new one"""
    from sgtd_amd import manager
    c = te.cases()["sort_counts/E257"]
    g = manager.STDescManager(**c.cfg)
    for step in ("empty", "emptied"):
        if step == "emptied":
            _add(g, manager, c, c.run_bounds())
            g.finalize()
            assert g.remove_frames(sorted(set(c.frame.tolist()))) == c.E
        assert g.candidate_selector(c.query_descs(manager, 0)) == [] and g.stats()["last_M"] == 0, step
        st = g.stats()
        assert (st["n_entries"], st["n_buckets"], st["tail_entries"]) == (0, 0, 0), step
        keys, off, ids = g.table_dump()
        assert len(keys) == 0 and len(ids) == 0 and off.tolist() == [0], step
    # the refill: a call with NULL optional fields lands on rows that held data, so its zeros come from copy_in's memset
    n = te.cases()["cold_store/null_fields"]
    _add(g, manager, n, n.run_bounds())
    check_all(g, manager, n, "refilled")
    g.close()


@pytest.mark.parametrize("bad", [float("inf"), -2.0])
def test_a_side_outside_the_key_is_refused_and_the_handle_stays_usable(bad):
    from sgtd_amd import manager
    c = te.cases()["sort_counts/E65"]
    g = manager.STDescManager(**c.cfg)
    _add(g, manager, c, c.run_bounds())
    g.AddSTDescs(_one(manager, [[4.125, bad, 6.125]], [[1, 2, 3]], [int(c.frame.max()) + 1]))
    with pytest.raises(manager.SgtdError) as ei:
        g.candidate_selector(c.query_descs(manager, 0))
    assert ei.value.status == -6
    assert g.remove_frames([int(c.frame.max()) + 1]) == 1
    check_all(g, manager, c, "after the refused side %r" % bad)
    g.close()


def test_a_nan_side_matches_nothing_and_disturbs_nothing():
    """outside the reference's defined behaviour: only that the entry appears in no rough list and that every other
    entry's answers stay what they were"""
    from sgtd_amd import manager
    c = te.cases()["sort_counts/E257"]
    exp = expected(c)
    g = manager.STDescManager(**c.cfg)
    _add(g, manager, c, c.run_bounds())
    for ax in range(3):
        s = c.side[:1].copy()
        s[0, ax] = np.nan
        g.AddSTDescs(_one(manager, s, c.label[:1], [int(c.frame.max()) + 1 + ax]))
    assert g.stats()["n_entries"] == c.E + 3
    g.query_descs(c.query_descs(manager, 0))
    g.results()
    got, want = g.result_rough(0), exp["census"][0]["rough"]
    assert got["db_entry"].max() < c.E
    for key in ("q_idx", "cell", "db_entry", "frame"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    g.close()


if __name__ == "__main__":
    if sys.argv[1:] == ["noblock"]:
        assert os.environ.get("SGTD_COPY_IN_BLOCK") == "0"
        n = 0
        for name in ("cold_store/offsets", "cold_store/null_fields", "cold_store/block_switch"):
            for form in ("per_frame", "tail"):
                run_form(name, form)
                n += 1
        print("noblock ok: %d" % n)
