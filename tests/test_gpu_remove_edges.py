"""sgtd_remove_frames (remove_kernels.hip.h, remove_entries, multi::remove_frames) at its structural edges, in every form
of a handle.  Workloads: tests/_remove_edges.py (tests/test_remove_edges.py shows without a GPU that they are sharp).

  forms   answered (one segment that has answered a batch); unfinalized; loaded (save_table, load_table, remove); view
          (the owner removes, the view refuses and answers again once re-attached); add0 / add1 / add1025 (an AddSTDescs
          of that many entries after the removal); twice (every removal as two calls in a row); pending (a batch enqueued
          with fetch=False, then the removal); tail (a table with a tail segment); multi (a three-shard handle on one GPU,
          for the workloads whose calls carry the current frame id)
  checks  primary: fetch_entries of every surviving index, all seven fields as bit patterns, against numpy's field[keep].
          State: the count the call returns, stats()["n_entries"], current_frame_id_ unchanged, n_frames where every call
          is one frame, and result_votes' lo and length against the survivors' least and greatest frame.  Queries (the
          workloads marked `query`): the census and the dump of test_gpu_table_edges.py against the oracle holding the
          survivors alone.  All comparisons are exact.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _remove_edges as re_  # noqa: E402
import test_gpu_table_edges as gte  # noqa: E402

pytestmark = pytest.mark.gpu

W_ALL = re_.workloads()
COMBOS = [(n, f) for n, w in W_ALL.items() for f in w.forms]
ADD_N = dict(add0=0, add1=1, add1025=1025)
_SYNTH = {}


def _a_frame():
    """one small frame of keypoints (its answer is not looked at: it only leaves a batch pending)"""
    if not _SYNTH:
        from sgtd_amd import synth
        m = synth.make_map(2, 40, stream=977)
        _SYNTH["f"] = (m.xyz[:1], m.label[:1])
    return _SYNTH["f"]


def _fields_descs(mod, fields):
    d = mod.Descs(len(fields["frame"]))
    for f in re_.NAMES7:
        getattr(d, f)[...] = fields[f]
    return d


def _add(g, mod, w, bounds):
    for lo, hi in bounds:
        g.AddSTDescs(w.descs(mod, lo, hi))


def _ask_one(g, mod, fields, qframe):
    """a batch of one descriptor: the first of `fields`"""
    d = mod.Descs(1)
    d.side[:], d.label[:], d.frame[:] = fields["side"][:1], fields["label"][:1], qframe
    g.query_descs(d)
    return g.results()


def _check_words(got, want, tag):
    for f in re_.NAMES7:
        a, b = getattr(got, f), want[f]
        assert a.dtype == b.dtype and len(a) == len(b), (tag, f)
        x, y = re_.words(a), re_.words(b)
        if not np.array_equal(x, y):
            bad = np.flatnonzero((x != y).any(axis=1))
            raise AssertionError("%s: %s differs at %d of %d surviving entries, first at %d: got %s want %s"
                                 % (tag, f, len(bad), len(x), bad[0], x[bad[0]], y[bad[0]]))


def check_after(g, mod, w, surv, tag, current, n_calls=None, state=None, owner=None, case=None):
    """handle g after the removal: surv are the fields it must hold (state: the handle whose counters are read, owner: the
    handle that dumps, case: the survivors as the oracle's workload for the census)"""
    state = state or g
    E2 = len(surv["frame"])
    st = state.stats()
    assert st["n_entries"] == E2, (tag, st["n_entries"], E2)
    assert state.current_frame_id_ == current, tag
    if n_calls is not None:
        assert st["n_frames"] == n_calls, (tag, st["n_frames"], n_calls)
    if E2:
        _check_words(g.fetch_entries(np.arange(E2, dtype=np.int64)), surv, tag)
    # the surviving span, as the vote array of a batch shows it
    qframe = (int(surv["frame"].max()) if E2 else int(w.frame.max())) + 1
    _ask_one(g, mod, surv if E2 else w.fields(), qframe)
    lo, v = g.result_votes(0)
    f = surv["frame"].astype(np.int64)
    assert (lo, len(v)) == ((int(f.min()), int(f.max() - f.min()) + 1) if E2 else (0, 1)), (tag, lo, len(v))
    if E2 == 0:
        assert not v.any(), tag
        keys, off, ids = (owner or g).table_dump()
        assert len(keys) == 0 and len(ids) == 0 and off.tolist() == [0], tag
    elif case is not None:
        exp = gte.expected(case)
        gte.check_census(g, mod, case, exp, tag)
        gte.check_dump(owner or g, case, exp, tag)
    else:
        assert int(v[int(surv["frame"][0]) - lo]) >= 1, tag          # the descriptor finds its own entry


def _remove(g, w, steps, tag, kept=None):
    """the removal calls; every call returns the number of entries it took.  -> the keep mask afterwards"""
    kept = np.ones(w.E, bool) if kept is None else kept
    for k, s in enumerate(steps):
        hit = kept & np.isin(w.frame, np.asarray(s, np.int64).astype(np.uint32))
        assert g.remove_frames(np.asarray(s, np.int64).astype(np.uint32)) == int(hit.sum()), (tag, k)
        kept = kept & ~hit
    return kept


def _calls_left(w, kept, more=0):
    return (len(set(w.frame[kept].tolist())) + more) if w.per_frame else None


def run_form(name, form, tmp_path=None):
    from sgtd_amd import manager
    w = W_ALL[name]
    tag = "%s/%s" % (name, form)
    made = []

    def new(**kw):
        g = manager.STDescManager(**dict(w.cfg, **kw))
        made.append(g)
        return g

    case = (lambda extra=None, t="": w.case(None, extra, t) if w.query else None)
    first = w.cfg.get("first_frame_id", 0)
    current = first + len(w.bounds)
    full_q = int(w.frame.max()) + 1
    if form == "multi":
        g = new(devices=[0, 0, 0])
        _add(g, manager, w, w.bounds)
        g.finalize()
        kept = _remove(g, w, w.steps, tag)
        assert g.current_frame_id_ == current and g.stats()["n_entries"] == int(kept.sum()), tag
        assert g.stats()["n_frames"] == _calls_left(w, kept), tag
        shard = (w.frame.astype(np.int64) // re_.SHARD_BLOCK) % 3
        for s in range(3):                               # entry ids: shard << 40 | the shard's own insertion index
            idx = np.flatnonzero(kept & (shard == s))
            if len(idx):
                got = g.fetch_entries((s << 40) + np.arange(len(idx), dtype=np.int64))
                _check_words(got, {f: v[idx] for f, v in w.fields().items()}, "%s shard %d" % (tag, s))
        if w.query:
            c = case()
            gte.check_census(g, manager, c, gte.expected(c), tag, multi=True)
    elif form == "view":
        owner = new()
        _add(owner, manager, w, w.bounds)
        owner.finalize()
        g = new()
        g.attach_table(owner)
        _ask_one(g, manager, w.fields(), full_q)
        kept = _remove(owner, w, w.steps, tag)
        with pytest.raises(manager.SgtdError) as ei:     # a view cannot remove frames
            g.remove_frames(w.steps[-1])
        assert ei.value.status == -7, tag
        if (~kept).any():                                # and its owner's table is no longer the one it attached to
            with pytest.raises(manager.SgtdError) as ei:
                _ask_one(g, manager, w.fields(), full_q)
            assert ei.value.status == -7, tag
            g.attach_table(owner)
        check_after(g, manager, w, w.survivors(), tag, current, _calls_left(w, kept), state=owner, owner=owner, case=case())
    else:
        g = new()
        steps = re_.split_steps(w.steps) if form == "twice" else w.steps
        if form == "tail":
            _add(g, manager, w, w.bounds[:w.cut])
            g.finalize()
            _ask_one(g, manager, w.fields(), full_q)
            _add(g, manager, w, w.bounds[w.cut:])
            g.finalize()
            assert g.stats()["tail_entries"] == w.E - w.bounds[w.cut][0], tag
        else:
            _add(g, manager, w, w.bounds)
        if form == "loaded":
            g.finalize()
            path = os.path.join(str(tmp_path), "edges.tbl")
            g.save_table(path)
            g = new()
            g.load_table(path)
        elif form == "pending":
            g.finalize()
            g.query_frames(*_a_frame(), fetch=False)
        elif form not in ("unfinalized", "tail"):
            g.finalize()
            _ask_one(g, manager, w.fields(), full_q)
            assert g.stats()["tail_entries"] == 0, tag
        assert g.current_frame_id_ == current, tag
        if form == "answered" and len(w.steps) > 1:      # the state after every call, not only after the last
            kept = np.ones(w.E, bool)
            for k in range(len(w.steps)):
                kept = _remove(g, w, w.steps[k:k + 1], tag, kept)
                check_after(g, manager, w, w.survivors(k + 1), "%s step %d" % (tag, k), current, _calls_left(w, kept))
        else:
            kept = _remove(g, w, steps, tag)
        assert np.array_equal(kept, w.keep()), tag
        extra, more = None, 0
        if form in ADD_N:
            extra, more = w.added(ADD_N[form]), 1
            g.AddSTDescs(_fields_descs(manager, extra))
        check_after(g, manager, w, w.survivors(None, extra), tag, current + more, _calls_left(w, kept, more), case=case(extra, "/" + form if extra is not None else ""))
        assert g.stats()["tail_entries"] == 0 or kept.all(), tag     # (a call that removed nothing leaves a tail a tail)
    for h in reversed(made):
        h.close()


@pytest.mark.parametrize("name, form", COMBOS, ids=["%s-%s" % nf for nf in COMBOS])
def test_every_form_keeps_field_of_keep(name, form, tmp_path):
    run_form(name, form, tmp_path)


def test_more_tiles_than_workgroups_and_one_scan_block():
    """2048 x 1024 + 1 entries, about 290 MB of descriptors on the device: 2049 tiles, the last of one entry.  The flag
    kernel's grid is 4 workgroups per CU (1024 on 256 CUs), so every workgroup walks a second tile, and device_scan over
    the tile counts needs a second block (2048 counts per block).  No smaller table reaches either edge: both are counts
    of 1024-entry tiles.  One add, one removal, one fetch of all seven fields; no finalize"""
    from sgtd_amd import manager
    import torch
    w = re_.large()
    assert w.n_tiles() > 4 * torch.cuda.get_device_properties(0).multi_processor_count
    g = manager.STDescManager(**w.cfg)
    g.AddSTDescs(w.descs(manager, 0, w.E))
    keep = w.keep()
    assert g.remove_frames([re_.GO, re_.GO2]) == int((~keep).sum())
    assert g.stats()["n_entries"] == int(keep.sum()) and g.current_frame_id_ == 1
    got = g.fetch_entries(np.arange(int(keep.sum()), dtype=np.int64))
    _check_words(got, w.survivors(), "large")
    g.close()
