"""BuildSingleScanSTD at its edges in every form that reaches build_frames_kernel, against the oracle, bit for bit
(_build_edges.desc_bits_equal: -0.0 is not +0.0; two NaNs are equal).  Workloads: tests/_build_edges.py; that they reach
the edges, and that the oracle equals a second restatement on them, is tests/test_build_edges.py.

  forms   sgtd_build one frame at a time (the one-transfer output form, and the general one for the large frames);
          sgtd_add_frames on ragged batches, read back from the table; sgtd_query_frames on the same batches (the query
          descriptors, and candidate_selector's results for some of them: the sweep records the kernel writes);
          sgtd_loop_frames on a session of mixed frames; a two-shard handle on one GPU; SGTD_COPY_IN_BLOCK=0 and
          SGTD_FRAME_DIRECT=0 (read once per process: a process of its own)
  sizes   the frame one past the global form's limit is refused (SGTD_ERR_UNSUPPORTED) alone and inside a batch,
          65536 keypoints are SGTD_ERR_INVALID, and the handle answers afterwards

Run as a script (`python tests/test_gpu_build_edges.py knobs0`) it checks the descriptor input forms with both knobs off.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _build_edges as be  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = list(be.FAMILIES)
_EXPECT = {}


def mods():
    from oracle import oracle
    from sgtd_amd import manager
    oracle.build_library()
    return oracle, manager


def expected(name):
    """[(cfg, frames, the oracle's descriptors per frame, built as frame 0, 1, ... of an add_last sequence, the
    oracle's table dump after it)] of one family, once"""
    if name not in _EXPECT:
        oracle, _ = mods()
        out = []
        for cfg, frames in be.family(name):
            o = oracle.OracleManager(**cfg)
            descs = []
            for xyz, lab in frames:
                descs.append(o.build(xyz, lab))
                o.add_last()
            out.append((cfg, frames, descs, o.table_dump()))
        _EXPECT[name] = out
    return _EXPECT[name]


def same(got, want, tag, frame=None):
    """bit equality of every field; frame: the id the device's descriptors must carry instead of the oracle's"""
    fields = be.RefBuild.FIELDS if frame is None else tuple(f for f in be.RefBuild.FIELDS if f != "frame")
    assert be.desc_bits_equal(got, want, fields) == "", tag
    if frame is not None:
        assert np.all(got.frame[:got.n] == frame), tag


@pytest.mark.parametrize("name", FAMILIES)
def test_one_frame_at_a_time(name):
    _, manager = mods()
    n_desc = 0
    for c, (cfg, frames, descs, _) in enumerate(expected(name)):
        g = manager.STDescManager(**cfg)
        for k, ((xyz, lab), want) in enumerate(zip(frames, descs)):
            got = g.BuildSingleScanSTD(xyz, lab)
            same(got, want, "%s/cfg%d/frame%d n=%d" % (name, c, k, len(xyz)), frame=0)
            n_desc += got.n
        g.close()
    assert n_desc > 100


def _table_descs(g, n):
    return g.fetch_entries(np.arange(n, dtype=np.int64))


@pytest.mark.parametrize("name", FAMILIES)
def test_add_frames_on_ragged_batches(name):
    """one sgtd_add_frames call per config; the table's entries in insertion order are the frames' descriptors with frame
    ids 0, 1, ..., and the table's buckets are the oracle's"""
    _, manager = mods()
    for c, (cfg, frames, descs, dump) in enumerate(expected(name)):
        g = manager.STDescManager(**cfg)
        xyz, lab, off = be.batch_of(frames)
        g.add_frames(xyz, lab, kp_off=off)
        assert g.current_frame_id_ == len(frames)
        total = sum(d.n for d in descs)
        assert g.stats()["n_entries"] == total, (name, c)
        ent = _table_descs(g, total)
        at = 0
        for k, want in enumerate(descs):
            same(ent.take(np.arange(at, at + want.n)), want, "%s/cfg%d/frame%d n=%d" % (name, c, k, len(frames[k][0])))
            at += want.n
        if total:
            for a, b in zip(g.table_dump(), dump):
                np.testing.assert_array_equal(a, b, err_msg="%s/cfg%d table" % (name, c))
        g.close()


def _query_chunks(g, frames, limit=600):
    """(first frame, frames) of the query_frames calls that carry `frames`: at most sgtd_max_batch frames each (and at
    most `limit`: more than either grid the build launch chooses)"""
    step = int(max(1, min(limit, g.max_batch(max(len(f[0]) for f in frames)))))
    return [(k, frames[k:k + step]) for k in range(0, len(frames), step)]


@pytest.mark.parametrize("name", FAMILIES)
def test_query_frames_on_ragged_batches(name):
    _, manager = mods()
    for c, (cfg, frames, descs, _) in enumerate(expected(name)):
        g = manager.STDescManager(**cfg)
        for k0, part in _query_chunks(g, frames):
            xyz, lab, off = be.batch_of(part)
            g.query_frames(xyz, lab, kp_off=off)
            for q in range(len(part)):
                same(g.result_query_descs(q), descs[k0 + q], "%s/cfg%d/frame%d" % (name, c, k0 + q), frame=0)
        g.close()


SELECT_CASES = (("mixed_batches", 0), ("ties", 2), ("degenerate", 1), ("contention", 0))


@pytest.mark.parametrize("name,c", SELECT_CASES)
def test_query_frames_select_like_the_oracle(name, c):
    """the frames of one config as the map (add_frames), then the same frames as one query batch: candidates, votes,
    match lists and the rough list with its distances (what the kernel's sweep records feed)"""
    from test_gpu_parity import _check_query
    oracle, manager = mods()
    cfg, frames = be.family(name)[c]
    g, o = manager.STDescManager(**cfg), oracle.OracleManager(**cfg)
    xyz, lab, off = be.batch_of(frames)
    g.add_frames(xyz, lab, kp_off=off)
    for x, l in frames:
        o.build(x, l, export=False)
        o.add_last()
    res = g.query_frames(xyz, lab, kp_off=off)
    n_cand = 0
    for q in list(range(len(frames)))[:24]:
        want = o.build(*frames[q])
        r = _check_query(g, o, res, q, want)
        n_cand += len(r["cand_frame"])
    assert n_cand > 0
    g.close()


def test_loop_frames_on_a_mixed_session():
    """the first mixed batch twice over as one session: the second visit finds the first"""
    from test_gpu_loop_frames import _oracle_loop, _same_as_oracle
    oracle, manager = mods()
    cfg, frames = be.family("mixed_batches")[0]
    frames = frames + frames
    o = oracle.OracleManager(**cfg)
    descs = []
    for i, (x, l) in enumerate(frames):
        o.set_current_frame_id(i)
        descs.append(o.build(x, l))
    assert all(oracle.DEFAULTS[k] == v for k, v in cfg.items())      # (the helper's oracle has the shipped settings)
    sel, _, _ = _oracle_loop(oracle, descs, 0)
    g = manager.STDescManager(**cfg)
    xyz, lab, off = be.batch_of(frames)
    res = g.loop_frames(xyz, lab, kp_off=off, batch=len(frames))
    _same_as_oracle(g, res, sel)
    for q, want in enumerate(descs):
        assert g.result_query_descs(q).n == want.n, q
    assert g.stats()["n_entries"] == sum(d.n for d in descs)
    assert int(np.sum(res.n_cand > 0)) >= 5
    g.close()


def test_two_shard_handle_on_one_gpu():
    _, manager = mods()
    for c, (cfg, frames, descs, _) in enumerate(expected("ties")):
        g = manager.STDescManager(devices=[0, 0], **cfg)
        for k, ((xyz, lab), want) in enumerate(zip(frames, descs)):
            same(g.BuildSingleScanSTD(xyz, lab), want, "ties/cfg%d/frame%d" % (c, k), frame=0)
        xyz, lab, off = be.batch_of(frames)
        g.add_frames(xyz, lab, kp_off=off)
        assert g.stats()["n_entries"] == sum(d.n for d in descs)
        g.close()


def _build_status(g, manager, xyz, lab, n=None):
    d = manager.Descs(1)
    s = d.soa()
    n_out = C.c_int64(0)
    x = np.ascontiguousarray(xyz, np.float32)
    l = np.ascontiguousarray(lab, np.uint32)
    return g._L.sgtd_build(g._h, x.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p), len(x) if n is None else n,
                           C.byref(s), 1, C.byref(n_out))


@pytest.mark.parametrize("K", be.SWITCH_KS)
def test_refused_sizes(K):
    oracle, manager = mods()
    cfg = be.cfg_of(K, 0.5, 50.0)
    g, o = manager.STDescManager(**cfg), oracle.OracleManager(**cfg)
    small = be.random_frame(50, 3, K)
    big = be.refused_frame(K)
    assert len(big[0]) == be.largest_n(K) + 1

    def still_answers():
        same(g.BuildSingleScanSTD(*small), o.build(*small), "after a refusal", frame=g.current_frame_id_)

    assert _build_status(g, manager, *big) == -6                     # SGTD_ERR_UNSUPPORTED
    still_answers()
    xyz, lab, off = be.batch_of([small, big, small])
    for call in (g.add_frames, g.query_frames):
        with pytest.raises(manager.SgtdError) as ei:
            call(xyz, lab, kp_off=off)
        assert ei.value.status == -6
        still_answers()
    assert g.stats()["n_entries"] == 0
    huge = np.zeros((65536, 3), np.float32)
    assert _build_status(g, manager, huge, np.zeros(65536, np.uint32)) == -1      # SGTD_ERR_INVALID
    with pytest.raises(manager.SgtdError) as ei:
        g.add_frames(huge, np.zeros(65536, np.uint32), kp_off=np.array([0, 65536]))
    assert ei.value.status == -1
    still_answers()
    g.close()


def run_knobs_off():
    """descriptors built one frame at a time, handed to AddSTDescs (the field-by-field copy: SGTD_COPY_IN_BLOCK=0) and
    read back from the table; search_frame on one of them without the direct form (SGTD_FRAME_DIRECT=0)"""
    _, manager = mods()
    n = 0
    for name in ("equal_sides", "degenerate", "extras", "ties"):
        for c, (cfg, frames, descs, _) in enumerate(expected(name)):
            g = manager.STDescManager(**cfg)
            for xyz, lab in frames:
                d = g.BuildSingleScanSTD(xyz, lab)
                g.AddSTDescs(d)
            total = sum(d.n for d in descs)
            ent = _table_descs(g, total)
            at = 0
            for k, want in enumerate(descs):
                same(ent.take(np.arange(at, at + want.n)), want, "%s/cfg%d/frame%d" % (name, c, k))
                at += want.n
            q = g.BuildSingleScanSTD(*frames[0])
            if q.n:
                out = g.search_frame(q, lists_only=True)
                assert out["status"] == 0
            n += total
            g.close()
    return n


def test_descriptor_input_forms_with_the_knobs_off_in_a_process_of_its_own():
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "knobs0"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, SGTD_COPY_IN_BLOCK="0", SGTD_FRAME_DIRECT="0"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "knobs0 ok" in p.stdout


if __name__ == "__main__":
    if sys.argv[1:] == ["knobs0"]:
        assert os.environ.get("SGTD_COPY_IN_BLOCK") == "0" and os.environ.get("SGTD_FRAME_DIRECT") == "0"
        print("knobs0 ok: %d descriptors" % run_knobs_off())
