"""With the oracle alone: every family of tests/_sweep_setup.py reaches the edge it is named for (the GPU tests are
tests/test_gpu_sweep_setup.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _overflow_edges as ov  # noqa: E402
import _select_edges as se  # noqa: E402
import _sweep_setup as ss  # noqa: E402


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle
    oracle.build_library()
    return oracle


def test_widths_has_every_pass_width_and_gates_that_differ(oracle):
    wl, ans, _ = ss.expected(oracle, "main")
    sizes = []
    for k in wl.tags["widths"]:
        for cell, sides in ss.width_homes(wl.sets[k][0]).items():
            sizes.append(len(sides))
            masks = {ss.gate_mask(s) for s in sides}
            # (up to four descriptors of a home cell are ONE pass: its columns' gates differ per range)
            assert len(sides) == 1 or len(masks) >= 2, (cell, masks)
            assert ov.home_groups(sides, [ss.WIDTH_LABEL] * len(sides)) == 1          # one GroupRow: they share their passes
        assert ans[k]["M"] > 0 and len(ans[k]["cand_frame"]) > 0
    # R = 1, 2, 3, 4 as passes of their own, 5 .. 9 as a pass of four (or two) and a ragged last one
    assert sorted(sizes) == list(range(1, 10))


def test_lengths_are_the_visit_lists_lengths(oracle):
    wl, ents = ss.lengths_workload()
    _, ans, _ = ss.expected(oracle, "lengths")
    assert [len(e) for e in ents] == list(ss.LENGTHS)
    for i, n in enumerate(ss.LENGTHS):
        # one bucket, every entry in the sub-cell of the query: whatever the query's reach prunes, the list is the bucket
        assert {se.c_int(v + 0.5) for v in ents[i][:, 0]} == {3} and {se.sub_cell(s) for s in ents[i]} == {se.sub_cell(ss.LEN_Q)}
        o = oracle.OracleManager(**ov.sel_config())
        wl.load(o, oracle)
        o.select(ss.query_descs(wl, oracle, i))
        assert o.counters()["P"] == n, (n, o.counters())
        assert 0 < ans[i]["M"] < n or n == 1                   # (some of the entries match, some do not)
    # group tails of one, two and three words behind whole four-word groups, and the second window
    words = [(n + 63) // 64 for n in ss.LENGTHS]
    assert {w % 4 for w in words} == {0, 1, 2} and max(words) == 65 and 64 in words


def test_band_sets_have_matches_at_the_threshold(oracle):
    wl, ans, _ = ss.expected(oracle, "main")
    for k in wl.tags["shell"][:2]:
        near = ov.near_threshold(ans[k]["rough"], wl.sets[k][0], ss.ROUGH)
        assert near.sum() > 0
        assert ov.band_rel(wl.sets[k][0][0], ss.ROUGH) > ov.NEAR_REL          # inside the f32 pre-test's band: queued
    cap = ov.queue_entries(ov.QUEUE_REC_CAP, 1)
    for n, held in ((cap + 1, False), (cap + 2, True)):
        wl, a, frames = ss.expected(oracle, n, held)
        ents = ov.queue_case(n)[1]
        thr = float(se.norm3(ov.QUEUE_Q)) * ss.ROUGH
        in_band = np.abs(se.norm3(ents - ov.QUEUE_Q) / thr - 1.0) < ov.band_rel(ov.QUEUE_Q, ss.ROUGH) / 4
        # every entry lies deep inside the f32 pre-test's band, on either side of the threshold: all are queued but the
        # one of the frame the query carries (a frame holds one of them), which does not count
        assert in_band.all() and len(ents) - (1 if held else 0) == cap + 1 and ov.queue_overflow(cap + 1, cap)
        assert 0 < a[0]["M"] - se.BOOST * n < n
        assert (frames[0] != se.QUERY_FRAME) == held


def test_room_set_outgrows_its_first_slabs(oracle):
    wl, ans, _ = ss.expected(oracle, "main")
    k = wl.tags["gate"][0]
    # lists of a thousand records against a first room of at most rate / 256 of the visit list + 256
    assert ans[k]["M"] > 512 * ans[k]["D"]
    _, held, frames = ss.expected(oracle, "main", held=True)
    assert frames[k] == ans[k]["cand_frame"][0] and held[k]["M"] < ans[k]["M"]
