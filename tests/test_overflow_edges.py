"""The workloads of tests/_overflow_edges.py reach the edges of the work buffers, shown with the oracle alone (no GPU): the
caps tests/test_gpu_overflow_edges.py sets lie on both sides of what each batch needs and above the hooks' floors, and
the hooks and capacity comparisons the helper restates are the engine's."""
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


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from sgtd_amd import synth
    oracle.build_library()
    return oracle, synth


def test_hooks_and_guards_are_the_engines():
    """every hook's floor and every capacity comparison the helper states is one line of the engine's sources"""
    lines = ov.source_lines(ROOT)
    assert set(lines) == set(ov.HOOKS) | set(ov.GUARDS)
    assert {k: v[0] for k, v in ov.HOOKS.items()} == {"SGTD_REC_CAP": 1024, "SGTD_POOL_UNITS": 64, "SGTD_GROUP_CAP": 1,
                                                      "SGTD_PAIR_CAP": 64, "SGTD_AMB_MIN": 1}
    with open(os.path.join(ROOT, "sgtd_amd", "csrc", "sgtd_accel.hip")) as fh:
        src = fh.read()
    assert "size_t amb_min = %d;" % ov.AMB_MIN_DEFAULT in src
    # the comparisons at their edge: a need of exactly the capacity fits, one more does not
    for f in (ov.pairs_overflow, ov.groups_overflow, ov.queue_overflow):
        assert not f(66, 66) and f(66, 65) and not f(0, 0)
    assert ov.records_must_overflow(2049, 2048) and not ov.records_must_overflow(2048, 2048)
    assert ov.queue_entries(1024, 1) == 16 and ov.queue_entries(1024) == ov.AMB_MIN_DEFAULT == ov.queue_entries(1 << 22)
    assert ov.queue_entries(1 << 23) == 1 << 17


def test_pair_totals_leave_room_above_the_floor(mods):
    """T - 1 is still above SGTD_PAIR_CAP's floor of 64: for the one-query cases (homes, stale's first query) and the batch"""
    oracle, synth = mods
    floor = ov.HOOKS["SGTD_PAIR_CAP"][0]
    wl, ex = ov.sel_expected(oracle)
    homes = ex[wl.tags["homes"][0]]
    assert homes["T"] >= floor + 2 and homes["T"] == int(np.diff(homes["cand_off"]).sum())
    c, sx = ov.stale_expected(oracle)
    assert sx[0]["T"] >= floor + 2 and sx[1]["T"] == 0 and sx[2]["T"] > 0
    fe = ov.frame_expected(oracle, synth)
    T = sum(a["T"] for a in fe["answers"])
    assert T >= floor + 2 and all(a["T"] > 0 for a in fe["answers"])
    # the deferred form (stale_long): the kept lists' totals differ between the masks, and every non-empty one is above the floor
    _, _, lx = ov.stale_long_expected(oracle)
    nc = len(lx[0]["cand_frame"])
    assert nc == 40
    totals = {name: rec.masked(lx[0], mask)["cand_off"][-1] for name, mask in rec.keep_masks(nc).items()}
    assert totals["none"] == 0 and totals["all"] == lx[0]["T"] and len(set(totals.values())) == 5
    assert all(totals[k] >= floor + 2 for k in ("all", "bit0", "highest", "alternating"))
    assert rec.keep_masks(nc)["highest"] == 1 << (nc - 1) and totals["highest"] == int(np.diff(lx[0]["cand_off"])[-1])


def test_rough_matches_exceed_the_record_ladder(mods):
    """M > 2048: caps of 1024 and M / 2 lie under it (the frame batch and stale's first query)"""
    oracle, synth = mods
    fe = ov.frame_expected(oracle, synth)
    M = sum(a["M"] for a in fe["answers"])
    assert M > 2048 and M // 2 > ov.HOOKS["SGTD_REC_CAP"][0]
    c, sx = ov.stale_expected(oracle)
    assert sx[0]["M"] > 2048
    assert all(len(a["rough"]["q_idx"]) == a["M"] for a in sx)


def test_homes_has_the_home_cells_of_its_construction(mods):
    oracle, _ = mods
    wl, ex = ov.sel_expected(oracle)
    assert len(wl.tags["homes"]) == 1
    side, label, _ = wl.sets[wl.tags["homes"][0]]
    assert len(side) == sum(range(1, 10)) + 1
    assert ov.home_groups(side, label) == ov.HOMES_G == 10
    assert ov.HOMES_G - 1 > ov.HOOKS["SGTD_GROUP_CAP"][0]
    # the restatement's own edges: the marker and cell 0
    assert ov.home_groups([[63.2, 1.5, 1.5], [63.7, 1.5, 1.5]], [(1, 1, 1)] * 2) == 2       # at the marker: alone
    assert ov.home_groups([[62.2, 1.5, 1.5], [62.7, 1.5, 1.5]], [(1, 1, 1)] * 2) == 1
    assert ov.home_groups([[0.2, 1.5, 1.5], [0.7, 1.5, 1.5]], [(1, 1, 1)] * 2) == 1
    assert ov.home_groups([[0.0, 1.5, 1.5], [0.7, 1.5, 1.5]], [(1, 1, 1)] * 2) == 2         # probes cell -1: alone
    assert ov.home_groups([[5.2, 1.5, 1.5], [5.7, 1.5, 1.5]], [(1, 1, 1), (1, 1, 2)]) == 2


def test_filter_and_prior_drop_and_keep_candidates(mods):
    oracle, synth = mods
    fe = ov.frame_expected(oracle, synth)
    full = set(fe["answers"][0]["cand_frame"].tolist())
    allowed, f_ans, f_map = fe["filtered"]
    kept = set(f_ans[0]["cand_frame"].tolist())
    first, last = int(fe["answers"][0]["cand_frame"][0]), int(fe["answers"][0]["cand_frame"][-1])
    assert first != last and not {first, last} & kept and kept & full and len(allowed) == ov.FRAME_MAP["n_frames"] - 2
    assert int((f_map < 0).sum()) == fe["descs"][first].n + fe["descs"][last].n
    center, radius, near, p_ans, p_map = fe["prior"]
    assert 0 < len(near) < ov.FRAME_MAP["n_frames"]
    got = set(p_ans[0]["cand_frame"].tolist())
    assert got and got <= set(near.tolist()) and full - set(near.tolist())
    assert np.allclose(ov.pose12(fe["map"].pose)[:, [3, 7]], fe["map"].pose[:, :2])


@pytest.mark.parametrize("skip", [0, 2])
def test_loop_session_finds_session_frames(mods, skip):
    oracle, synth = mods
    m, ses, sels = ov.loop_expected(oracle, synth, skip)
    n_map = m.xyz.shape[0]
    assert len(sels) == ov.LOOP_SESSION and n_map == ov.LOOP_MAP["n_frames"]
    among = [int((s["cand_frame"] >= n_map).sum()) for s in sels]
    assert sum(a > 0 for a in among) >= 1 and all(a == 0 for a in among[:skip + 1])
    assert all((s["cand_frame"] < n_map + max(i - skip, 0)).all() for i, s in enumerate(sels))
    assert sum(s["T"] for s in sels) >= ov.HOOKS["SGTD_PAIR_CAP"][0] + 2 and sum(s["M"] for s in sels) > 2048


def test_multi_shards_pair_totals_differ(mods):
    """the gate set: shard 0's pair total is above MULTI_PAIR_CAP, the others' are below: only some shards rewrite"""
    oracle, _ = mods
    wl, ex = ov.sel_expected(oracle)
    k = wl.tags["gate"][0]
    totals = [s[k]["T"] for s in ov.shard_expected(oracle)]
    assert len(set(totals)) == len(totals) == 3
    assert sum(ov.pairs_overflow(t, ov.MULTI_PAIR_CAP) for t in totals) == 1
    assert min(totals) < ov.MULTI_PAIR_CAP < max(totals) and ov.MULTI_PAIR_CAP >= ov.HOOKS["SGTD_PAIR_CAP"][0]
    frames = np.concatenate([a[2][:1] for a in wl.adds])
    assert set(ov.shards_of_frames(frames, 3).tolist()) == {0, 1, 2} and np.array_equal(frames, np.arange(len(frames)))


def test_shell_queues_more_than_a_64th_of_its_records(mods):
    """at least 17 of the oracle's rough matches lie within 1e-6 relative of the threshold: they are queued for the exact
    test (the band of f32_bounds, restated in the helper), and a queue of rec_cap / 64 entries cannot hold them — at
    SGTD_REC_CAP 1024 (16 entries) and at AMB_REC_CAP, eight times the set's records or more.  The gate and runs
    families sit at the gate's and the run rule's edges, not at the threshold: none of their matches is that near"""
    oracle, _ = mods
    wl, ex = ov.sel_expected(oracle)
    for k in ov.AMB_SETS:
        assert wl.sets[k][2] == "shell"
        near = int(ov.near_threshold(ex[k]["rough"], wl.sets[k][0], ov.ROUGH).sum())
        assert near >= 17 and ov.queue_overflow(near, ov.queue_entries(1024, 1))
        cap = ov.AMB_REC_CAP[k]
        assert ov.queue_overflow(near, ov.queue_entries(cap, 1)) and cap >= 8 * ex[k]["M"]
        assert not ov.queue_overflow(ex[k]["M"], ov.queue_entries(cap))       # the default floor holds them all
    for fam in ("gate", "runs"):
        for k in wl.tags[fam]:
            assert int(ov.near_threshold(ex[k]["rough"], wl.sets[k][0], ov.ROUGH).sum()) == 0


def test_queue_case_queues_exactly_its_band_entries(mods):
    """n entries at the threshold to within 1e-9 relative, four orders of magnitude inside the f32 pre-test's band (the f32
    rounding of the sides costs 1e-6 of the threshold at most): every one is queued, nothing else is — 128 fit the queue of
    QUEUE_REC_CAP / 64 entries, 129 do not; matches and misses are both among them, and the records fit the buffer many times"""
    oracle, _ = mods
    cap = ov.queue_entries(ov.QUEUE_REC_CAP, 1)
    assert cap == 128
    thr = float(ov.se.norm3(ov.QUEUE_Q)) * ov.ROUGH
    band = ov.band_rel(ov.QUEUE_Q, ov.ROUGH)
    f32_rel = 2.0 * 2.0 ** -24 * float(np.abs(ov.QUEUE_Q).max() + 1.0) * np.sqrt(3.0) / thr
    assert band > 1e-5 and ov.QUEUE_REL + f32_rel < band / 4
    for n in (cap, cap + 1):
        wl, ents, exp = ov.queue_expected(oracle, n)
        dis = ov.se.norm3(ents - ov.QUEUE_Q)
        assert len(ents) == n and np.all(np.abs(dis / thr - 1.0) <= 2 * ov.QUEUE_REL)
        assert np.all((ents + 0.5).astype(np.int64) == (ov.QUEUE_Q + 0.5).astype(np.int64))      # one bucket, probed once
        r = exp["rough"]
        own = r["q_idx"] == 0
        assert 0 < int(own.sum()) < n                                   # matches and misses among the queued
        assert np.all(r["dis"][~own] == 0.0) and int((~own).sum()) == n * ov.se.BOOST
        assert ov.queue_overflow(n, cap) == (n > cap) and exp["M"] * 8 <= ov.QUEUE_REC_CAP
        assert len(exp["cand_frame"]) > 0
