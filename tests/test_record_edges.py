"""The workloads of tests/test_gpu_record_edges.py, checked without a GPU: a plain restatement of the passes over the match
records (STDesc.cpp:404-453, tests/_record_edges.py) equals the oracle on every query of every case, every family really
reaches the edge it is named for (asserted from the oracle's answer and pq_geometry), the helper's copies of the kernels'
constants equal the headers, and every mutant of the restatement is caught by a named case."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _record_edges as rec  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("cand_frame", "cand_votes", "cand_off", "q_idx", "db_entry")


@pytest.fixture(scope="module")
def world(oracle_mod):
    """name -> (case, reference table, the oracle's answer per query, the restatement's answer per query)"""
    out = {}
    for c in rec.cases():
        o = oracle_mod.OracleManager(**c.config())
        c.load(o, oracle_mod)
        tab = c.ref_table()
        theirs, ours = [], []
        for k in range(len(c.queries)):
            sel = o.select(c.query_descs(oracle_mod, k))
            sel.update(votes=o.votes(), M=o.counters()["M"])
            theirs.append(sel)
            ours.append(c.ref_answer(tab, k))
        out[c.name] = (c, tab, theirs, ours)
    return out


def _same(a, b):
    return a["M"] == b["M"] and np.array_equal(a["votes"], b["votes"]) and all(np.array_equal(a[k], b[k]) for k in KEYS)


def test_restatement_equals_the_oracle(world):
    for name, (c, _, theirs, ours) in world.items():
        for k, (a, b) in enumerate(zip(ours, theirs)):
            np.testing.assert_array_equal(a["votes"], b["votes"], err_msg="%s %d votes" % (name, k))
            assert a["M"] == b["M"], (name, k)
            for key in KEYS:
                np.testing.assert_array_equal(a[key], b[key], err_msg="%s %d %s" % (name, k, key))


def test_header_constants_equal_the_helper_copies():
    src = ""
    for f in ("common.hip.h", "probe_kernels.hip.h", "select_kernels.hip.h", "sgtd_accel.hip"):
        src += open(os.path.join(ROOT, "sgtd_amd", "csrc", f)).read()
    for name in ("SGTD_PQ_THREADS", "SGTD_PQ_WORDS", "SGTD_VT_BINS", "SGTD_TOPK_BINS", "SGTD_TOPK_POOL", "SGTD_CAND_HASH",
                 "SGTD_MAX_CAND"):
        m = re.findall(r"#define\s+%s\s+(\d+)" % name, src)
        assert m and all(int(v) == getattr(rec, name) for v in m), name
    m = re.search(r"tile_span = span <= (\d+) \* (\d+) \? span : (\d+) \* (\d+);", src)
    assert m and int(m.group(1)) * int(m.group(2)) == int(m.group(3)) * int(m.group(4)) == rec.VOTES_TILE_FRAMES
    assert "(f * 0x9E3779B1u) >> 24" in src and rec.hash_slot(1) == 0x9E
    assert "SGTD_PQ_WAVES * SGTD_PQ_WORDS * SGTD_WAVE" in src and rec.PQ_TILE_RECS == 8192


# ---- every family reaches its edge ---------------------------------------------------------------------------------
def test_vote_floor_reaches(world):
    c, _, theirs, _ = world["vote_floor"]
    v = theirs[0]["votes"][:4].tolist()
    assert sorted(v) == [4, 4, 5, 6] and theirs[0]["cand_frame"].tolist() == [2, 1]
    assert len(theirs[1]["cand_frame"]) == 0 and theirs[1]["votes"].max() == 4 and theirs[1]["M"] > 0
    assert theirs[1]["cand_off"].tolist() == [0] and len(theirs[1]["q_idx"]) == 0
    assert theirs[2]["cand_frame"].tolist() == [3] and sorted(theirs[2]["votes"][[1, 3]].tolist()) == [4, 5]


def test_cut_reaches(world):
    for cn in (1, 3, 50, 64):
        c, _, theirs, _ = world["cut/cn%d" % cn]
        for k, n in enumerate((cn - 1, cn, cn + 1)):
            v = theirs[k]["votes"]
            assert int((v >= 5).sum()) == n and int((v == 4).sum()) == 2
            assert len(set(v[v >= 5].tolist())) == n                     # distinct counts
            assert len(theirs[k]["cand_frame"]) == min(n, cn)
            if n > 2:
                assert np.any(np.diff(v[v >= 5]) < 0) and np.any(np.diff(v[v >= 5]) > 0)      # not in frame order
        # ties at the cut: more frames tied at the last candidate's votes than slots left; the lowest ids win
        t = theirs[3]
        v, cf, cv = t["votes"], t["cand_frame"], t["cand_votes"]
        last = cv[-1]
        tied = np.nonzero(v == last)[0]
        took = cf[cv == last]
        assert last == 6 and len(tied) == 5 and 0 < len(took) < len(tied), (cn, last, len(tied), len(took))
        assert took.tolist() == tied[:len(took)].tolist()
        assert not np.all(np.diff(tied) == 1)                              # (other frames between the tied ones)
        t = theirs[4]
        assert int((t["votes"] == 5).sum()) == cn + 2 == int((t["votes"] > 0).sum())
        assert t["cand_frame"].tolist() == np.nonzero(t["votes"] == 5)[0][:cn].tolist()


def test_pool_reaches(world):
    for tie in (5, 7):
        for n in (1023, 1024, 1025):
            c, _, theirs, _ = world["pool/tie%d/n%d" % (tie, n)]
            t = theirs[0]
            v = np.sort(t["votes"])[::-1]
            thr = v[c.cn - 1]                        # the threshold both top-k kernels search: the cn-th largest count
            assert thr == tie and int((t["votes"] >= thr).sum()) == n
            assert t["cand_votes"][:3].tolist() == [tie + 3, tie + 2, tie + 1]
            assert t["cand_frame"][:3].tolist() == [n - 1, 3, n // 2]
            assert t["cand_frame"][3:].tolist() == [f for f in range(60) if f != 3][:c.cn - 3]
            if tie > 5:
                assert int(((t["votes"] >= 5) & (t["votes"] < tie)).sum()) == 4


def test_bins_reaches(world):
    for cn in (50, 3):
        c, _, theirs, _ = world["bins/clip/cn%d" % cn]
        t = theirs[0]
        assert t["votes"][:10].tolist() == [4094, 4095, 4096, 4097, 8190, 8191, 8192, 8193, 8195, 8194]
        want = [8, 9, 7, 6, 5, 4, 3, 2, 1, 0]
        assert t["cand_frame"].tolist() == want[:cn]
        # the cut of cn = 3 falls inside the last bin of both searches: five frames at or beyond 8191, nine at or beyond 4095
        assert int((t["votes"] >= rec.SGTD_TOPK_BINS - 1).sum()) == 5 and int((t["votes"] >= rec.SGTD_VT_BINS - 1).sum()) == 9
    for third in (63, 64, 127, 128):
        t = world["bins/lane%d" % third][2][0]
        assert np.sort(t["votes"])[::-1][:4].tolist() == [200, 150, third, third - 1]
        assert t["cand_votes"].tolist() == [200, 150, third]


def test_span_reaches(world):
    for wide in (False, True):
        for rem in (0, 1, 15):
            c, _, theirs, _ = world["span/%s/rem%d" % ("wide" if wide else "narrow", rem)]
            t = theirs[0]
            lo, n = c.info["lo"], c.info["span"]
            f = np.asarray(c.eframe)
            assert f.min() == lo > 0 and f.max() - lo + 1 == n and n % 16 == rem
            assert lo in t["cand_frame"] and lo + n - 1 in t["cand_frame"]
            assert (n > 120000 and c.max_frame_n == 200000) if wide else n * 4 < 64 * 1024
            if wide:
                a, b = c.info["collide"]
                assert rec.hash_slot(a) == rec.hash_slot(b) and a in t["cand_frame"] and b in t["cand_frame"]
                assert lo + 36863 in t["cand_frame"] and lo + 36864 in t["cand_frame"]
                assert len(t["cand_frame"]) == 8
            else:
                assert len(t["cand_frame"]) == 4


def _geo(world, name):
    c, _, theirs, ours = world[name]
    L = ours[0]["lengths"]
    np.testing.assert_array_equal(L, c.info["lengths"])          # (the oracle-equal restatement's list lengths)
    return L, rec.pq_geometry(L)


def test_lists_reaches(world):
    for nd in (511, 512, 513, 1024, 1025):
        L, g = _geo(world, "lists/nd%d" % nd)
        assert len(L) == nd and len(g) == (nd + 511) // 512
        assert set((L[L > 0] % 4).tolist()) == {0, 1, 2, 3}
        assert L[0] == 0 and L[1] == 0 and L[-1] == 0 and np.any(L[2:-2] == 0) and g[-1]["K"] == int((L[(len(g) - 1) * 512:] > 0).sum())
    assert _geo(world, "lists/nd513")[1][1]["K"] == 0 and _geo(world, "lists/nd1025")[1][2]["RQ"] == 0     # (a last super-block of one empty list)
    L, g = _geo(world, "lists/empty_block")
    assert [x["RQ"] > 0 for x in g] == [True, False, True, False]       # (the fourth: one empty list)
    for rq in (2047, 2048, 2049, 4097):
        L, g = _geo(world, "lists/rq%d" % rq)
        assert len(g) == 1 and g[0]["RQ"] == rq and g[0]["n_tiles"] == (rq + 2047) // 2048
        assert set((L % 4).tolist()) == {0, 1, 2, 3}
    L, g = _geo(world, "lists/long")
    assert L.tolist() == [3, 25001, 6] and L[1] > 3 * rec.PQ_TILE_RECS and g[0]["n_tiles"] == 4
    assert g[0]["starts"][1:3].max() == 0                       # tiles 1 and 2 and all their waves start in mid-list
    L, g = _geo(world, "lists/short")
    assert g[0]["K"] == 512 and g[0]["RQ"] == 512 and g[0]["starts"][0, :2].min() >= 63 and g[0]["starts"][0, :2].max() == 256
    for n in (63, 64, 65):
        L, g = _geo(world, "lists/starts%d" % n)
        s = g[0]["starts"]
        assert s[0, 0, -1] == n and s[0, 0, -1] == s.max()       # wave 0 sees exactly n starts, no wave more
        assert s.shape[0] == 1 and s[0, 1:].max() < 63           # (one tile; the other waves stay on the marks)


def test_mix_reaches(world):
    c, tab, theirs, ours = world["mix"]
    t = theirs[0]
    assert len(t["cand_frame"]) == 64 == c.cn and set(t["cand_frame"].tolist()) == set(c.info["cands"])
    rq, re_ = c.ref_records(tab, 0)
    L = ours[0]["lengths"]
    sb, pre = rec.record_tiles(L)
    first = np.cumsum(L) - L
    tile = (pre[rq] + (np.arange(len(rq)) - first[rq]) // 4) // rec.PQ_TILE_QUADS
    slot_of = np.full(c.max_frame_n, -1)
    slot_of[t["cand_frame"]] = np.arange(64)
    slot = slot_of[tab.arrays()[1][re_]]
    assert int((tile == 0).sum()) == 8192 and np.all(slot[tile == 0] == -1)             # a tile with 0 candidate records
    assert int((tile == 1).sum()) == 8192 and np.all(slot[tile == 1] == 0)              # a tile of one candidate's records
    s2 = slot[tile == 2]
    assert set(s2.tolist()) == set(range(-1, 64)) and int((s2 == -1).sum()) >= 1000      # all 64 slots and others, interleaved
    # equal-slot records of tile 2 from different descriptors and from different waves
    quad = pre[rq] + (np.arange(len(rq)) - first[rq]) // 4
    m = (tile == 2) & (slot == 63)
    assert len(set(rq[m].tolist())) >= 20 and len(set(((quad[m] % rec.PQ_TILE_QUADS) // 256).tolist())) >= 4
    # the records the f64 test kills: entries of candidate frames within 1e-12 (relative) beyond the threshold
    assert len(c.ekey) - t["M"] == c.info["n_dead"] == 56
    side, frame, _ = tab.arrays()
    qs = rec.key_sides_labels(c.queries[0][41:42])[0][0]
    thr = float(rec.se.norm3(qs)) * rec.ROUGH
    d = rec.se.norm3(side - qs)
    dead = (d >= thr) & (d < thr * (1 + 1e-12))
    assert int(dead.sum()) == 56 and np.all(slot_of[frame[dead]] >= 0) and np.all(slot_of[frame[dead]] < 8)
    # a match in a lower cell than the key's own, inserted behind the key's own cell's entry
    m = rq == 41
    assert np.any(np.diff(re_[m][slot[m] == 0]) < 0)


def test_ids_reaches(world):
    c = world["ids/by_frame"][0]
    f = np.asarray(c.eframe)
    assert np.any(np.diff(f) < 0) and f[0] == 5
    c = world["ids/tail"][0]
    assert c.tail_at == 3 and c.stamped and len(c.calls) == 6
    for cn in (50, 64):
        for n, bits in ((1 << 13, 13), ((1 << 13) + 1, 14), (1 << 16, 16), (1 << 17, 17)):
            c, tab, theirs, _ = world["ids/big%d/cn%d" % (n, cn)]
            f = tab.arrays()[1]
            assert np.bincount(f).max() == n == int((f == 2).sum()) and (n - 1).bit_length() == bits
            t = theirs[0]
            k = t["cand_frame"].tolist().index(2)
            e = t["db_entry"][t["cand_off"][k]:t["cand_off"][k + 1]]
            rank = e - int(np.nonzero(f == 2)[0][0])
            assert rank.min() == n - 7 and rank.max() == n - 1           # the ranks use every bit


def test_stale_reaches(world):
    c, _, theirs, _ = world["stale"]
    assert [len(t["cand_frame"]) for t in theirs] == [40, 0, 3]
    assert min(np.diff(theirs[0]["cand_off"])) >= 60 and theirs[1]["M"] > 0
    assert not set(theirs[0]["cand_frame"].tolist()) & set(theirs[2]["cand_frame"].tolist())


def test_tiny_keypoint_frames_reach_the_vote_floor(oracle_mod):
    """rec.tiny: queries whose best frame has 4, 5 and 6 votes, with and without candidates"""
    (mx, ml, moff), (qx, ql, qoff) = rec.tiny()
    o = oracle_mod.OracleManager(**rec.TINY_CONFIG)
    for f in range(len(moff) - 1):
        assert o.build(mx[moff[f]:moff[f + 1]], ml[moff[f]:moff[f + 1]], export=False) >= 1
        o.add_last()
    best, nc = [], []
    for q in range(len(qoff) - 1):
        o.build(qx[qoff[q]:qoff[q + 1]], ql[qoff[q]:qoff[q + 1]], export=False)
        nc.append(len(o.select()["cand_frame"]))
        best.append(int(o.votes().max()))
    assert {4, 5, 6} <= set(best) and min(best) >= 1
    assert all((n > 0) == (b >= 5) for n, b in zip(nc, best)) and nc.count(0) >= 10 and sum(n > 0 for n in nc) >= 2


# ---- mutants of the restatement ------------------------------------------------------------------------------------
CAUGHT_BY = {
    "tie_high": ("cut/cn3", 3), "floor4": ("vote_floor", 0), "floor6": ("vote_floor", 0), "no_zero": ("vote_floor", 0),
    "rounds_plus": ("cut/cn3", 2), "rounds_minus": ("cut/cn3", 1), "clip4095": ("bins/clip/cn50", 0),
    "clip8191": ("bins/clip/cn50", 0), "sort_entry": ("lists/nd513", 0), "sort_desc_entry": ("mix", 0),
    "tile_reversed": ("lists/long", 0), "drop_partial_quad": ("lists/nd513", 0), "dead_kept": ("mix", 0),
    "unmasked_offsets": ("stale", 0),
}


@pytest.mark.parametrize("mutant", rec.MUTANTS)
def test_mutant_is_caught(world, mutant):
    name, k = CAUGHT_BY[mutant]
    c, tab, theirs, ours = world[name]
    if mutant == "unmasked_offsets":
        keep = rec.keep_masks(len(theirs[k]["cand_frame"]))["alternating"]
        want = rec.masked(theirs[k], keep)
        assert _same(c.ref_answer(tab, k, keep=keep), want), "the masked restatement equals the masked oracle on %s" % name
        assert not _same(c.ref_answer(tab, k, mutant, keep=keep), want), "%s is not caught by %s" % (mutant, name)
        return
    assert _same(ours[k], theirs[k])
    assert not _same(c.ref_answer(tab, k, mutant), theirs[k]), "%s is not caught by %s query %d" % (mutant, name, k)
