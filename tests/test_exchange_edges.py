"""The edge cases of tests/_exchange_edges.py judged on the CPU: merge_ref (the reference's loop, STDesc.cpp:423-433,
written literally) equals dist.merge_candidates (a sort of 64-bit keys in torch) on every case, every mutant of the rule
changes the expected result on the cases named for it, every case's precondition holds, gather_ref equals
dist.merge_verified, and dist.search_loop_choice equals the loop of STDesc.cpp:105-146 on hand-made score rows.  No device."""
import numpy as np
import pytest

import _exchange_edges as xe

CASES = sorted(xe.cases())
ANY_TABLE = ("query_counts", "flags")       # cases whose tables each show ONE thing: a mutant must show on some, not on all


def _torch_tables(t):
    import torch
    return torch.from_numpy(t["frames"].copy()), torch.from_numpy(t["votes"].copy())


# ---- the restatement ----
@pytest.mark.parametrize("name", [n for n in CASES if n != "equal_keys"])
def test_merge_ref_is_dist_merge_candidates(name):
    from sgtd_amd.dist import merge_candidates
    for t in xe.cases()[name]:
        want = xe.expected(t, -1)
        f, v, n = merge_candidates(*_torch_tables(t), t["cn"])
        assert f.numpy().shape == want["frame"].shape, (name, t["note"])
        assert np.array_equal(f.numpy(), want["frame"]) and np.array_equal(v.numpy(), want["votes"]), (name, t["note"])
        assert np.array_equal(n.numpy(), want["n_cand"]), (name, t["note"])


def test_equal_keys_is_where_the_two_part():
    """the sort keeps both copies of an equal key, the reference's vote array holds one count per frame"""
    from sgtd_amd.dist import merge_candidates
    t, = xe.cases()["equal_keys"]
    f, _, n = merge_candidates(*_torch_tables(t), t["cn"])
    want = xe.expected(t, -1)
    assert (f.numpy() == 500).sum(1).tolist() == [2, 2] and (want["frame"] == 500).sum(1).tolist() == [1, 1]
    assert np.array_equal(n.numpy(), want["n_cand"] + 1)


@pytest.mark.parametrize("name", CASES)
def test_preconditions_hold(name):
    tables = xe.cases()[name]
    assert tables
    for t in tables:
        assert bool(t["pre"](t)), (name, t["note"])
        n_tables, nq, cn = t["frames"].shape
        assert xe.per_of(n_tables * cn) is not None and cn <= 64 and n_tables <= 1024
        # src and keep say the same thing, and keep follows my_table
        for my in xe.my_tables(n_tables):
            e = xe.expected(t, my)
            for q in range(nq):
                word = 0
                for s in e["src"][q, :e["n_cand"][q]]:
                    if int(s) >> 8 == my:
                        word |= 1 << (int(s) & 255)
                assert int(e["keep"][q]) == word
                assert (e["src"][q, e["n_cand"][q]:] == -1).all() and (e["frame"][q, e["n_cand"][q]:] == -1).all()


def test_case_list_is_the_issues():
    shapes = {name: sorted(t["frames"].shape[::2] for t in ts) for name, ts in xe.cases().items()}
    for name, want in xe.PER_SHAPES.items():
        assert shapes[name] == sorted(want)
    assert [xe.per_of(n) for n in (64, 65, 256, 257, 512, 513, 1024, 1025)] == [1, 4, 4, 8, 8, 16, 16, None]
    assert shapes["same_lane"] == [(4, 64), (16, 64)] and shapes["keep_bits"] == [(3, 64)]
    assert [t["frames"].shape[1] for t in xe.cases()["query_counts"]] == list(xe.QUERY_COUNTS)
    assert sorted(xe.expected(t, -1)["flags"] for t in xe.cases()["flags"]) == [0, 1, 1, 1, 2, 2, 3, 3]
    assert xe.specials_of(1024) == [0, 15, 16, 31, 32, 47, 48, 63, 64, 1023] and xe.specials_of(64) == [0, 15, 16, 31, 32, 47, 48, 63]


def test_packed_round_trip():
    t, = xe.cases()["ties"]
    for pad in (0, 3):
        a = xe.packed(t["frames"], t["votes"], flag_table=(0, 2), nq={1: 9}, cn=6, serial=11, stride_pad=pad)
        assert a.dtype == np.int32 and a.size == 3 * (2 * 4 * 5 + 4 + pad)
        f, v, words = xe.unpacked(a, 3, 4, 5, pad)
        assert np.array_equal(f, t["frames"]) and np.array_equal(v, t["votes"])
        assert words.tolist() == [[1, 4, 6, 11], [0, 9, 6, 11], [1, 4, 6, 11]]
        assert xe.flags_ref(a, 3, 4, 5, pad) == 3
    assert xe.flags_ref(xe.packed(t["frames"], t["votes"]), 3, 4, 5) == 0


# ---- every mutant shows ----
@pytest.mark.parametrize("mutant", xe.MUTANTS)
def test_mutant_changes_its_cases(mutant):
    names = xe.MUTANT_CASES[mutant]
    assert names and set(names) <= set(CASES)
    for name in names:
        shown = [bool(xe.differs(t, mutant)) for t in xe.cases()[name]]
        assert any(shown) if name in ANY_TABLE else all(shown), (mutant, name, shown)


def test_mutants_show_where_they_should():
    """what a mutant changes is what it is about"""
    c = xe.cases()
    assert {k for _, k in xe.differs(c["keep_bits"][0], "keep_table0")} == {"keep"}
    assert {k for _, k in xe.differs(c["same_lane"][0], "src_merged_pos")} == {"src"}
    assert {k for t in c["flags"] for _, k in xe.differs(t, "flags_table0") + xe.differs(t, "flags_nq_only")} == {"flags"}
    keys, = c["equal_keys"]
    assert xe.differs(keys, "tie_high") == []          # (nothing ties there but the equal keys themselves)
    # lane_gives_up loses exactly the keys behind the first of a lane: query 0 of same_lane holds two of lane 0
    t = c["same_lane"][0]
    a, b = xe.expected(t, -1), xe.expected(t, -1, "lane_gives_up")
    assert a["frame"][0, 0] == b["frame"][0, 0] and a["frame"][0, 1] != b["frame"][0, 1]


# ---- the verification results of the merged candidates ----
@pytest.mark.parametrize("name", ["ties", "full_and_empty", "per_65", "keep_bits", "query_counts"])
def test_gather_ref_is_dist_merge_verified(name):
    """finite values, distinct frames: the gather by src equals the search for the frame id in the shards' tables"""
    import torch
    from sgtd_amd.dist import merge_verified
    rng = np.random.default_rng(3)
    for t in xe.cases()[name]:
        n_tables, nq, cn = t["frames"].shape
        e = xe.expected(t, -1)
        score = rng.normal(size=(n_tables, nq, cn))
        pose = rng.normal(size=(n_tables, nq, cn, 12))
        gathered = np.concatenate([score.reshape(n_tables, -1), pose.reshape(n_tables, -1)], axis=1)
        got_s, got_p = xe.gather_ref(xe.bits(gathered), e["src"], nq, cn)
        # (slots whose frame did not qualify may repeat a frame id of another query's; inside one query they are distinct)
        live = t["frames"] >= 0
        for q in range(nq):
            ids = t["frames"][:, q][live[:, q]]
            assert len(set(ids.tolist())) == ids.size
        want_s, want_p = merge_verified(torch.from_numpy(e["frame"]), torch.from_numpy(t["frames"].copy()), torch.from_numpy(score), torch.from_numpy(pose))
        assert np.array_equal(got_s.view(np.float64), want_s.numpy()), (name, t["note"])
        assert np.array_equal(got_p.view(np.float64), want_p.numpy()), (name, t["note"])
        unused = e["frame"] < 0
        assert (got_s[unused] == xe.MINUS_ONE).all() and (got_p[unused] == 0).all()


def test_gather_cases_reach_their_edges():
    g = xe.gather_cases()
    assert sorted(c["nq"] * c["cn"] for c in g.values() if c["nq"] * c["cn"] > 200) == [255, 256, 257]
    assert (g["all_unused"]["src"] == -1).all() and g["nq0"]["src"].size == 0
    for name in ("last_slot", "last_slot_cn64", "n255", "n256", "n257"):
        c = g[name]
        assert c["src"][-1, -1] == (c["n_tables"] - 1) << 8 | (c["cn"] - 1), name
    assert g["table_1023"]["src"][0, 0] >> 8 == 1023
    for name, c in g.items():
        score, pose = xe.gather_ref(c["gathered"], c["src"], c["nq"], c["cn"])
        if name not in ("all_unused", "nq0"):
            seen = set(score.reshape(-1).tolist()) | set(pose.reshape(-1).tolist())
            assert len(seen & set(xe.DOUBLES.tolist())) >= (4 if name != "table_1023" else 1), name
    score, pose = xe.gather_ref(g["last_slot"]["gathered"], g["last_slot"]["src"], 6, 5)
    assert set(xe.DOUBLES.tolist()) <= set(g["last_slot"]["gathered"].reshape(-1).tolist())
    assert score[5, 0] == g["last_slot"]["gathered"][2, 29] and np.array_equal(pose[5, 3], g["last_slot"]["gathered"][2, 30 + 29 * 12:30 + 30 * 12])


# ---- SearchLoop's choice ----
def test_search_loop_choice_is_the_reference_loop():
    import torch
    from sgtd_amd.dist import search_loop_choice
    frames = np.array([[10, 11, 12, 13]] * 8, np.int32)
    rows = [([0.3, 0.7, 0.7, 0.1], 4, 0.4),        # two equal maxima: the first wins
            ([0.2, 0.4, 0.1, 0.0], 4, 0.4),        # the best exactly at icp_threshold: rejected
            ([0.0, -1.0, -0.5, 0.0], 4, -1.0),     # a best that is <= 0 (the threshold below it)
            ([-1.0, -1.0, -1.0, -1.0], 4, 0.4),
            ([0.9, 0.8, 0.7, 0.6], 0, 0.4),        # n_cand = 0
            ([0.5, 0.6, 0.9, 0.95], 2, 0.4),       # a stronger score beyond n_cand: ignored
            ([0.3, 0.2, 0.9, 0.95], 2, 0.4),       # ... and the live ones fall short
            ([0.41, 0.2, 0.1, 0.05], 1, 0.4)]
    for thr in sorted({r[2] for r in rows}):
        sel = [k for k, r in enumerate(rows) if r[2] == thr]
        scores = np.array([rows[k][0] for k in sel], np.float64)
        n_cand = np.array([rows[k][1] for k in sel], np.int32)
        want = xe.search_loop_ref(frames[sel], n_cand, scores, thr)
        bc, bf, bs = search_loop_choice(torch.from_numpy(frames[sel]), torch.from_numpy(n_cand), torch.from_numpy(scores), thr)
        got = list(zip(bc.tolist(), bf.tolist(), bs.tolist()))
        assert got == want, (thr, got, want)
    all_want = [xe.search_loop_ref(frames[k:k + 1], [r[1]], [r[0]], r[2])[0] for k, r in enumerate(rows)]
    assert all_want == [(1, 11, 0.7), (-1, -1, 0.0), (-1, -1, 0.0), (-1, -1, 0.0), (-1, -1, 0.0), (1, 11, 0.6), (-1, -1, 0.0), (0, 10, 0.41)]
