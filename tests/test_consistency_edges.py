"""The edge worlds of tests/_consistency_edges.py judged on the CPU: every mutant of the rule changes the expected result
on the world named for it (and the mutants of the paths past 4096 edges change no smaller world: the big sizes are
needed), the fast reference helpers equal the plain restatement, and every world's precondition holds.  No device."""
import numpy as np
import pytest

import _consistency_edges as ce
import _consistency_ref as cr

N_BIG = ce.n_big()
N_WAVES = ce.n_waves(N_BIG)


def _ref(w, max_trans, max_rot, shortcut=False):
    tt, min_trace = cr.thresholds(max_trans, max_rot)
    return cr.consistent(w["ids"], w["poses"], w["frame_a"], w["frame_b"], w["rel_pose"], tt, min_trace, shortcut=shortcut)


_small = {}


def small_ref(k):
    if k not in _small:
        name, w, mt, mr = ce.small_worlds()[k]
        _small[k] = (name, _ref(w, mt, mr))
    return _small[k]


def _rounds_direct(adj, valid):
    """the rounds of the choice under the shortcut rule, counted the plain way"""
    P = valid.copy()
    rounds = 0
    while P.any():
        idx = np.flatnonzero(P)
        d = adj[np.ix_(idx, idx)].sum(1)
        rounds += 1
        if (d == idx.size - 1).all():
            break
        P &= adj[idx[int(np.argmax(d))]]
    return rounds


def _same_choice(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


def test_sizes():
    assert N_BIG == 4161 and N_WAVES == 4096 and (N_BIG + 63) // 64 == 66 and N_BIG % 64 == 1
    assert N_BIG > N_WAVES and (N_BIG + 63) // 64 > 64
    for n_cus in (32, 64, 256, 304):
        n = ce.n_big(n_cus)
        assert n > ce.n_waves(n, n_cus) and (n + 63) // 64 > 64 and n - 65 >= cr.WAVE_BITS


# ---- the fast helpers ----
def test_adjacency_rows_equals_adjacency():
    w = ce.parity_recipe(300)
    fb = w["frame_b"].copy()
    fb[[7, 200]] = 4_000_000_000                    # two invalid edges
    P, A, valid = cr.edges(w["ids"], w["poses"], w["frame_a"], fb, w["rel_pose"])
    tt, min_trace = cr.thresholds(1.0, np.deg2rad(5.0))
    adj, g2, gt = cr.adjacency(P, A, valid, tt, min_trace)
    rows = ce.sample_rows(300, 256)
    assert {0, 7, 63, 64, 127, 128, 200, 255, 256, 298, 299} <= set(rows.tolist()) | {7, 200}
    rows = np.unique(np.concatenate([rows, [7, 200]]))
    a, r2, rt = cr.adjacency_rows(P, A, valid, tt, min_trace, rows)
    assert np.array_equal(a, adj[rows]) and adj[rows].any()
    assert np.array_equal(r2, np.minimum(g2, g2.T)[rows]) and np.array_equal(rt, np.minimum(gt, gt.T)[rows])
    assert not a[rows == 7].any() and not a[:, 200].any()


def test_greedy_fast_equals_greedy_on_small_worlds():
    for k in range(len(ce.small_worlds())):
        name, ref = small_ref(k)
        for shortcut in (False, True):
            slow = cr.greedy(ref["adj"], ref["valid"], shortcut)
            fast = cr.greedy_fast(ref["adj"], ref["valid"], shortcut)
            assert _same_choice(fast, slow), (name, shortcut)
            assert _same_choice(fast, (ref["in_set"], ref["degree"], ref["pick"], ref["n_set"])), name
        assert cr.greedy_fast(ref["adj"], ref["valid"], True)[4] == _rounds_direct(ref["adj"], ref["valid"]), name
        assert cr.greedy_fast(ref["adj"], ref["valid"], False)[4] == ref["n_set"], name


def test_greedy_fast_equals_greedy_on_random_graphs():
    rng = np.random.default_rng(11)
    many_rounds = 0
    for case in range(50):
        n = int(rng.integers(1, 301))
        adj = np.triu(rng.random((n, n)) < rng.choice([0.05, 0.3, 0.7, 0.95, 1.0]), 1)
        valid = rng.random(n) < 0.9
        adj &= valid[:, None] & valid[None, :]
        adj |= adj.T
        for shortcut in (False, True):
            assert _same_choice(cr.greedy_fast(adj, valid, shortcut), cr.greedy(adj, valid, shortcut)), (case, shortcut)
        rounds = cr.greedy_fast(adj, valid, True)[4]
        assert rounds == _rounds_direct(adj, valid), case
        many_rounds += rounds > 3
    assert many_rounds > 20
    none = np.zeros(5, bool)
    assert cr.greedy_fast(np.zeros((5, 5), bool), none, True)[3:] == (0, 0)
    assert np.array_equal(cr.unpack_rows(cr.pack_rows(adj), n), adj)


# ---- chains ----
@pytest.mark.parametrize("low", [False, True])
def test_chains_take_the_rounds_claimed(low):
    for n in ce.SMALL_CHAINS + (N_BIG,):
        w = ce.chain(n, low)
        adj = ce.shift_adjacency(w)
        want = ce.chain_expect(n, low)
        got = cr.greedy_fast(adj, np.ones(n, bool), True)
        assert _same_choice(got, want) and got[4] == want[4] == n - 1, (n, low)
        if n < 200:
            ref = _ref(w, w["max_trans"], w["max_rot"])
            assert np.array_equal(ref["adj"], adj) and ref["valid"].all(), n
    assert [n - 1 for n in ce.SMALL_CHAINS] == [16, 17, 48, 49, 112, 113]     # on and one past 16, 16 + 32, 16 + 32 + 64 rounds sent


# ---- knife pairs ----
def test_knife_pairs_discriminate():
    pairs = ce.knife_pairs()
    assert len(pairs) >= 8
    for m in ce.PAIR_MUTANTS:
        assert sum(m in p["flips"] for p in pairs) >= 3, m
    w = ce.knife_world()
    min_trace = cr.thresholds(1.0, ce.KNIFE_ROT)[1]
    for p in pairs:
        assert p["max_trans"] * p["max_trans"] == p["d2"] and 0.01 < p["d2"] < 4.0
        d2, tr = ce.pair_values(w, [p["lo"]], [p["hi"]])
        assert d2[0] == p["d2"] and tr[0] > min_trace
        for m in ce.PAIR_MUTANTS:
            md2, mtr = ce.pair_mutant_values(w, [p["lo"]], [p["hi"]], m)
            assert (m in p["flips"]) == (not (md2[0] <= p["d2"] and mtr[0] >= min_trace)), (p, m)
            if m in p["flips"]:
                assert md2[0] > p["d2"]


def test_contracted_dot_is_a_fused_multiply_add():
    # 1 + 2^-30 squared is 1 + 2^-29 + 2^-60: the product rounds the last term away, a fused add of -1 keeps it
    x = np.array([1.0 + 2.0 ** -30])
    assert (x * x - 1.0)[0] == 2.0 ** -29 and ce.fma(x, x, -1.0)[0] == 2.0 ** -29 + 2.0 ** -60
    a = np.random.default_rng(2).normal(size=(6, 50))
    assert np.array_equal(ce.dot3_contracted(a[0], a[1], a[2], np.zeros(50), a[4], np.zeros(50)), a[0] * a[1])
    assert (ce.dot3_contracted(*a) != ce.dot3_plain(*a)).any() and (ce.dot3_sum_right(*a) != ce.dot3_plain(*a)).any()
    assert np.allclose(ce.dot3_contracted(*a), ce.dot3_plain(*a), rtol=0, atol=1e-14)


def test_every_knife_run_sits_on_the_bound_alone():
    runs = ce.knife_runs()
    assert len(runs) == len(ce.knife_pairs()) * len(ce.PLACEMENTS)
    for name, w, p, (i, j) in runs:
        tt, min_trace = cr.thresholds(p["max_trans"], ce.KNIFE_ROT)
        assert tt == p["d2"], name
        ref = _ref(w, p["max_trans"], ce.KNIFE_ROT)
        assert ref["valid"].all() and ref["gap_d2"][i, j] == 0.0 and ref["adj"][i, j] and ref["adj"][j, i], name
        assert np.count_nonzero(ref["gap_d2"] <= 1e-9 * max(1.0, tt)) == 1, name
        assert ref["min_gap_tr"] > 1e-9 * max(1.0, abs(min_trace)), name
        assert 3 < ref["n_set"] < 140, name
    # the placements: the diagonal's word, two words of one 128-column tile, two tiles, rows of different 64-row blocks
    assert [(i >> 6 == j >> 6, i >> 7 == j >> 7) for i, j in ce.PLACEMENTS] == [(True, True), (False, True), (False, False), (False, True), (False, False), (False, False)]


# ---- the mutants of the choice ----
_big = {}


def big_adj(name):
    if name not in _big:
        w = ce.BIG_ANALYTIC[name]()
        _big[name] = (w, ce.shift_adjacency(w))
    return _big[name]


def _flips(adj, valid, mutant, n_cus=ce.N_CUS_MI355X):
    want = cr.greedy_fast(adj, valid, True)
    got = cr.greedy_fast(adj, valid, True, ce.greedy_parts(mutant, valid.size, n_cus))
    return not (_same_choice(got, want) and got[4] == want[4])


@pytest.mark.parametrize("mutant,world", [(m, w) for m, ws in ce.MUTANT_WORLDS.items() if m not in ce.PAIR_MUTANTS for w in ws if w != "noisy_big"])
def test_mutant_flips_its_world(mutant, world):
    if world == "remaining_degree":
        w = ce.remaining_degree()
        adj = ce.shift_adjacency(w)
    elif world == "chain_big":
        for name in ("chain_big_high", "chain_big_low"):
            assert _flips(big_adj(name)[1], np.ones(N_BIG, bool), mutant), name
        return
    else:
        w, adj = big_adj(world)
    assert _flips(adj, np.ones(adj.shape[0], bool), mutant)


def test_big_only_mutants_leave_every_small_world():
    """below 4096 edges the count pass has a wave per row and one step over the words, and the select pass's scan stays in
    wave 0: nothing there can show these four"""
    for k in range(len(ce.small_worlds())):
        name, ref = small_ref(k)
        for mutant in ce.BIG_ONLY_MUTANTS:
            assert not _flips(ref["adj"], ref["valid"], mutant), (name, mutant)
    rng = np.random.default_rng(5)
    n = 4096
    adj = np.triu(rng.random((n, n)) < 0.5, 1)
    adj |= adj.T
    for mutant in ce.BIG_ONLY_MUTANTS:
        assert not _flips(adj, np.ones(n, bool), mutant), mutant


def test_small_worlds_catch_the_small_mutants():
    w = ce.remaining_degree()
    ref = _ref(w, 5.0, 0.1)
    assert np.array_equal(ref["adj"], ce.shift_adjacency(w))
    assert ref["degree"].tolist() == [16, 15] + [12] * 6 + [8] * 8 + [11] * 5 + [1] * 4
    assert np.flatnonzero(ref["in_set"]).tolist() == [0] + list(range(2, 8)) + list(range(16, 21)) and ref["pick"][2] == 1
    inside = (ref["adj"][1] & ref["adj"][0]).sum(), (ref["adj"][2] & ref["adj"][0]).sum()
    assert inside == (6, 11)                        # x has the larger degree, G1 the larger degree inside P
    wrong = cr.greedy_fast(ref["adj"], ref["valid"], True, ce.greedy_parts("total_degree", 25))
    assert np.flatnonzero(wrong[0]).tolist() == list(range(0, 8))


# ---- the big worlds' preconditions ----
def test_groups_big():
    w, adj = big_adj("groups_big")
    in_set, degree, pick, n_set, rounds = cr.greedy_fast(adj, np.ones(N_BIG, bool), True)
    assert n_set == N_BIG // 3 and rounds == 2 and (degree == N_BIG // 3 - 1).all()
    members = np.flatnonzero(w["group"] == 0)
    assert members[0] == 0 and members[-1] == N_BIG - 1 and np.bincount(w["group"]).tolist() == [N_BIG // 3] * 3
    assert np.array_equal(np.flatnonzero(in_set), members) and np.array_equal(pick[members], np.arange(members.size))
    assert np.unique(members >> 6).size == 66          # the shortcut's members lie in every row word


def test_hub_then_clique_big():
    w, adj = big_adj("hub_then_clique_big")
    in_set, degree, pick, n_set, rounds = cr.greedy_fast(adj, np.ones(N_BIG, bool), True)
    K = np.arange(N_BIG - 65, N_BIG)
    assert rounds == 3 and n_set == 66 and degree[0] == 95 and (degree[1:31] == 30).all() and (degree[K] == 65).all()
    assert pick[0] == 0 and np.array_equal(pick[K], 1 + np.arange(65)) and in_set.sum() == 66
    assert (K[1:] >> 6).min() >= 64                     # what the shortcut takes lies in the second wave's words alone


@pytest.mark.parametrize("name", ["tie_far", "tie_split"])
def test_tie_worlds(name):
    w, adj = big_adj(name)
    u1, u2 = w["tie"]
    deg = adj.sum(1)
    assert u1 < u2 and deg[u1] == deg[u2] == deg.max() == 40 and np.count_nonzero(deg == deg.max()) == 2
    assert (u1 >= N_WAVES) == (name == "tie_far") and u2 >= N_WAVES and u1 % N_WAVES != u2 % N_WAVES
    in_set, degree, pick, n_set, rounds = cr.greedy_fast(adj, np.ones(N_BIG, bool), True)
    assert pick[u1] == 0 and not in_set[u2] and n_set == 21 and rounds == 3


def test_noisy_big():
    w = ce.noisy_big()
    n = N_BIG
    P, A, valid = cr.edges(w["ids"], w["poses"], w["frame_a"], w["frame_b"], w["rel_pose"])
    bad = np.array(sorted(w["invalid"]))
    assert np.array_equal(np.flatnonzero(~valid), bad) and 35 <= bad.size <= 50
    assert np.count_nonzero(bad >= cr.WAVE_BITS) >= 3 and bad[-1] == n - 1 and set(w["invalid"].values()) == {"no_pose", "beyond_store", "beyond_u32", "nan_rel", "inf_pose", "nan_rot"}
    Pa, Aa, valid_a = cr.edges(w["ids"], w["poses"], None, w["frame_b"], w["rel_pose"], pose_a=w["poses"][w["frame_a"]])
    assert np.array_equal(valid_a, valid)           # the pose_a form sees the same invalid edges
    tt, min_trace = cr.thresholds(w["max_trans"], w["max_rot"])
    rows = ce.sample_rows(n, N_WAVES)
    assert rows.size >= 66 and np.unique(rows >> 6).size == 66 and np.unique(rows[:60] % 4).size == 4
    adj, g2, gt = cr.adjacency_rows(P, A, valid, tt, min_trace, rows)
    assert g2.min() > 1e-9 * max(1.0, tt) and gt.min() > 1e-9 * max(1.0, abs(min_trace))
    assert not adj[:, bad].any() and not adj[np.isin(rows, bad)].any()
    # words_64 shows: a row with neighbours past the first 64 words has another degree under it
    assert (adj[:, cr.WAVE_BITS:].sum(1) > 0).sum() > 10
    deg = adj.sum(1)[valid[rows]]
    assert 0.02 * n < np.median(deg) < 0.9 * n        # no clique, not empty: the choice takes many rounds


def test_max_edges_expectation_on_a_small_copy():
    group = ce.max_edges()["group"]
    assert group.size == ce.MAX_EDGES and np.bincount(group).tolist() == [16384, 8192, 4096, 4096] and group[0] == 1
    assert ce.max_edges()["ids"].size == 8192
    g = group[:1000]
    s = np.zeros((1000, 3))
    s[:, 0] = 100 * g
    w = ce.shift_world(s, n_frames=96, max_trans=1.0)
    ref = _ref(w, 1.0, 0.1, shortcut=True)
    assert np.array_equal(ref["adj"], ce.shift_adjacency(w)) and np.array_equal(ce.group_rows(g), ref["rows"])
    want = ce.group_greedy(g)
    assert _same_choice(want, (ref["in_set"], ref["degree"], ref["pick"], ref["n_set"]))
    assert want[4] == cr.greedy_fast(ref["adj"], ref["valid"], True)[4] == 2 and want[2][1] == 0


def test_store_steps():
    w = ce.store_world()
    tt, min_trace = cr.thresholds(w["max_trans"], w["max_rot"])
    seen = []
    for k in range(4):
        ids, poses = ce.store_after(k)
        ref = cr.consistent(ids, poses, w["frame_a"], w["frame_b"], w["rel_pose"], tt, min_trace)
        assert cr.clear_of_thresholds(ref, tt, min_trace), k
        seen.append(ref)
    assert not seen[0]["valid"][20] and seen[0]["valid"].sum() == 149
    assert not np.array_equal(seen[1]["rows"], seen[0]["rows"]) and seen[1]["valid"].sum() == 149     # the moved pose changes decisions
    assert seen[2]["valid"].sum() < 149 and not seen[2]["valid"][70]
    assert seen[3]["valid"][20] and seen[3]["valid"].sum() == seen[2]["valid"].sum() + 1 and ce.store_after(3)[0].max() == 340
