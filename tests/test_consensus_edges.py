"""The edge cases of tests/_consensus_edges.py judged on the CPU: the restatement with replaceable parts is
_consensus_ref.consensus bit for bit, every mutant of the rule changes the expected result on the cases named for it (and
the arithmetic mutants of the pair rule change no integer case: the knife pairs are needed), and every case's precondition
holds.  No device."""
import functools

import numpy as np
import pytest

import _consensus_edges as ce
import _consensus_ref as ref
import _consistency_ref as cr

CASES = sorted(ce.cases())
INTEGER_CASES = [n for n in CASES if not ce.cases()[n]["noisy"]]
KNIFE_TRACE = cr.thresholds(1.0, ce.KNIFE_ROT)[1]


def _thr(name):
    c = ce.cases()[name]
    return cr.thresholds(c["max_trans"], c["max_rot"])


@functools.lru_cache(None)
def result(name, mutant=None):
    tt, min_trace = _thr(name)
    return ce.consensus_with(ce.cases()[name]["batch"], tt, min_trace, mutant)


@functools.lru_cache(None)
def knife_result(k, mutant=None):
    """the first run of knife pair k (placement 0, the only query of its call)"""
    name, b, p, (i, j), q = ce.knife_runs()[2 * len(ce.PLACEMENTS) * k]
    assert q == 0 and (i, j) == ce.PLACEMENTS[0]
    return ce.consensus_with(b, p["d2"], KNIFE_TRACE, mutant), (i, j)


def _same_as_reference(b, tt, min_trace, where):
    want = ce.reference(b, tt, min_trace)
    got = ce.consensus_with(b, tt, min_trace)
    assert ce.differs(got, want) == [], where
    assert np.array_equal(got["adj"], want["adj"]) and np.array_equal(got["valid"], want["valid"]), where
    assert got["min_gap_d2"] == want["min_gap_d2"] and got["min_gap_tr"] == want["min_gap_tr"], where
    for r in (ce.reference(b, tt, min_trace, shortcut=True), ce.consensus_with(b, tt, min_trace, shortcut=True)):
        assert ce.differs(r, want) == [], (where, "shortcut")


# ---- the restatement ----
@pytest.mark.parametrize("name", CASES)
def test_restatement_is_the_reference(name):
    _same_as_reference(ce.cases()[name]["batch"], *_thr(name), name)


def test_restatement_is_the_reference_on_knife_runs():
    runs = ce.knife_runs()
    assert len(runs) == len(ce.knife_pairs()) * len(ce.PLACEMENTS) * 2
    for name, b, p, _, _ in runs[::7] + runs[-2:]:
        _same_as_reference(b, p["d2"], KNIFE_TRACE, name)


def test_quat_with_is_the_reference_quat():
    import _relax_ref as rr
    rng = np.random.default_rng(3)
    mats = ce.cube_rotations() + [cr.rot_axis_angle(rng.normal(size=3), a) for a in rng.uniform(0, np.pi, 200)]
    for R in mats:
        assert np.array_equal(ce.bits(ce.quat_with(R)[0]), ce.bits(rr.quat_of(R))), R
    assert sorted({ce.quat_with(R)[1] for R in mats}) == [0, 1, 2, 3]


# ---- every mutant shows ----
@pytest.mark.parametrize("mutant", [m for m in ce.MUTANTS if "knife_pairs" not in ce.MUTANT_CASES[m] or m == "lt_bound"])
def test_mutant_changes_its_cases(mutant):
    names = [n for n in ce.MUTANT_CASES[mutant] if n != "knife_pairs"]
    assert len(names) >= 2
    for name in names:
        assert ce.differs(result(name, mutant), result(name)) != [], (mutant, name)


@pytest.mark.parametrize("mutant", ce.ARITH_MUTANTS + ("roles_by_lane", "lt_bound"))
def test_pair_mutant_changes_knife_pairs(mutant):
    pairs = ce.knife_pairs()
    shown = 0
    for k, p in enumerate(pairs):
        want, (i, j) = knife_result(k)
        got = knife_result(k, mutant)[0]
        expect = mutant == "lt_bound" or ("roles_swapped" if mutant == "roles_by_lane" else mutant) in p["flips"]
        assert (ce.differs(got, want) != []) == expect, (mutant, p)
        if expect:
            shown += 1
            assert "rows" in ce.differs(got, want) and not got["adj"][0, j, i]
            # roles_by_lane: lane i still takes the pair with the lower index first, lane j does not: asymmetric rows
            assert bool(got["adj"][0, i, j]) == (mutant == "roles_by_lane")
    assert shown >= 3, (mutant, shown)


@pytest.mark.parametrize("mutant", ce.ARITH_MUTANTS + ("roles_by_lane",))
def test_arithmetic_pair_mutants_leave_the_integer_cases(mutant):
    """exact arithmetic gives the same d2 and tr under any association, contraction and role order: none of the integer
    cases, the ones ON a threshold included, can show these"""
    for name in INTEGER_CASES:
        assert ce.differs(result(name, mutant), result(name)) == [], (mutant, name)


def test_mutants_leave_what_they_should():
    """cheap to state: the validity mutants change no case whose candidates are all plainly valid or rejected, the choice
    mutants none that is one clique"""
    for mutant in ("score_gt0", "frame_signed", "frame_le_n_ids", "has_ignored", "T_rot_only", "T_trans_only", "B_unchecked", "ncand_unclamped"):
        for name in ("tie", "descending", "half_turns", "full_wave"):
            assert ce.differs(result(name, mutant), result(name)) == [], (mutant, name)
    for mutant in ("total_degree", "seed_lowest_member"):
        assert ce.differs(result("full_wave", mutant), result("full_wave")) == [], mutant
    for mutant in ("no_flip", "flip_vs_lowest", "flip_le", "quat_trace_only", "quat_ge"):
        for name in ("tie", "descending", "zero_rot"):          # identity rotations: every dot is 1
            assert ce.differs(result(name, mutant), result(name)) == [], (mutant, name)


# ---- knife pairs ----
def test_knife_pairs_sit_on_the_bound_alone():
    pairs = ce.knife_pairs()
    assert len(pairs) >= 8
    for m in ce.ARITH_MUTANTS:
        assert sum(m in p["flips"] for p in pairs) >= 3, m
    src = ce.knife_source()
    for p in pairs:
        assert src["n_cand"][p["q"]] == 64 and p["lo"] < p["hi"]
        assert p["max_trans"] * p["max_trans"] == p["d2"] and 0.01 < p["d2"] < 4.0
    for name, b, p, (i, j), q in ce.knife_runs():
        tt, min_trace = cr.thresholds(p["max_trans"], ce.KNIFE_ROT)
        assert tt == p["d2"] and min_trace == KNIFE_TRACE and b["n_cand"].size == q + 1, name
        r = ce.consensus_with(b, tt, min_trace)
        g = r["gap_d2"][q]
        assert g[i, j] == 0.0 and r["adj"][q, i, j] and r["adj"][q, j, i], name
        assert (int(r["rows"][q, i]) >> j) & 1 and (int(r["rows"][q, j]) >> i) & 1, name
        assert np.count_nonzero(g <= 1e-9 * max(1.0, tt)) == 1, name
        d2, tr = ce.z_values((r["world"][0][q], r["world"][1][q]), np.array([i]), np.array([j]))
        assert d2[0] == tt and tr[0] > min_trace + 1e-6, name
        assert r["n_set"][q] >= 2
    assert {(i, j) for _, _, _, (i, j), _ in ce.knife_runs()} == set(ce.PLACEMENTS) == {(0, 1), (0, 63), (62, 63), (31, 32), (5, 40)}


# ---- exact thresholds with integer rotations ----
def test_quarter_turn_under_half_pi():
    """1 + 2 cos(pi / 2) = 1 + 1.2246e-16 rounds to the double above 1.0 (half an ulp of 1.0 is 1.1102e-16): a quarter turn,
    tr == 1 exactly, falls just short of it; so does the 3-cycle with tr == 0"""
    tt, min_trace = _thr("quarter_turn")
    assert min_trace == np.nextafter(1.0, 2.0) and tt == 1.0
    r = result("quarter_turn")
    P = (r["world"][0][0], r["world"][1][0])
    d2, tr = ce.z_values(P, np.array([0, 0, 0]), np.array([1, 2, 3]))
    assert d2.tolist() == [0.0, 0.0, 0.0] and tr.tolist() == [1.0, 0.0, 1.0]
    assert r["valid"].all() and not r["adj"][0, 0].any() and r["n_set"][0] == 1
    at_one = ce.consensus_with(ce.cases()["quarter_turn"]["batch"], tt, 1.0)          # ... and agrees through >= at 1.0 itself
    assert at_one["adj"][0, 0].tolist() == [False, True, False, True]


def test_half_turns():
    r = result("half_turns")
    assert _thr("half_turns")[1] == -1.0
    mats = [ce.I3, ce.HX, ce.HY, ce.HZ]
    for s in range(4):
        assert r["branch"][s, :4].tolist() == [(k + s) % 4 for k in range(4)]            # QUAT's w, x, y and z branch
        assert r["adj"][s][:4, :4].sum() == 12 and r["n_set"][s] == 4 and r["seed"][s] == 0 and int(r["mask"][s]) == 0xF
        assert [r["dots"][s][m] for m in range(4)] == [1.0, 0.0, 0.0, 0.0] and r["negated"][s] == []
        tr = ce.z_values((r["world"][0][s], r["world"][1][s]), np.array([0, 0, 0, 1, 1, 2]), np.array([1, 2, 3, 2, 3, 3]))[1]
        assert tr.tolist() == [-1.0] * 6                                                   # ON the bound, through >=
        assert np.array_equal(r["world"][0][s, 0], mats[s])
        # Q = (1, 1, 1, 1) whichever is the seed: the fused rotation is the 3-cycle
        assert np.array_equal(r["pose"][s].reshape(3, 4)[:, :3], ce.C3) and r["spread_trace"][s] == 0.0


@pytest.mark.parametrize("name", ["three_cycles_a", "three_cycles_b"])
def test_three_cycles(name):
    assert len(ce.zero_dot_pairs()) >= 8
    r = result(name)
    for q in range(4):
        R = r["world"][0][q]
        assert (np.trace(R[1]), np.trace(R[5])) == (0.0, 0.0) and not R[1].diagonal().any()      # tr == 0, the all-equal diagonal
        assert r["branch"][q, 1] == 3 and r["branch"][q, 5] == 3                                 # ... falls through to the last branch
        assert r["seed"][q] == 1 and r["n_set"][q] == 2 and r["dots"][q][5] == 0.0 and r["negated"][q] == []
        ws = ce.quat_with(R[1])[0][0], ce.quat_with(R[5])[0][0]
        assert (ws[0] < 0) != (ws[1] < 0)
        assert ce.quat_with(R[1], "quat_ge")[1] == 0 and ce.quat_with(R[5], "quat_ge")[1] == 0


# ---- hemisphere ----
@pytest.mark.parametrize("name", sorted(ce.HEMISPHERE_SEEDS))
def test_hemisphere(name):
    b = ce.cases()[name]["batch"]
    r = result(name)
    assert ce.cases()[name]["max_rot"] >= np.deg2rad(15.0)
    negated = 0
    for q, role in enumerate(b["roles"]):
        members = ref.members_of(r["mask"][q], 32).tolist()
        assert sorted(role["members"] + [role["seed"]]) == members and r["seed"][q] == role["seed"]
        assert members[0] == role["low"] < role["seed"] and r["degree"][q, role["seed"]] == r["degree"][q].max() == 15
        R = r["world"][0][q]
        tr = np.array([np.trace(R[m]) for m in role["members"][:8]])
        angle = np.rad2deg(np.arccos((tr - 1.0) / 2.0))
        assert ((angle > 114.0) & (angle < 126.0)).all() and (tr > 0).sum() == 4 and (tr < 0).sum() == 4
        q_low, q_seed = ce.quat_with(R[role["low"]])[0], ce.quat_with(R[role["seed"]])[0]
        assert r["branch"][q, role["low"]] == 0 and q_low[0] > 0 and q_low[3] < 0            # before tr == 0: w > 0, z < 0
        assert r["branch"][q, role["seed"]] == 3 and q_seed[0] < 0 and q_seed[3] > 0         # behind it: the z branch, w < 0
        assert r["dots"][q][role["low"]] < 0 and role["low"] in r["negated"][q]
        # X lies on the same side of the seed and of the lowest member, which lie on opposite sides of each other: the
        # rule leaves it, "negate against the lowest member" (the rule's Q negated as a whole, were it not for X) too
        qx = ce.quat_with(R[role["x"]])[0]
        assert float(qx @ q_seed) > 0.01 and float(qx @ q_low) > 0.01 and float(q_low @ q_seed) < -0.9 and role["x"] not in r["negated"][q]
        negated += len(r["negated"][q])
    assert negated >= 6
    for mutant in ("no_flip", "flip_vs_lowest"):
        assert not np.array_equal(ce.bits(result(name, mutant)["pose"]), ce.bits(r["pose"])), mutant


# ---- validity ----
@pytest.mark.parametrize("name", ["validity", "validity_rev"])
def test_validity_cases(name):
    b = ce.cases()[name]["batch"]
    r = result(name)
    n_ids = int(b["ids"].max()) + 1
    assert n_ids == 40 and 20 not in b["ids"].tolist() and b["ids"].size == 39
    assert [int(np.flatnonzero(~np.isfinite(b["poses"][i]))[0]) for i in range(12)] == list(range(12))
    lane = (lambda k: 63 - k) if name == "validity_rev" else (lambda k: k)
    for q in range(2):
        T, f, s = b["rel_pose"][q], b["cand_frame"][q], b["score"][q]
        for i in range(12):
            assert np.isnan(T[lane(i), i]) and np.isinf(T[lane(12 + i), i]) and f[lane(24 + i)] == i
        assert {float(T[lane(12 + i), i]) for i in range(12)} == {np.inf, -np.inf}
        assert s[lane(36)] == 0.0 and not np.signbit(s[lane(36)]) and s[lane(37)] == 0.0 and np.signbit(s[lane(37)])
        assert s[lane(38)] == np.inf and np.isnan(s[lane(39)])
        assert [int(f[lane(k)]) for k in range(40, 45)] == [-1, n_ids - 1, n_ids, 2 ** 31 - 1, 20]
        want_valid = sorted(lane(k) for k in [36, 37, 38, 41] + list(range(45, 64)))
        assert np.flatnonzero(r["valid"][q]).tolist() == want_valid and r["n_valid"][q] == 23
    assert r["n_set"].tolist() == [22, 23] and np.isfinite(r["support_score"][0]) and r["support_score"][1] == np.inf
    assert not (int(r["mask"][0]) >> lane(38)) & 1 and (int(r["mask"][1]) >> lane(38)) & 1


def test_n_cand_cases():
    r = result("ncand")
    assert ce.cases()["ncand"]["batch"]["n_cand"].tolist() == [70, -1, 64]
    assert r["n_valid"].tolist() == [64, 0, 64] and (r["degree"][1] == -1).all() and ce.differs(
        {k: v[:1] for k, v in r.items() if k in ce.INT_KEYS + ce.DBL_KEYS + ("rows", "degree", "pick")},
        {k: v[2:] for k, v in r.items() if k in ce.INT_KEYS + ce.DBL_KEYS + ("rows", "degree", "pick")}) == []      # 70 counts as 64
    r = result("ncand_cn3")
    assert ce.cases()["ncand_cn3"]["batch"]["n_cand"].tolist() == [5, 3, 2] and r["n_valid"].tolist() == [3, 3, 2]
    assert result("ncand_cn3", "ncand_unclamped")["n_valid"].tolist() == [5, 3, 2]
    r = result("cn1")
    assert ce.cases()["cn1"]["batch"]["score"].shape == (4, 1) and r["n_valid"].tolist() == [1, 1, 0, 0] and r["n_set"].tolist() == [1, 1, 0, 0]
    assert r["degree"][:, 0].tolist() == [0, 0, -1, -1] and np.isnan(r["pose"][2:]).all() and r["spread_t2"][:2].tolist() == [0.0, 0.0]


# ---- choice ----
def test_choice_cases():
    r = result("isolated")
    assert r["n_valid"][0] == 8 and (r["degree"][0] == 0).all() and r["seed"][0] == 0 and r["n_set"][0] == 1 and int(r["mask"][0]) == 1
    r = result("descending")
    members = [10, 20, 30, 40, 63]
    assert r["pick"][0, members].tolist() == [4, 3, 2, 1, 0] and r["seed"][0] == 63 and r["n_set"][0] == 5
    assert r["degree"][0, members].tolist() == [4, 5, 6, 7, 8] and (r["pick"][0] >= 0).sum() == 5
    r = result("remaining_degree")
    assert r["degree"][0, :25].tolist() == [16, 15] + [12] * 6 + [8] * 8 + [11] * 5 + [1] * 4
    assert ref.members_of(r["mask"][0], 32).tolist() == [0] + list(range(2, 8)) + list(range(16, 21)) and r["pick"][0, 2] == 1
    assert ref.members_of(result("remaining_degree", "total_degree")["mask"][0], 32).tolist() == list(range(8))
    r = result("remaining_degree_rev")
    assert r["degree"][0, 0] == 16 and r["degree"][0, 24] == 15 and r["n_set"][0] == 12 and not (int(r["mask"][0]) >> 24) & 1
    r = result("full_wave")
    assert r["n_set"].tolist() == [64, 63, 63] and int(r["mask"][0]) == 2 ** 64 - 1 and r["pick"][0].tolist() == list(range(64))
    assert r["pick"][1, 17] == -1 and r["degree"][1, 17] == -1 and r["degree"][2, 0] == 0 and r["seed"][2] == 1
    # 63 rounds of the plain greedy, no shortcut on the way: a clique minus one edge
    for name, left_out, first in (("chain_high", 63, 0), ("chain_low", 1, 2)):
        r = result(name)
        assert r["n_set"][0] == 63 and r["pick"][0].max() == 62 >= 40 and r["pick"][0, left_out] == -1 and r["seed"][0] == first
        adj, valid = r["adj"][0], r["valid"][0]
        P, rounds = valid.copy(), 0
        while P.any():
            idx = np.flatnonzero(P)
            d = adj[np.ix_(idx, idx)].sum(1)
            if (d == idx.size - 1).all():
                break
            P &= adj[idx[int(np.argmax(d))]]
            rounds += 1
        assert rounds >= 62, (name, rounds)          # (the shortcut could fire only over the last one left)
    assert result("chain_low")["pick"][0, 0] == 62


# ---- the order of the sums ----
@pytest.mark.parametrize("name", sorted(ce.SUM_ORDER_SEEDS))
def test_sum_order(name):
    b = ce.cases()[name]["batch"]
    r = result(name)
    members = ref.members_of(r["mask"][0], 64)
    assert members.size >= 20 and r["n_valid"][0] == 64
    t = r["world"][1][0][members]
    assert np.abs(t).min(0).max() > 9e4 and 0.03 < t.std(0).min() and t.std(0).max() < 0.3          # 1e5 m, 0.1 m of noise
    s = b["score"][0][members]
    assert s.min() == 1.0 and s.max() == 1e15 and np.unique(np.floor(np.log10(s))).size >= 8
    order = members[np.argsort(r["pick"][0][members])]
    assert not np.array_equal(order, members) and order[0] == r["seed"][0] != members[0]
    changed = ce.differs(result(name, "sum_pick_order"), r)
    assert "pose" in changed and "support_score" in changed and set(changed) <= set(ce.DBL_KEYS), changed


# ---- stale outputs ----
def test_stale_pair():
    first, second = ce.stale_pair()
    assert first["n_cand"].tolist() == [64] * 5 and first["score"].shape == second["score"].shape == (5, 64)
    a, z = result("stale_first"), result("stale_second")
    assert (a["n_valid"] == 64).all() and (a["n_set"] == 64).all() and (a["seed"] == 0).all() and (a["mask"] == np.uint64(2 ** 64 - 1)).all()
    assert (a["degree"] == 63).all() and (a["rows"] != 0).all() and np.array_equal(a["pick"], np.tile(np.arange(64), (5, 1)))
    assert np.isfinite(a["pose"]).all() and (a["support_score"] > 0).all() and (a["spread_t2"] > 0).all() and (a["spread_trace"] < 3.0).all()
    assert second["n_cand"].tolist() == [0, 64, 1, 64, 40] and (second["score"][1] < 0).all()
    assert z["n_valid"].tolist()[:3] == [0, 0, 1] and z["n_set"].tolist()[:3] == [0, 0, 1] and z["seed"].tolist()[:3] == [-1, -1, 0]
    assert np.isnan(z["pose"][:2]).all() and (z["degree"][:2] == -1).all() and (z["rows"][:3] == 0).all() and z["spread_t2"][2] == 0.0
    # every word of the five queries' outputs differs between the two, or is a default in the second
    assert (z["pick"][:2] == -1).all() and z["pick"][2].tolist() == [0] + [-1] * 63


# ---- the noisy cases keep clear of the thresholds ----
@pytest.mark.parametrize("name", [n for n in CASES if ce.cases()[n]["noisy"]])
def test_noisy_cases_are_clear_of_the_thresholds(name):
    tt, min_trace = _thr(name)
    r = ce.reference(ce.cases()[name]["batch"], tt, min_trace)
    assert ref.clear_of_thresholds(r, tt, min_trace), (name, r["min_gap_d2"], r["min_gap_tr"])


def test_every_case_is_small_and_grouped():
    grouped = [n for g in ce.CASE_GROUPS.values() for n in g]
    assert sorted(grouped + ["stale_first", "stale_second"]) == CASES
    for name in CASES:
        s = ce.cases()[name]["batch"]["score"]
        assert s.shape[0] <= 64 and s.shape[1] <= 64, name
    for m, names in ce.MUTANT_CASES.items():
        assert all(n == "knife_pairs" or n in ce.cases() for n in names), m
