"""The workloads of tests/test_gpu_build_edges.py, checked without a GPU: a plain restatement of BuildSingleScanSTD
(tests/_build_edges.py, written from STDesc.cpp:174-315) equals the oracle bit for bit on every frame of every family,
the workloads really reach the construction's edges, and named mutants of the restatement are caught by their family.

Reached (counts of the restatement's own bookkeeping; the assertions below hold floors well under them):
  limits         kept sides equal to min_len 24, to max_len 90 (8 of them |p1 p2|); dropped one f32 step of a coordinate outside 45 / 54; kept
                 as close inside 48 / 66; min_len_margin 0.0; a key field of 2097125 (21 bits)
  equal_sides    each of the four kinds in all six keypoint orders; the unequal side in every raw slot for the two
                 isosceles kinds (slot p1p2 only through near-tie triangles), slots p1p3 and p2p3 for right isosceles;
                 equal sides at the first / second / third swap 120 / 104 / 168 times, the first swap fired 24 times
  milli          41 keys shared by different triangles, 55 sub-millimetre pairs that both stay, 48 triplets decided
                 differently by an f64 truncation
  contention     16872 claimants of one key, a loser 35994 triplets after its winner; T = 2^k - 1: n_desc = T for
                 K = 3 (63, 127, 1023), and 45/63, 175/255, 762/1023, 160/255, 2868/4095, 2805/4095, 2353/4095 for
                 K >= 4, each the number of different triangles
  ties           2896 keypoints whose tie decides membership, 2245 with tied members in different quarters, 50 whose
                 own index is not at rank 0
  degenerate     49 zero sides, 74 NaN cosines (inf cannot occur), 175 cosines of exactly 1, 27 of exactly 0
  mutants        frames that differ: filter_ge 66, swap1_ge 120, swap2_ge 104, swap3_ge 168, key_f64 48, last_wins 96,
                 ties_high 21, assoc 3; self_first 0 (an equivalent mutant, see _build_edges.EQUIVALENT_MUTANTS)
Run time on the development machine: 38 s (tests/test_select_edges.py: 8 s); the restatement's Python loop over 1.5e6
triplets of the shapes and mixed_batches families is most of it.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _build_edges as be  # noqa: E402

_RUNS = {}


def runs(name, oracle_mod):
    """[(cfg, xyz, label, restatement, oracle descriptors)] of one family, once"""
    if name not in _RUNS:
        out = []
        for cfg, frames in be.family(name):
            o = oracle_mod.OracleManager(**cfg)
            for xyz, lab in frames:
                out.append((cfg, xyz, lab, be.ref_build(xyz, lab, cfg), o.build(xyz, lab)))
        _RUNS[name] = out
    return _RUNS[name]


def audit(oracle_mod, rows):
    acc = {}
    for cfg, xyz, lab, _, _ in rows:
        key = tuple(sorted(cfg.items()))
        if key not in acc:
            acc[key] = (oracle_mod.OracleManager(**cfg), oracle_mod.OrcAudit())
        acc[key][0].audit_build(xyz, lab, acc[key][1])
    return [a.as_dict() for _, a in acc.values()]


@pytest.mark.parametrize("name", list(be.FAMILIES))
def test_restatement_equals_the_oracle_bit_for_bit(name, oracle_mod):
    n_desc = 0
    for k, (cfg, xyz, lab, r, d) in enumerate(runs(name, oracle_mod)):
        assert be.desc_bits_equal(r, d) == "", (name, k, cfg, len(xyz))
        n_desc += r.n
    assert n_desc > 100


def test_bit_comparison_tells_zeros_apart_and_nans_not():
    z = np.zeros(3)
    assert be.field_bits_equal(z, z.copy()) and not be.field_bits_equal(z, -z)
    assert not be.field_bits_equal(np.zeros(3, np.float32), -np.zeros(3))
    n1 = np.array([np.nan, 1.0])
    n2 = np.array([-np.nan, 1.0])
    assert be.field_bits_equal(n1, n2) and not be.field_bits_equal(n1, np.array([np.inf, 1.0]))
    assert be.field_bits_equal(np.float32([1.5, -0.0]), np.float64([1.5, -0.0]))
    assert not be.field_bits_equal(np.float64([1.0]), np.float64([np.nextafter(1.0, 2.0)]))


def _emitted_raw(r):
    return [r.raw[t] for t in r.t.tolist()]


def limit_counts(rows, tol=2.5e-7):
    """kept sides equal to a limit, dropped sides within one f32 step of a coordinate outside it, kept ones as close
    inside"""
    c = dict(min_at=0, max_at=0, max_at_p1p2=0, min_out=0, max_out=0, min_in=0, max_in=0)
    for cfg, _, _, r, _ in rows:
        lo, hi = cfg["descriptor_min_len"], cfg["descriptor_max_len"]
        for raw in _emitted_raw(r):
            c["min_at"] += sum(s == lo for s in raw)
            c["max_at"] += sum(s == hi for s in raw)
            c["max_at_p1p2"] += raw[0] == hi
            c["min_in"] += sum(lo < s <= lo * (1 + tol) for s in raw)
            c["max_in"] += sum(hi * (1 - tol) <= s < hi for s in raw)
        for t in np.nonzero(r.state == 0)[0].tolist()[:1]:            # (a frame is one triangle, three times)
            c["min_out"] += sum(lo * (1 - tol) <= s < lo for s in r.raw[t])
            c["max_out"] += sum(hi < s <= hi * (1 + tol) for s in r.raw[t])
    return c


def test_limits_are_reached(oracle_mod):
    rows = runs("limits", oracle_mod)
    assert min(a["min_len_margin"] for a in audit(oracle_mod, rows)) == 0.0
    c = limit_counts(rows)
    assert all(v >= 8 for v in c.values()), c
    # the 21-bit key fields at their largest: a kept side at the largest max_len check_cfg accepts with an exact side
    assert any(k[2] >= 2097125 for _, _, _, r, _ in rows for k in r.claims)


def equal_side_counts(rows):
    """kind -> the index orders (0..5) among emitted descriptors, kind -> raw slots (0 p1p2, 1 p1p3, 2 p2p3) that held
    the unequal side, and the emitted descriptors whose first / second / third swap had equal sides to decide or a
    first swap that fired"""
    orders, slots = {k: set() for k in be.KINDS}, {k: set() for k in be.KINDS}
    dec = dict(swap1_equal=0, swap2_equal=0, swap3_equal=0, swap1_fired=0)
    for k, (_, _, _, r, _) in enumerate(rows):
        for raw in _emitted_raw(r):
            kind = be.kind_of(*sorted(raw))
            if kind is None:
                continue
            orders[kind].add(k % 6)
            if kind != "equilateral":
                slots[kind].add([j for j in range(3) if list(raw).count(raw[j]) == 1][0])
            a, b, c = raw
            dec["swap1_equal"] += a == b
            dec["swap1_fired"] += a > b
            if a > b:
                a, b = b, a
            dec["swap2_equal"] += b == c
            if b > c:
                b, c = c, b
            dec["swap3_equal"] += a == b
    return orders, slots, dec


def test_equal_sides_are_reached(oracle_mod):
    """the unequal side of an exactly isosceles triangle sits in two of the three raw slots only: p2 and p3 come in
    k-NN order, so |p1 p2| <= |p1 p3| but for f32 rounding.  The near-tie triangles (equal f32 squared distances, f64
    sides a hair apart) are what makes the first swap fire."""
    orders, slots, dec = equal_side_counts(runs("equal_sides", oracle_mod))
    for kind in be.KINDS:
        assert orders[kind] == set(range(6)), (kind, orders)
    assert slots["two_short_equal"] == {0, 1, 2} and slots["two_long_equal"] == {0, 1, 2} and slots["right_isosceles"] == {1, 2}, slots
    assert min(dec.values()) >= 8, dec


def milli_counts(rows):
    c = dict(collisions=0, sub_mm_pairs=0, f64_flips=0)
    for cfg, xyz, lab, r, _ in rows:
        for key, ts in r.claims.items():
            c["collisions"] += len({tuple(sorted(r.raw[t])) for t in ts}) > 1
        em = [tuple(sorted(raw)) for raw in _emitted_raw(r)]
        for i in range(len(em)):
            for j in range(i + 1, len(em)):
                c["sub_mm_pairs"] += all(abs(u - v) < 1e-3 for u, v in zip(em[i], em[j]))
        c["f64_flips"] += int(np.sum(r.state != be.ref_build(xyz, lab, cfg, mutant="key_f64").state))
    return c


def test_millimetre_keys_are_reached(oracle_mod):
    c = milli_counts(runs("milli", oracle_mod))
    assert all(v >= 8 for v in c.values()), c


def contention_counts(rows):
    c = dict(max_claimants=0, max_loser_distance=0, full_tables=[])
    for cfg, xyz, _, r, _ in rows:
        for ts in r.claims.values():
            c["max_claimants"] = max(c["max_claimants"], len(ts))
            c["max_loser_distance"] = max(c["max_loser_distance"], ts[-1] - ts[0])
        K, n = cfg["descriptor_near_num"], len(xyz)
        if (K, n) in be.FULL_TABLES:
            T = n * be.tpi_of(K)
            sets = {frozenset((i, int(r.nn[i, m]), int(r.nn[i, q]))) for i in range(n) for m in range(1, K - 1) for q in range(m + 1, K)}
            c["full_tables"].append((K, n, T, int(np.sum(r.state > 0)), r.n, len(sets)))
    return c


def test_contention_is_reached(oracle_mod):
    """a frame of T = 2^k - 1 triplets has a dedup table of T + 1 slots.  With K = 3 (points on a circle) every triplet
    is its own triangle and the table is full but for one slot.  With K >= 4 two neighbours that see each other find
    the same triangle twice, whatever the points: there every triplet is valid and every collision is a triangle found
    again, never two triangles that share millimetres."""
    c = contention_counts(runs("contention", oracle_mod))
    assert c["max_claimants"] >= 200 and c["max_loser_distance"] >= 4 * be.BUILD_THREADS, c
    assert len(c["full_tables"]) == len(be.FULL_TABLES)
    for K, n, T, valid, n_desc, triangles in c["full_tables"]:
        assert T & (T + 1) == 0 and valid == T and n_desc == triangles, (K, n)
        if K == 3:
            assert n_desc == T, (K, n)


def _d2_row(x, i):
    d = x[i][None, :] - x
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def tie_counts(rows):
    c = dict(membership=0, across_quarters=0, self_not_first=0)
    for cfg, xyz, _, r, _ in rows:
        K, n = cfg["descriptor_near_num"], len(xyz)
        for i in np.nonzero(r.d2[:, K - 1] == r.d2[:, K])[0].tolist():
            c["membership"] += 1
            group = np.nonzero(_d2_row(xyz, i) == r.d2[i, K - 1])[0]
            c["across_quarters"] += be.parts_of(K) == 4 and len({be.quarter_of(j, n) for j in group.tolist()}) > 1
        c["self_not_first"] += int(np.sum(r.nn[:, 0] != np.arange(n)))
    return c


def test_ties_are_reached(oracle_mod):
    rows = runs("ties", oracle_mod)
    lattice = [row for row in rows if len(row[1]) >= 144]
    for a in audit(oracle_mod, lattice):
        assert 2 * a["knn_tied_points"] >= a["knn_points"] > 0, a
    c = tie_counts(rows)
    assert c["membership"] >= 20 and c["across_quarters"] >= 10 and c["self_not_first"] >= 3, c
    assert {cfg["descriptor_near_num"] for cfg, _, _, _, _ in rows} >= {8, 9, 10, 12, 16}
    assert any(len(xyz) > be.lds_switch(10) for cfg, xyz, _, _, _ in rows if cfg["descriptor_near_num"] == 10)


def test_shapes_and_batches_are_tie_free_and_complete(oracle_mod):
    from sgtd_amd import synth
    seen = {}
    for name in ("shapes", "mixed_batches"):
        for cfg, frames in be.family(name):
            K = cfg["descriptor_near_num"]
            for xyz, _ in frames:
                assert len(xyz) < 2 or not synth.has_knn_ties(xyz, min(K, len(xyz) - 1)), (name, K, len(xyz))
                if name == "shapes":
                    seen.setdefault(K, set()).add(len(xyz))
    assert set(seen) == set(be.SHAPE_KS)
    for K in be.SHAPE_KS:
        assert seen[K] == set(be.shape_sizes(K)), K
        assert {K - 1, K, K + 1} <= seen[K] and ({256, 257, 513} if K >= 9 else {1024, 1025}) <= seen[K]
    # the network sizes: every KM of the kernel, and K below its KM
    assert {4: 4, 5: 8, 7: 8, 8: 8, 9: 10, 10: 10, 11: 12, 12: 12, 13: 16, 16: 16}.keys() <= seen.keys()
    for K in be.SWITCH_KS:
        s, top = be.lds_switch(K), be.largest_n(K)
        assert be.lds_bytes(s, K, True) <= be.LDS_LIMIT < be.lds_bytes(s + 1, K, True)
        assert be.lds_bytes(top, K, False) <= be.LDS_LIMIT < be.lds_bytes(top + 1, K, False)
        assert {s - 1, s, s + 1, top} <= seen[K] and be.REFUSED[K] == top + 1
    b1, b2, b3 = (frames for _, frames in be.family("mixed_batches"))
    big = be.lds_switch(be.MIXED_K) + 1
    for b in (b1, b2):
        sizes = [len(f[0]) for f in b]
        assert {0, be.MIXED_K - 1, be.MIXED_K, big} <= set(sizes) and any(150 <= n <= 201 for n in sizes)
    assert len(b2) >= 1100 and len(b3) > 512 and max(len(f[0]) for f in b3) <= be.lds_switch(be.MIXED_K)
    allx = [f[0].tobytes() for b in (b1, b2, b3) for f in b if len(f[0])]
    assert len(set(allx)) == len(allx)                      # every frame its own points


def degenerate_counts(rows):
    c = dict(zero_sides=0, nan_angles=0, inf_angles=0, cos_one=0, cos_zero=0)
    for _, _, _, r, _ in rows:
        c["zero_sides"] += int(np.sum(r.side == 0))
        c["nan_angles"] += int(np.sum(np.isnan(r.angle)))
        c["inf_angles"] += int(np.sum(np.isinf(r.angle)))
        c["cos_one"] += int(np.sum(r.angle == 1.0))
        c["cos_zero"] += int(np.sum(r.angle == 0.0))
    return c


def test_degenerate_values_are_reached(oracle_mod):
    """(a zero side comes with two equal other sides, so a cosine's numerator is 0 when its denominator is: NaN, never
    inf)"""
    c = degenerate_counts(runs("degenerate", oracle_mod))
    assert c["zero_sides"] >= 20 and c["nan_angles"] >= 20 and c["cos_one"] >= 20 and c["cos_zero"] >= 20, c
    lab = np.concatenate([r.label.ravel() for _, _, _, r, _ in runs("extras", oracle_mod)])
    assert {0, 16, 65536, 2 ** 31 - 1} <= set(lab.tolist())
    assert any(np.isinf(r.d2).any() for _, _, _, r, _ in runs("extras", oracle_mod))     # the f32 distance overflows


MUTANT_FAMILY = dict(be.MUTANTS)


@pytest.mark.parametrize("mutant", list(MUTANT_FAMILY))
def test_mutant_of_the_restatement_is_caught_by_its_family(mutant, oracle_mod):
    name = MUTANT_FAMILY[mutant]
    caught = sum(be.desc_bits_equal(be.ref_build(xyz, lab, cfg, mutant=mutant), d) != "" for cfg, xyz, lab, _, d in runs(name, oracle_mod))
    assert caught >= 1, "the %s family does not notice the mutant %s" % (name, mutant)


@pytest.mark.parametrize("mutant", be.EQUIVALENT_MUTANTS)
def test_equivalent_mutant_changes_nothing(mutant, oracle_mod):
    """(see _build_edges.EQUIVALENT_MUTANTS: stated, so that nobody looks for a workload that cannot exist)"""
    n = 0
    for name in ("ties", "degenerate"):
        for cfg, xyz, lab, r, d in runs(name, oracle_mod):
            m = be.ref_build(xyz, lab, cfg, mutant=mutant)
            assert be.desc_bits_equal(m, d) == ""
            n += int(np.sum(m.nn != r.nn)) if len(xyz) >= cfg["descriptor_near_num"] else 0
    assert n > 0                              # (the mutant did change neighbour lists)


if __name__ == "__main__":            # the counts of the module docstring
    from oracle import oracle
    oracle.build_library()
    print("limits       ", limit_counts(runs("limits", oracle)))
    print("equal_sides  ", equal_side_counts(runs("equal_sides", oracle)))
    print("milli        ", milli_counts(runs("milli", oracle)))
    print("contention   ", contention_counts(runs("contention", oracle)))
    print("ties         ", tie_counts(runs("ties", oracle)))
    print("degenerate   ", degenerate_counts(runs("degenerate", oracle)))
    for m, fam in MUTANT_FAMILY.items():
        print("mutant %-10s frames of %s that differ: %d" % (m, fam, sum(
            be.desc_bits_equal(be.ref_build(x, l, c, mutant=m), d) != "" for c, x, l, _, d in runs(fam, oracle))))
