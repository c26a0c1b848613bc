"""The workloads of tests/test_gpu_filter_edges.py, checked without a GPU: the restatement of the frame-filter rule
(tests/_filter_edges.py) equals the oracle that holds only the allowed frames on every case and filter, every family
reaches the edges it is named for (asserted on the workloads themselves), every mutant of the restatement changes the
expected answer of a named case, and the position prior's rule (test_position_prior_host.prior_rows) decides its edge
cases as the header states."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _filter_edges as fe  # noqa: E402
from test_position_prior_host import prior_rows  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rec, se = fe.rec, fe.se


@pytest.fixture(scope="module")
def world():
    """name -> (case, {filter name: the restatement's answer})"""
    out = {}
    for c in fe.cases():
        out[c.name] = (c, {f.name: fe.ref_filtered(c, 0, f) for f in c.filters})
    return out


def _filt(c, name):
    return next(f for f in c.filters if f.name == name)


def test_restatement_equals_the_oracle_of_the_allowed_frames(world, oracle_mod):
    n = 0
    for name, (c, ours) in world.items():
        side, label, frame = c.entry_arrays()
        for f in c.filters:
            a = ours[f.name]
            held = a["held"]
            o = oracle_mod.OracleManager(**c.config())
            o.add(c._descs(oracle_mod, side[held], label[held], frame[held]))
            b = o.select(c.query_descs(oracle_mod, 0))
            where = "%s %s" % (name, f.name)
            np.testing.assert_array_equal(a["votes"], o.votes(), err_msg=where)
            assert a["M"] == o.counters()["M"], where
            for key in fe.KEYS:
                np.testing.assert_array_equal(a[key], b[key], err_msg=where + " " + key)
            r = o.rough_matches()
            for key in ("q_idx", "cell", "db_entry", "frame", "dis"):
                np.testing.assert_array_equal(a["rough"][key], r[key], err_msg=where + " rough " + key)
            # the filter pass restated over the records of the whole table gives the same answer
            assert fe.same(fe.ref_by_records(c, 0, f), a), where
            n += 1
    assert n == sum(len(c.filters) for c, _ in world.values()) >= 150


def test_header_constants_equal_the_helper_copies():
    src = open(os.path.join(ROOT, "sgtd_amd", "csrc", "filter_kernels.hip.h")).read()
    src += open(os.path.join(ROOT, "sgtd_amd", "csrc", "sgtd_accel.hip")).read()
    assert "lane * 4u < m" in src and "k = (u32)lane + SGTD_WAVE; k * 4u < m" in src and fe.FILT_PREFETCH == 4 * rec.WAVE
    m = re.search(r"if \(lds <= (\d+)\)\s+filter_records_kernel<true>", src)
    assert m and int(m.group(1)) * 8 == fe.LDS_FRAMES


# ---- every family reaches its edges --------------------------------------------------------------------------------
def test_lists_reaches(world):
    lengths, quad_kill, tail_kill, past = set(), set(), {}, {256: set(), 512: set()}
    for L in fe.LIST_LENGTHS:
        c, ours = world["lists/L%d" % L]
        assert c.stamped and c.info["L"] == L and len(c.frames()) == L + 3
        lengths.add(len(fe.list_positions(c, 0, c.filters[0])[0]))
        for f in c.filters:
            fr, killed = fe.list_positions(c, 0, f)
            np.testing.assert_array_equal(fr, np.arange(L))               # record j of the list is frame j
            j = np.arange(L)
            quad_kill |= set((j[killed] % 4).tolist())
            tail = j >= (L // 4) * 4                                       # the records of a last, partial quad
            if L % 4:
                tail_kill.setdefault(L % 4, set()).update((j[killed & tail] % 4).tolist())
                if killed[-1]:
                    tail_kill.setdefault(("last", L % 4), set()).add(L)
            for lim in (256, 512):
                past[lim] |= {("killed", bool(x)) for x in killed[j >= lim]}
            # the votes say which record died, M how many
            a = ours[f.name]
            want = np.zeros(c.max_frame_n)
            al = fe.filt_allows(f, 0, c.frames())
            want[c.frames()[al]] = fe.BOOST
            want[fr[~killed]] += 1
            np.testing.assert_array_equal(a["votes"], want)
            assert a["M"] == int((~killed).sum()) + fe.BOOST * int(al.sum())
    assert lengths == set(fe.LIST_LENGTHS)
    assert quad_kill == {0, 1, 2, 3}
    assert tail_kill[1] == {0} and tail_kill[2] == {0, 1} and tail_kill[3] == {0, 1, 2}
    assert all(tail_kill[("last", m)] for m in (1, 2, 3))                  # the last record of a partial quad killed
    for lim in (256, 512):
        assert past[lim] == {("killed", True), ("killed", False)}
    # the shard filter: a range that starts off a block border and ends inside the table, flips at 63 | 64 and 127 | 128
    for L in (255, 256, 257, 260, 511, 513, 1030):
        c, _ = world["lists/L%d" % L]
        f = _filt(c, "shard")
        assert f.lo % 64 != 0 and f.lo + f.n < L + 3
        assert fe.filt_allows(f, 0, [63, 64, 127, 128]).tolist() == [True, False, False, True]


def test_slots_reaches(world):
    assert [len(world["slots/n%d" % n][0].queries[0]) for n in fe.SLOT_COUNTS] == [1, 63, 64, 65, 257, 600]
    for n in fe.SLOT_COUNTS:
        c, ours = world["slots/n%d" % n]
        for f in c.filters:
            a = ours[f.name]
            al = fe.filt_allows(f, 0, np.arange(12))
            assert 0 < al.sum() < 12 and np.all((a["votes"][:12] > 0) == al)
            assert sorted(a["cand_frame"].tolist()) == (np.nonzero(al)[0].tolist() if n > 1 else [])
        if n > 1:
            lengths = np.bincount(c.records(0)[0], minlength=n)
            assert set(lengths[:n - 1].tolist()) == set(range(1, min(n, 6)))       # lists of 1 .. 5 records


def _dead_positions(c, desc):
    """the list of descriptor `desc` with its undecided records: (frame, already dead) per record, the records within
    1e-12 (relative) beyond the threshold taken as the ones the sweep leaves to the f64 test"""
    rq, _, re_ = c.records(0, 1.0 + 1e-12)
    e = re_[rq == desc]
    side, frame, _ = c.full_table().arrays()
    qs = rec.key_sides_labels(c.queries[0][desc:desc + 1])[0][0]
    thr = float(se.norm3(qs)) * rec.ROUGH
    d = se.norm3(side[e] - qs)
    assert np.all(d < thr * (1.0 + 1e-12))
    return frame[e].astype(np.int64), d >= thr


def test_dead_reaches(world):
    c, ours = world["dead/ladder"]
    fr, is_dead = _dead_positions(c, 0)
    assert is_dead.sum() >= 5 and c.n_dead(0) == int(is_dead.sum()) and (~is_dead).sum() >= 15
    shared = {}
    for f in c.filters:
        killed = ~fe.filt_allows(f, 0, fr) & ~is_dead
        quads = np.arange(len(fr)) // 4
        shared[f.name] = len(set(quads[killed].tolist()) & set(quads[is_dead].tolist()))
        # M loses each killed record once and an already-dead one never
        al = fe.filt_allows(f, 0, c.frames())
        assert ours[f.name]["M"] == int((~is_dead & ~killed).sum()) + fe.BOOST * int(al.sum())
    assert shared["no_live"] >= 2 and shared["half_live"] >= 1 and shared["all"] == 0
    # inside and beyond the threshold alternate, so a quad holds both wherever the undecided records begin
    sh = np.asarray(c.info["shifts"])
    assert np.all((sh[:-1:2] < 1) & (sh[1::2] >= 1))


def test_bits_reaches(world):
    for span in fe.BIT_SPANS:
        c, ours = world["bits/span%d" % span]
        assert c.table_lo == fe.TABLE_LO and c.span == span and not c.stamped
        loc = np.array([0, 63, 64, 65, span - 1])
        seen = {int(l): set() for l in loc}
        offsets, ends = set(), set()
        for f in c.filters:
            if f.name in ("below", "above"):
                assert ours[f.name]["M"] == 0 and f.rows.all()
                assert (f.lo + f.n <= fe.TABLE_LO) if f.name == "below" else (f.lo >= fe.TABLE_LO + span)
                continue
            offsets.add(f.lo - fe.TABLE_LO)
            ends.add("inside" if f.lo + f.n < fe.TABLE_LO + span else "past")
            al = fe.filt_allows(f, 0, fe.TABLE_LO + loc)
            for l, a in zip(loc, al):
                seen[int(l)].add(bool(a))
            if f.n % 64:               # bits at and beyond n_frames are set: frames the range does not cover
                assert int(f.rows[0, -1] >> np.uint64(f.n % 64)) == (1 << (64 - f.n % 64)) - 1
        assert offsets == set(fe.BIT_OFFSETS) and ends == {"inside", "past"}
        assert all(v == {True, False} for v in seen.values()), seen
    assert sorted(s % 64 for s in fe.BIT_SPANS) == [0, 1, 63]


def test_wide_reaches(world):
    spans = []
    for span in fe.WIDE_SPANS:
        c, ours = world["wide/span%d" % span]
        assert c.span == span and c.table_lo == fe.TABLE_LO and c.max_frame_n == 600000 and 20 <= len(c.frames()) <= 48
        words = (span + 63) // 64
        spans.append(words * 8)
        loc = c.frames() - fe.TABLE_LO
        assert {0, span - 1} <= set(loc.tolist())
        border = [w for w in set((loc // 64).tolist()) if w * 64 in loc and w * 64 - 1 in loc]
        assert any(w > 1000 for w in border) and any(w == words - 1 or w == words - 2 for w in border)
        for f in c.filters:
            al = fe.filt_allows(f, 0, c.frames())
            assert 0 < al.sum() < len(al) and ours[f.name]["M"] == (fe.BOOST + 1) * int(al.sum())
        assert {bool(fe.filt_allows(f, 0, [fe.TABLE_LO + span - 1])[0]) for f in c.filters} == {True, False}
    assert spans[0] == 65536 and spans[1] > 65536                       # the last LDS launch and the first from memory


def test_rough_reaches(world):
    c, ours = world["rough/steps"]
    lengths = np.bincount(c.records(0)[0], minlength=len(c.queries[0]))
    assert tuple(lengths[:len(fe.ROUGH_LENGTHS)]) == fe.ROUGH_LENGTHS
    fr, is_dead = _dead_positions(c, len(fe.ROUGH_LENGTHS))
    assert is_dead.sum() >= 5
    n = {k: len(v["rough"]["q_idx"]) for k, v in ours.items()}
    assert n["none"] == 0 and 0 < n["alternating"] < n["all"] == len(c.records(0)[0])
    kept = np.isin(c.full_table().arrays()[1][c.records(0)[2]], np.arange(1, 200, 2))
    assert n["alternating"] == int(kept.sum())


# ---- mutants -------------------------------------------------------------------------------------------------------
CAUGHT_BY = {
    "f_le_span": ("bits/span129", "s-65/inside/off"), "bit31": ("bits/span128", "s-1/past/on"),
    "word_border": ("bits/span191", "s+1/past/on"), "tail_last_ignored": ("lists/L5", "last"),
    "past256_ignored": ("lists/L257", "last"), "dead_twice": ("dead/ladder", "half_live"),
    "shift_sign": ("bits/span129", "s+1/past/on"), "no_last_mask": ("lists/L257", "shard"),
}


@pytest.mark.parametrize("mutant", [m for m in fe.MUTANTS if m != "row0"])
def test_mutant_is_caught(world, mutant):
    name, fname = CAUGHT_BY[mutant]
    c, ours = world[name]
    caught = [(n, f.name) for n, (cc, oo) in world.items() for f in cc.filters
              if (n, f.name) == (name, fname) and not fe.same(fe.ref_filtered(cc, 0, f, mutant=mutant), oo[f.name])]
    assert caught, "%s is not caught by %s %s" % (mutant, name, fname)


def test_every_mutant_changes_some_answer_in_every_family_it_belongs_to(world):
    """the wide family catches the row mutants too (the row read from LDS and from memory)"""
    for span in fe.WIDE_SPANS:
        c, ours = world["wide/span%d" % span]
        for mutant in ("bit31", "word_border", "shift_sign"):
            assert any(not fe.same(fe.ref_filtered(c, 0, f, mutant=mutant), ours[f.name]) for f in c.filters), mutant


def test_row0_mutant_is_caught_by_the_keypoint_batch(oracle_mod):
    """per-query rows exist only for batches: every query of the keypoint batch answers differently under row 0 and under
    the row before its own"""
    from sgtd_amd import synth
    m, qs, gt, filters = fe.kp_world(synth)
    assert len(set(gt.tolist())) == fe.KP_QUERIES
    ob = oracle_mod.OracleManager()
    descs = []
    for i in range(fe.KP_FRAMES):
        ob.set_current_frame_id(fe.TABLE_LO + i)
        descs.append(ob.build(m.xyz[i], m.label[i]))
    ids = fe.TABLE_LO + np.arange(fe.KP_FRAMES)

    def answer(filt, row, q, mutant=None):
        o = oracle_mod.OracleManager()
        for i in np.nonzero(fe.filt_allows(filt, row, ids, fe.TABLE_LO, mutant))[0]:
            o.add(descs[i])
        o.set_current_frame_id(fe.TABLE_LO + fe.KP_FRAMES)
        o.build(qs.xyz[q], qs.label[q], export=False)
        r = o.select()
        return r["cand_frame"].tolist(), r["cand_votes"].tolist()

    for name in ("per_query", "above"):
        f = filters[name]
        assert f.rows.shape[0] == fe.KP_QUERIES + 1 and f.lo != fe.TABLE_LO
        own = [answer(f, q, q) for q in range(fe.KP_QUERIES)]
        if name == "per_query":
            assert all(fe.TABLE_LO + gt[q] in own[q][0] for q in range(fe.KP_QUERIES))
        assert len({str(a) for a in own}) == fe.KP_QUERIES                     # a different answer for every query
        changed = 0
        for q in range(1, fe.KP_QUERIES):
            assert answer(f, q, q, "row0") == answer(f, 0, q)
            changed += answer(f, 0, q) != own[q] and answer(f, q - 1, q) != own[q]
        assert changed >= (fe.KP_QUERIES - 1 if name == "per_query" else 6), name
    assert filters["above"].lo > fe.TABLE_LO and filters["shared"].rows.shape[0] == 1


# ---- the prior's rule ------------------------------------------------------------------------------------------------
def test_prior_rule_decides_the_edges():
    got = {}
    for name, t, center, radius, want in fe.PRIOR_EDGES:
        c = np.asarray(center, np.float64)[None, :]
        with np.errstate(over="ignore"):
            row = prior_rows(t[None, :], np.ones(1, bool), c, np.array([radius]))
        assert row.shape == (1, 1) and bool(row[0, 0]) is want, name
        with np.errstate(over="ignore"):
            assert not prior_rows(t[None, :], np.zeros(1, bool), c, np.array([radius]))[0, 0], name       # never without a pose
        got[name] = bool(row[0, 0])
    # the literal decisions
    assert got == {
        "r3_exact": True, "r3_ulp_below": False, "r3_ulp_above": True, "r2_exact": True, "r2_ulp_below": False,
        "r2_ulp_above": True, "nan_z_dims2": True, "inf_z_dims2": True, "nan_z_dims3": False, "r0_centre2": True,
        "r0_centre3": True, "r0_ulp_off": False, "inf_coord": False, "neg_inf_coord3": False, "overflow_r_inf": True,
        "overflow_r_1e200": True, "overflow_r_1e100": False, "neg_zero": True, "denormal_r0": False, "denormal_exact": True,
        "denormal_ulp_below": False}
    assert 2.0 * 2.0 + 3.0 * 3.0 + 6.0 * 6.0 == 7.0 * 7.0
    with np.errstate(over="ignore"):
        assert np.isinf(np.float64(3e38 + 1e200) * np.float64(3e38 + 1e200))       # d2 overflows, the coordinate is finite
    assert np.isfinite(np.float32(3e38)) and np.float32(1e-45) > 0 and float(np.float32(1e-45)) ** 2 > 0.0
    for k, e in enumerate(fe.PRIOR_EDGES):
        t, loc = fe.prior_scene(129, e, k)
        assert loc in fe.PRIOR_EDGE_LOCALS and np.array_equal(t[loc], e[1], equal_nan=True)
    assert {fe.PRIOR_EDGE_LOCALS[k % 5] for k in range(len(fe.PRIOR_EDGES))} == set(fe.PRIOR_EDGE_LOCALS)
