"""The workloads of tests/test_gpu_remove_edges.py, checked without a GPU: the numpy model of sgtd_remove_frames' two passes
(tests/_remove_edges.py) equals field[keep] on every workload; every workload reaches the count it exists for; and every
switch of the model (a plausible mistake in the compaction) changes the result on the workload named for it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _remove_edges as re_  # noqa: E402

W_ALL = re_.workloads()
NAMES = list(W_ALL)
# the workloads the whole model runs on with all seven fields; the rest with the three widths' narrowest fields
FULL = ("counts/E5/every_other_entry", "counts/E1025/all_but_first", "align/k1_m5", "bitmap/span33/hi", "rank/single_gone")


def _gone(w):
    return [x for s in w.steps for x in s]


def _model(w, mutant=None, names=None):
    names = names or (re_.NAMES7 if w.name in FULL else ("vertex", "center", "label", "frame"))
    return re_.model_remove(w.fields(), _gone(w), mutant=mutant, names=names)


def _differs(w, out, state=None, got_state=None):
    keep = w.keep()
    for f, v in out.items():
        want = re_.words(w.fields()[f])[keep]
        if v.shape != want.shape or not np.array_equal(v, want):
            return True
    return state is not None and state != got_state


def _true_state(w):
    keep = w.keep()
    fr = w.frame[keep].astype(np.int64)
    gone = len(set(w.frame[~keep].tolist()))
    return (int(keep.sum()), int(fr.min()) if len(fr) else None, int(fr.max()) if len(fr) else None, gone)


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_field_of_keep(name):
    w = W_ALL[name]
    if w.E == 0 or not w.keep().any() and w.E > 4096:
        pytest.fail("a workload without entries")
    out, state = _model(w)
    assert not _differs(w, out), name
    assert state == _true_state(w), name


def test_model_equals_field_of_keep_on_the_large_workload():
    w = re_.large()
    keep = w.keep()
    for f in ("vertex", "frame"):
        src = re_.words(w.fields()[f])
        np.testing.assert_array_equal(re_.model_fast(src, keep), src[keep])
    # the vectorised model is the plain one: both on a small workload
    s = W_ALL["counts/E2049/every_other_wave"]
    src = re_.words(s.fields()["vertex"])
    np.testing.assert_array_equal(re_.model_fast(src, s.keep()), _model(s, names=("vertex",))[0]["vertex"])


# ---- the fields --------------------------------------------------------------------------------------------------------
def test_every_word_names_its_entry_field_and_place():
    f = re_.make_fields(np.arange(5000), np.zeros(5000, np.uint32))
    pool = np.concatenate([re_.words(f[k]).reshape(-1) for k in ("angle", "center", "vertex", "node_id")])
    assert len(np.unique(pool)) == pool.size
    assert len(np.unique(f["side"], axis=0)) == 5000
    assert f["label"].min() >= 0 and f["label"].max() <= 15 and len(np.unique(f["label"], axis=0)) > 2000
    for k in ("angle", "center", "vertex"):
        v = f[k]
        assert np.isnan(v).sum() >= 900 and np.isnan(v).any(axis=1).sum() >= 900, k
        tiny = np.finfo(v.dtype).tiny
        assert ((np.abs(v) < tiny) & np.signbit(v)).sum() >= 900, k
        assert np.isfinite(v).all(axis=1).sum() >= 2900, k
    # two different indices never share a field row
    g = re_.make_fields(np.arange(re_.LARGE_E - 3000, re_.LARGE_E), np.zeros(3000, np.uint32))
    for k in ("angle", "center", "vertex", "node_id", "side"):
        both = np.concatenate([re_.words(f[k]), re_.words(g[k])])
        assert len(np.unique(both, axis=0)) == len(both), k


# ---- reach -------------------------------------------------------------------------------------------------------------
def test_counts_reach():
    tiles = {1: 1, 5: 1, 1023: 1, 1024: 1, 1025: 2, 2047: 2, 2048: 2, 2049: 3}
    for E in re_.COUNT_E:
        for p in re_.COUNT_PATTERNS:
            w = W_ALL["counts/E%d/%s" % (E, p)]
            assert w.E == E and w.n_tiles() == tiles.get(E, 1)
            assert re_.WIDTH["frame"] * E < 4 or E >= 4            # E < 4: the narrowest field is less than one 16-byte vector
    k = W_ALL["counts/E2049/every_other_round"].keep().reshape(-1)[:2048].reshape(2, 4, 256)
    assert not k[:, 0].any() and k[:, 1].all() and not k[:, 2].any() and k[:, 3].all()
    k = W_ALL["counts/E1024/every_other_wave"].keep().reshape(16, 64)
    assert all(k[m].all() == (m % 2 == 1) and k[m].any() == (m % 2 == 1) for m in range(16))
    assert int(W_ALL["counts/E1/all_but_first"].keep().sum()) == 0          # a removal that empties the table
    assert int(W_ALL["counts/E2049/only_last"].keep().sum()) == 1


def test_rank_reach():
    for kind in ("gone", "kept"):
        w = W_ALL["rank/single_" + kind]
        k = w.keep().reshape(-1, 16, 64)
        odd = (k.sum(axis=2) != (64 if kind == "gone" else 0))
        assert w.n_tiles() == 12 and odd.sum() == 12
        got = sorted((int(np.flatnonzero(odd[t])[0]), int(np.flatnonzero(k[t, odd[t]][0] != (kind == "gone"))[0])) for t in range(12))
        assert got == sorted((r * 4 + wv, lane) for r, wv in re_.RANK_WAVES for lane in re_.RANK_LANES)
    seen = {n: set() for n in range(3)}
    for side in ("below", "above"):
        for c in range(re_.SPLIT_CHUNKS):
            w = W_ALL["rank/split_%s_%d" % (side, c)]
            k = w.keep().reshape(-1, 16, 64)
            assert w.n_tiles() == 13
            for t in range(13):
                for n, (r, wv) in enumerate(re_.RANK_WAVES):
                    s, below = re_.split_of(w.name, t, n)
                    lanes = np.arange(64)
                    np.testing.assert_array_equal(k[t, r * 4 + wv], lanes < s if below else lanes >= s)
                    seen[n].add((s, below))
    for n in range(3):                                  # every split 0 .. 64 of every one of the three waves, kept below and kept above
        assert seen[n] == {(s, b) for s in range(65) for b in (True, False)}, n


def test_tiles_reach():
    per = (lambda w: np.bincount(np.arange(w.E) // re_.TILE, weights=w.keep()).astype(int).tolist())
    assert per(W_ALL["tiles/middle_empty"]) == [1024, 0, 1024]
    assert per(W_ALL["tiles/first_empty"]) == [0, 1024, 1024]
    assert per(W_ALL["tiles/one_between"]) == [1024, 1, 1024]
    assert per(W_ALL["tiles/last_partial_empty"]) == [1024, 1024, 0] and W_ALL["tiles/last_partial_empty"].E % re_.TILE == 300


def test_align_reach():
    """the second tile's output offset times W takes every residue mod 4 that W can reach, and the head, the vectors and the
    tail of its output are each empty in one workload and not in another"""
    for W in (9, 6, 3, 1):
        reachable = {(k * W) % 4 for k in range(64)}
        residues, heads, vecs, tails = set(), set(), set(), set()
        for k in re_.ALIGN_K:
            for m in re_.ALIGN_M:
                w = W_ALL["align/k%d_m%d" % (k, m)]
                per = np.bincount(np.arange(w.E) // re_.TILE, weights=w.keep()).astype(int).tolist()
                assert per == [k, m]
                h, v, t = re_.output_split(k, m, W)
                assert h + 4 * v + t == m * W
                residues.add((k * W) % 4)
                heads.add(h > 0), vecs.add(v > 0), tails.add(t > 0)
        assert residues == reachable, W
        assert heads == tails == {True, False}, W
        # (W = 9 and 6: one entry is already more words than a head of at most 3 and a tail of at most 3 leave without a vector)
        assert vecs == ({True, False} if W <= 3 else {True}), W
    assert {(k * 9) % 4 for k in range(4)} == {0, 1, 2, 3} and {(k * 6) % 4 for k in range(4)} == {0, 2}


def test_bitmap_reach():
    for S in re_.SPANS:
        w = W_ALL["bitmap/span%d/lo" % S]
        assert int(w.frame.max()) - int(w.frame.min()) + 1 == S and (S + 31) // 32 == {1: 1, 31: 1, 32: 1, 33: 2, 64: 2, 65: 3}[S]
        assert w.per_frame
    w = W_ALL["bitmap/span65/hole"]
    st = _true_state(w)
    assert (st[1], st[2]) == (40, 104) and st[3] == 1
    assert _true_state(W_ALL["bitmap/span65/both"])[1:3] == (41, 103)
    for tag, in_lds in (("lds_last", True), ("global_first", False)):
        for end in ("lo", "hi"):
            w = W_ALL["bitmap/%s/%s" % (tag, end)]
            span = int(w.frame.max()) - int(w.frame.min()) + 1
            assert ((span + 31) // 32 * 4 <= re_.LDS_SWITCH_BYTES) == in_lds
            assert span == re_.LDS_SWITCH_FRAMES + (0 if in_lds else 1)
    w = W_ALL["bitmap/first_large"]
    assert w.cfg["first_frame_id"] == int(w.frame.min()) and not w.keep(2).__invert__().any()      # the first two calls remove nothing
    assert (~w.keep(3)).sum() > 0 and _true_state(w)[1:3] == (70018, 70049)
    w = W_ALL["bitmap/wave_runs"]
    starts = np.flatnonzero(np.diff(np.concatenate([[-1], w.frame.astype(np.int64)])))
    assert np.all(starts % re_.WAVE == 0)


def test_order_tail_and_stamped_reach():
    assert np.all(np.diff(W_ALL["order/descending"].frame.astype(np.int64)) <= 0)
    w = W_ALL["order/aba_remove_a"]
    runs = w.frame[np.concatenate([[0], np.flatnonzero(np.diff(w.frame.astype(np.int64))) + 1])].tolist()
    assert runs == [900, 41, 40, 3, 40, 17] and any(len(set(w.frame[a:b].tolist())) == 2 for a, b in w.bounds)
    assert not W_ALL["order/aba_remove_a"].per_frame
    cut_entry = sum(re_.TAIL_SIZES[:5])
    for k, (main, tail) in dict(main_only=(True, False), tail_only=(False, True), both=(True, True)).items():
        w = W_ALL["tail/" + k]
        gone = ~w.keep()
        assert (gone[:cut_entry].any(), gone[cut_entry:].any()) == (main, tail) and "tail" in w.forms and "multi" in w.forms
    sh = (lambda f: (f // re_.SHARD_BLOCK) % 3)
    w = W_ALL["stamped/shard1_all"]
    assert w.stamped and set(sh(w.frame[~w.keep()].astype(np.int64)).tolist()) == {1} and not (sh(w.frame[w.keep()].astype(np.int64)) == 1).any()
    assert sh(63) != sh(64) and sh(127) != sh(128) and "multi" in W_ALL["stamped/f63_64"].forms
    assert all((w.stamped and not w.cfg.get("first_frame_id")) == ("multi" in w.forms) for w in W_ALL.values())


def test_large_reach():
    w = re_.large()
    assert w.n_tiles() == 2049 > re_.SCAN_BLOCK > re_.FLAG_GRID and w.E % re_.TILE == 1
    per = np.bincount(np.arange(w.E) // re_.TILE, weights=w.keep()).astype(int)
    assert (per == 0).sum() >= 290 and len(set(per.tolist())) > 50 and per[re_.FLAG_GRID:].any()
    assert 280e6 < w.E * 4 * sum(re_.WIDTH.values()) < 300e6


# ---- the switches ------------------------------------------------------------------------------------------------------
CAUGHT_BY = dict(low_half_only="rank/single_gone", before_shifted="counts/E1025/all_but_first", wave_major="counts/E1024/every_other_round",
                 ne_1024="counts/E1025/all_but_first", head_from_entry="align/k1_m5", tail_dropped="align/k0_m5",
                 span_short="bitmap/span33/hi", present_lane0="bitmap/wave_runs")


@pytest.mark.parametrize("mutant", sorted(CAUGHT_BY))
def test_switches_are_caught(mutant):
    w = W_ALL[CAUGHT_BY[mutant]]
    out, state = _model(w, names=re_.NAMES7)
    assert not _differs(w, out, _true_state(w), state)
    out, state = _model(w, mutant=mutant, names=re_.NAMES7)
    assert _differs(w, out, _true_state(w), state), mutant
    if mutant == "head_from_entry":                     # per width: 9 and 1 are 1 mod 4, so there the entry offset gives the same head
        for f, v in out.items():
            assert (not np.array_equal(v, re_.words(w.fields()[f])[w.keep()])) == (re_.WIDTH[f] in (6, 3)), f
    if mutant == "present_lane0":                       # the entries are right: only the surviving span is not
        assert not _differs(w, out) and state[1:3] != _true_state(w)[1:3]


def test_low_half_only_is_caught_by_every_split_workload():
    for side in ("below", "above"):
        w = W_ALL["rank/split_%s_2" % side]
        assert _differs(w, _model(w, mutant="low_half_only", names=("frame", "label"))[0])


def test_count_not_reset_needs_more_tiles_than_workgroups():
    w = re_.large()
    src = re_.words(w.fields()["label"])
    got = re_.model_fast(src, w.keep(), mutant="count_not_reset")
    want = src[w.keep()]
    assert got.shape != want.shape or not np.array_equal(got, want)
    s = W_ALL["counts/E2049/every_other_entry"]          # three tiles, three workgroups: nothing to carry over
    assert not _differs(s, _model(s, mutant="count_not_reset", names=("label",))[0])


def test_every_switch_is_listed():
    assert set(CAUGHT_BY) | {"count_not_reset"} == set(re_.MUTANTS)
    for m, n in CAUGHT_BY.items():
        assert n in re_.__doc__ and m in re_.__doc__
