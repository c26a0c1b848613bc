"""The workloads of tests/test_gpu_loop_edges.py, checked without a GPU: no frame has k-NN ties; the restated loop
(tests/_loop_edges.py) with the plain bound equals the oracle driven through the reference's loop on every workload and
skip_near; a twin gets the votes the workload claims exactly when skip_near is below its distance; and every mutant of the
bound changes the expected result on the workload named for it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _loop_edges as le  # noqa: E402

S_ALL = le.all_sessions()
CASES = [(n, k) for n, s in S_ALL.items() for k in s.skips]
_MEMO = {}


def _oracle_loop(oracle_mod, name, skip):
    if (name, skip) not in _MEMO:
        _MEMO[(name, skip)] = S_ALL[name].oracle_loop(oracle_mod, skip)
    return _MEMO[(name, skip)]


@pytest.mark.parametrize("name", list(S_ALL))
def test_frames_have_no_knn_ties_and_the_shapes_claimed(name, oracle_mod):
    from sgtd_amd import synth
    s = S_ALL[name]
    k = oracle_mod.DEFAULTS["descriptor_near_num"]
    assert 10 <= s.F <= 24 and 40 <= s.n_kp <= 60
    d = s.descs(oracle_mod)
    for i, (x, l) in enumerate(s.frames()):
        if len(x) > k:
            assert not synth.has_knn_ties(x, k), (name, i)
            assert d[i].n > 100, (name, i)
        else:
            assert i in s.short and d[i].n == 0, (name, i)
        assert np.all(d[i].frame == s.first + i)
    for t, src in s.twins.items():
        assert np.array_equal(s.frames()[t][0], s.frames()[src][0]) and np.array_equal(d[t].side, d[src].side)


@pytest.mark.parametrize("name, skip", CASES)
def test_plain_bound_equals_the_oracle_loop(name, skip, oracle_mod):
    s = S_ALL[name]
    want = _oracle_loop(oracle_mod, name, skip)
    got = s.restated(oracle_mod, skip)
    for q in range(s.F):
        assert le.same_select(got[q], want[q]), (name, skip, q)
    # a twin's source gets the votes claimed exactly when skip_near is below the twins' distance (and the source is kept)
    for t, src in s.twins.items():
        if t < s.M:
            continue
        votes = want[t - s.M]["votes"]
        fid = s.first + src
        if skip < t - src and src not in s.removed:
            n = s.twin_votes(oracle_mod, t)
            assert n >= 100 and votes.get(fid) == n and fid in want[t - s.M]["cand_frame"].tolist(), (name, skip, t)
        else:
            assert fid not in votes, (name, skip, t)


def test_reach(oracle_mod):
    S = S_ALL
    # the bound itself: skip_near d - 1, d, d + 1 for the twins at distance 1 and 8
    assert {0, 1, 2, 7, 8, 9} <= set(S["bound"].skips) and S["bound"].twins == {7: 6, 12: 4}
    # tied twins: equal votes, the lower frame first
    r = _oracle_loop(oracle_mod, "tied", 0)[14]
    assert r["votes"][3] == r["votes"][9] and r["cand_frame"][:2].tolist() == [3, 9]
    r = _oracle_loop(oracle_mod, "tied", 7)[14]
    assert 9 not in r["votes"] and r["cand_frame"][0] == 3
    # the clamp: a bound below zero, below frame_lo, inside a hole; a large first frame
    assert all(len(r["cand_frame"]) == 0 for r in _oracle_loop(oracle_mod, "bound", le.BIG))
    assert all(len(r["cand_frame"]) == 0 for r in _oracle_loop(oracle_mod, "bound", 20))
    s = S["removed_head"]
    lo = s.records(oracle_mod)[1]
    assert lo == 3 and s.c - 7 < lo and all(not r["votes"] for r in _oracle_loop(oracle_mod, "removed_head", 7)[:3])
    assert _oracle_loop(oracle_mod, "removed_head", 0)[0]["cand_frame"].tolist()[:1] == [3]
    s = S["removed_hole"]
    loop = _oracle_loop(oracle_mod, "removed_hole", 4)
    assert s.c + 0 - 4 == 4 and 4 in s.removed and 2 in loop[0]["votes"] and 5 not in loop[1]["votes"]
    assert 5 in _oracle_loop(oracle_mod, "removed_hole", 3)[1]["votes"]
    assert S["first_large"].records(oracle_mod)[1] == 1000000
    # frames without descriptors: frame_lo above c, frame_hi below the last frames
    s = S["short"]
    _, lo, hi = s.records(oracle_mod)
    assert (lo, hi) == (2, 11) and s.c == 0 and s.F == 14 and 3 < 6 < 9
    # both key widths
    assert S["bound_wide"].cfg["std_side_resolution"] == 0.5 and not S["bound"].cfg


@pytest.mark.parametrize("mutant", sorted(le.MUTANTS))
def test_mutants_of_the_bound_are_caught(mutant, oracle_mod):
    name, skip = le.MUTANTS[mutant]
    s = S_ALL[name]
    want = _oracle_loop(oracle_mod, name, skip)
    plain = s.restated(oracle_mod, skip)
    assert all(le.same_select(plain[q], want[q]) for q in range(s.F))
    bad = s.restated(oracle_mod, skip, mutant=mutant, chunk=s.F)
    assert any(not le.same_select(bad[q], want[q]) for q in range(s.F)), mutant
    assert mutant in le.__doc__ and name in le.__doc__
