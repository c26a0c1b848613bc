"""sgtd_consistent_loops at its edges (tests/_consistency_edges.py) in every form of the call, against the rule of
include/sgtd_accel.h: the bit matrix word for word, in_set, degree, pick and n_set exactly, consistency_rounds against the
rounds of the choice under the shortcut rule.  The thresholds are the ones the library hands back.

Forms: frame_a ids; pose_a rows with frame_a NULL; a view holding the poses; a group handle over one device (and over two
where there are two); the same handle straight after a larger run whose matrix is all ones (every buffer holds another
run's words); a fresh handle; timing on.  The small worlds run in all of them, the worlds of N_BIG edges in the first
two, the one-device group and the reused handle.

What is exhaustive and what is sampled: the knife runs, the chains, remaining_degree and the store updates compare the
whole answer with the numpy restatement (every size below 200); the big integer worlds and max_edges compare the whole
matrix and the whole choice with the analytic answer; noisy_big compares sampled rows of the matrix (one of every 64-row
block and the rows at the edges) with the restatement and judges the choice on the device's own matrix."""
import ctypes as C
import time

import numpy as np
import pytest

import _consistency_edges as ce
import _consistency_ref as cr

pytestmark = pytest.mark.gpu

SMALL_FORMS = ["frame_a", "pose_a", "view", "group1", "group2", "reused", "fresh", "timing"]
BIG_FORMS = ["frame_a", "pose_a", "group1", "reused"]


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, manager, synth
    return manager, synth, _lib


@pytest.fixture(scope="module")
def n_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class Forms:
    """the handles of the forms, made when first asked for"""

    def __init__(self, mods):
        self.manager, self.synth, _ = mods
        self.h = {}
        self.order = []

    def _make(self, key):
        m = self.manager
        if key == "view":
            world = self.synth.make_map(8, 120, stream=3)
            owner = self._keep("owner", m.STDescManager())
            owner.add_frames(world.xyz, world.label)
            owner.finalize()
            view = m.STDescManager()
            view.attach_table(owner)
            return view
        if key == "group1":
            return m.STDescManager(devices=[0])
        if key == "group2":
            return m.STDescManager(devices=[0, 1])
        h = m.STDescManager()
        if key == "timing":
            h.set_timing(True)
        return h

    def _keep(self, key, h):
        self.h[key] = h
        self.order.append(key)
        return h

    def handle(self, form, new=False):
        key = form if form in ("view", "group1", "group2", "fresh", "timing") else "plain"
        if key == "group2":
            import torch
            if torch.cuda.device_count() < 2:
                pytest.skip("one device: no two-device group")
        if key == "fresh" and new and key in self.h:
            self.h.pop(key).close()
            self.order.remove(key)
        if key not in self.h:
            self._keep(key, self._make(key))
        return self.h[key]

    def close(self):
        for key in reversed(self.order):          # (the view before its owner)
            self.h[key].close()


@pytest.fixture(scope="module")
def forms(mods):
    f = Forms(mods)
    yield f
    f.close()


def _load(h, ids, poses):
    h.set_frame_poses(None, None)
    h.set_frame_poses(ids, poses)


def _run(forms, form, w, max_trans, max_rot, load=True, new=True):
    """one call in the form -> (handle, results, rows).  load: the world's store is set first (always on a new fresh
    handle); new: a fresh handle is a new one"""
    fresh = form == "fresh" and (new or "fresh" not in forms.h)
    h = forms.handle(form, new)
    if load or fresh:
        _load(h, w["ids"], w["poses"])
    fa, fb, rel = w["frame_a"], w["frame_b"], w["rel_pose"]
    if form == "reused":                          # twice the edges and seven: everything agrees with everything
        big = np.concatenate([np.arange(len(fb)), np.arange(len(fb)), np.arange(min(7, len(fb)))])
        before = h.consistent_loops(fa[big], fb[big], rel[big], 1e6, np.pi)
        assert before["in_set"].size == big.size > len(fb)
    if form == "pose_a":
        got = h.consistent_loops(None, fb, rel, max_trans, max_rot, pose_a=w["poses"][fa])
    else:
        got = h.consistent_loops(fa, fb, rel, max_trans, max_rot)
    rows = h.consistency_rows()
    if form == "timing":
        s = h.stats()
        for k in ("ms_consistency_pairs", "ms_consistency_greedy"):
            assert np.isfinite(s[k]) and s[k] >= 0.0, (k, s[k])
    return h, got, rows


def _same(got, rows, want, want_rows, where):
    """want: (in_set, degree, pick, n_set[, rounds])"""
    assert got["n_set"] == want[3], (where, got["n_set"], want[3])
    assert rows.shape == want_rows.shape and np.array_equal(rows, want_rows), (where, "rows")
    for k, v in zip(("in_set", "degree", "pick"), want):
        assert np.array_equal(got[k], v), (where, k)


_refs = {}


def _ref(name, w, thr, ids=None, poses=None):
    """the restatement's whole answer, computed once per world and thresholds, with the shortcut rule's rounds"""
    key = (name, float(thr[0]), float(thr[1]))
    if key not in _refs:
        ref = cr.consistent(w["ids"] if ids is None else ids, w["poses"] if poses is None else poses, w["frame_a"], w["frame_b"],
                            w["rel_pose"], thr[0], thr[1])
        ref["rounds"] = cr.greedy_fast(ref["adj"], ref["valid"], True)[4]
        _refs[key] = ref
    return _refs[key]


def _same_ref(h, got, rows, ref, where):
    _same(got, rows, (ref["in_set"], ref["degree"], ref["pick"], ref["n_set"]), ref["rows"], where)
    assert h.stats()["consistency_rounds"] == ref["rounds"], (where, h.stats()["consistency_rounds"], ref["rounds"])


# ---- the bitwise rule: pairs on the translation bound ----
@pytest.mark.parametrize("form", SMALL_FORMS)
def test_knife_pairs(forms, form):
    """every knife pair at every placement: the pair sits on the bound (tt == d2), no condition keeps anything clear of
    it, and the whole answer is the restatement's.  The store is set once per handle: the cached copy serves the rest"""
    runs = ce.knife_runs()
    assert len(runs) >= 8 * len(ce.PLACEMENTS)
    first, last_pair = True, None
    for name, w, p, (i, j) in runs:
        new = p is not last_pair
        h, got, rows = _run(forms, form, w, p["max_trans"], ce.KNIFE_ROT, load=first, new=new)
        first, last_pair = False, p
        thr = got["thresholds"]
        assert thr[0] == p["d2"], (name, thr[0], p["d2"])
        ref = _ref(name, w, thr)
        assert ref["gap_d2"][i, j] == 0.0 and ref["adj"][i, j]
        assert (rows[i, j >> 6] >> np.uint64(j & 63)) & np.uint64(1) and (rows[j, i >> 6] >> np.uint64(i & 63)) & np.uint64(1), name
        _same_ref(h, got, rows, ref, (form, name))


# ---- the host's round groups ----
@pytest.mark.parametrize("form", SMALL_FORMS)
def test_chains_end_on_and_past_a_group_of_rounds(forms, form):
    for low in (False, True):
        for n in ce.SMALL_CHAINS:
            w = ce.chain(n, low)
            h, got, rows = _run(forms, form, w, w["max_trans"], w["max_rot"])
            assert got["thresholds"][0] == 25.0
            ref = _ref(w["name"], w, got["thresholds"])
            _same_ref(h, got, rows, ref, (form, w["name"]))
            want = ce.chain_expect(n, low)
            _same(got, rows, want, cr.pack_rows(ce.shift_adjacency(w)), (form, w["name"], "analytic"))
            assert ref["rounds"] == want[4] == n - 1


@pytest.mark.parametrize("form", SMALL_FORMS)
def test_remaining_degree(forms, form):
    w = ce.remaining_degree()
    h, got, rows = _run(forms, form, w, w["max_trans"], w["max_rot"])
    ref = _ref(w["name"], w, got["thresholds"])
    _same_ref(h, got, rows, ref, form)
    assert got["degree"][:2].tolist() == [16, 15] and np.flatnonzero(got["in_set"]).tolist() == [0] + list(range(2, 8)) + list(range(16, 21))


# ---- the cached pose store ----
@pytest.mark.parametrize("form", SMALL_FORMS)
def test_store_updates(forms, form):
    """a pose replaced, a pose forgotten, a pose added beyond the stored range (the device copy grows), each by a
    set_frame_poses call for that id alone and followed by a run that must be the rule's on the store as it stands"""
    w = ce.store_world()
    steps = ce.store_steps()
    for k in range(len(steps) + 1):
        if k:
            forms.handle(form).set_frame_poses(steps[k - 1][1], steps[k - 1][2])
        h, got, rows = _run(forms, form, w, w["max_trans"], w["max_rot"], load=k == 0, new=k == 0)
        ids, poses = ce.store_after(k)
        ref = _ref("store_%d" % k, w, got["thresholds"], ids, poses)
        assert cr.clear_of_thresholds(ref, *got["thresholds"]), (k, ref["min_gap_d2"], ref["min_gap_tr"])
        _same_ref(h, got, rows, ref, (form, k, steps[k - 1][0] if k else "loaded"))
    assert got["degree"][20] >= 0 and got["degree"][70] == -1


# ---- past 4096 edges: integer worlds, the whole matrix and the whole choice ----
_analytic = {}


def _analytic_ref(name, n_cus):
    if name not in _analytic:
        w = ce.BIG_ANALYTIC[name](n_cus=n_cus)
        adj = ce.shift_adjacency(w)
        _analytic[name] = (w, cr.pack_rows(adj), cr.greedy_fast(adj, np.ones(adj.shape[0], bool), True))
    return _analytic[name]


@pytest.mark.parametrize("form", BIG_FORMS)
@pytest.mark.parametrize("name", sorted(ce.BIG_ANALYTIC))
def test_big_integer_worlds(forms, n_cus, name, form):
    w, want_rows, want = _analytic_ref(name, n_cus)
    n = ce.n_big(n_cus)
    assert len(w["frame_b"]) == n > ce.n_waves(n, n_cus) and want_rows.shape[1] > 64
    h, got, rows = _run(forms, form, w, w["max_trans"], w["max_rot"])
    assert got["thresholds"][0] == w["max_trans"] ** 2
    _same(got, rows, want, want_rows, (form, name))
    assert h.stats()["consistency_rounds"] == want[4], (form, name, h.stats()["consistency_rounds"], want[4])
    if name.startswith("chain_big"):
        assert want[4] == n - 1
    if name in ("tie_far", "tie_split"):
        u1, u2 = w["tie"]
        assert got["pick"][u1] == 0 and got["pick"][u2] == -1 and got["degree"][u1] == got["degree"][u2] == got["degree"].max()


# ---- past 4096 edges: a noisy world, sampled rows ----
_noisy = {}


@pytest.mark.parametrize("form", BIG_FORMS)
def test_noisy_big(forms, n_cus, form):
    """NOT a full n^2 comparison: the matrix is judged by sampled rows against the restatement (and by its structure as a
    whole), the choice by the restatement's greedy on the device's own matrix"""
    w = ce.noisy_big(n_cus)
    n = ce.n_big(n_cus)
    h, got, rows = _run(forms, form, w, w["max_trans"], w["max_rot"])
    thr = got["thresholds"]
    key = (float(thr[0]), float(thr[1]))
    if key not in _noisy:
        P, A, valid = cr.edges(w["ids"], w["poses"], w["frame_a"], w["frame_b"], w["rel_pose"])
        sample = ce.sample_rows(n, ce.n_waves(n, n_cus))
        _noisy[key] = (valid, sample) + cr.adjacency_rows(P, A, valid, thr[0], thr[1], sample)
    valid, sample, adj_rows, gap_d2, gap_tr = _noisy[key]
    bad = np.flatnonzero(~valid)
    assert np.array_equal(bad, np.array(sorted(w["invalid"])))
    assert gap_d2.min() > 1e-9 * max(1.0, abs(thr[0])) and gap_tr.min() > 1e-9 * max(1.0, abs(thr[1]))
    assert rows.shape == (n, (n + 63) // 64)
    padded = np.zeros((sample.size, rows.shape[1] * 64), bool)
    padded[:, :n] = adj_rows
    want = np.packbits(padded, axis=1, bitorder="little").view("<u8").astype(np.uint64)
    differ = np.flatnonzero((rows[sample] != want).any(1))
    assert differ.size == 0, (form, sample[differ][:8])
    # the whole matrix: symmetric, zero diagonal, zero padding bits, empty rows and columns for the invalid edges
    adj = cr.unpack_rows(rows, n)
    assert np.array_equal(adj, adj.T) and not adj.diagonal().any()
    assert not (rows[:, -1] >> np.uint64(n % 64)).any()
    assert not adj[bad].any() and not adj[:, bad].any()
    # the choice, on the matrix the device made
    in_set, degree, pick, n_set, rounds = cr.greedy_fast(adj, valid, True)
    _same(got, rows, (in_set, degree, pick, n_set), rows, form)
    assert h.stats()["consistency_rounds"] == rounds and rounds > 256 and 100 < n_set < n
    assert (got["degree"][bad] == -1).all() and (got["pick"][bad] == -1).all()
    members = np.flatnonzero(got["in_set"])
    assert adj[np.ix_(members, members)].sum() == members.size * (members.size - 1)          # a clique


# ---- the limit ----
def test_max_edges(forms, mods):
    """SGTD_MAX_LOOP_EDGES edges: 512 row words, one per thread of the select pass, a matrix of 128 MB.  The whole matrix
    against the group masks, 64 rows against the restatement, the choice against the restatement's greedy on the analytic
    adjacency; then the refusal one edge further, which leaves no result, and a small run after it"""
    t0 = time.time()
    w = ce.max_edges()
    n = ce.MAX_EDGES
    h, got, rows = _run(forms, "frame_a", w, w["max_trans"], w["max_rot"])
    t_dev = time.time() - t0
    assert got["thresholds"][0] == 1.0 and rows.shape == (n, 512)
    assert np.array_equal(rows, ce.group_rows(w["group"]))
    sample = ce.spread_rows(n, 64)
    P, A, valid = cr.edges(w["ids"], w["poses"], w["frame_a"], w["frame_b"], w["rel_pose"])
    adj_rows = cr.adjacency_rows(P, A, valid, got["thresholds"][0], got["thresholds"][1], sample)[0]
    assert valid.all() and np.array_equal(cr.unpack_rows(rows[sample], n), adj_rows)
    g8 = w["group"].astype(np.int8)
    adj = g8[:, None] == g8[None, :]
    np.fill_diagonal(adj, False)
    want = cr.greedy_fast(adj, valid, True)
    del adj
    assert all(np.array_equal(a, b) for a, b in zip(want[:3], ce.group_greedy(w["group"])[:3])) and want[3:] == (n // 2, 2)
    _same(got, rows, want, rows, "max_edges")
    assert h.stats()["consistency_rounds"] == 2 and got["pick"][1] == 0 and got["pick"][n - 3] == n // 2 - 1
    print("max_edges: %.1f s for the call and the matrix, %.1f s in all" % (t_dev, time.time() - t0))
    # one edge more: refused, and the results are gone
    _, _, lib = mods
    big = n + 1
    with pytest.raises(lib.SgtdError) as ei:
        h.consistent_loops(np.zeros(big, np.uint32), np.zeros(big, np.uint32), np.zeros((big, 12)), 1.0, 0.1)
    assert ei.value.status == -6 and "32768" in str(ei.value)
    thr = np.zeros(2)
    assert h._L.sgtd_result_consistent(h._h, None, None, None, thr.ctypes.data_as(C.c_void_p)) == -7
    with pytest.raises(lib.SgtdError):
        h.consistency_rows()
    # a run of 5 edges on the same handle
    s = np.zeros((5, 3))
    s[3, 0] = 40.0
    w5 = ce.shift_world(s)
    h, got, rows = _run(forms, "frame_a", w5, 5.0, 0.1)
    assert rows[:, 0].tolist() == [0b10110, 0b10101, 0b10011, 0, 0b00111]
    assert got["n_set"] == 4 and got["pick"].tolist() == [0, 1, 2, -1, 3] and got["degree"].tolist() == [3, 3, 3, 0, 3]
    _same_ref(h, got, rows, _ref("five", w5, got["thresholds"]), "five")
