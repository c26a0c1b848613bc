"""sgtd_pose_consensus at its edges (tests/_consensus_edges.py) in every form of the call, against the rule of
include/sgtd_accel.h: the rows word for word, the integers as they are, the doubles bit for bit, with the thresholds the
library hands back.  tests/test_consensus_edges.py shows on the CPU that these inputs tell every mutant of the rule apart.

Rows-form forms: a fresh handle; a handle that first ran 257 queries of 64 candidates (every buffer holds another run's
words); a view holding its own poses while its owner holds others; a group handle over three shards of one device with the
poses set on the group; a handle with a pending verified batch and batch-form results, which the rows form replaces.
The batch form runs on handles of candidate_num 1, 2 and 64: against the restatement fed from the getters and against the
rows form fed from the same arrays, for the verify, refined and aligned poses, after sgtd_verify_masked, and with a partly
stored pose map."""
import numpy as np
import pytest

import _consensus_edges as ce
import _consensus_ref as ref

pytestmark = pytest.mark.gpu

FORMS = ["fresh", "reused", "view", "group", "behind_batch"]
F, NQ = 60, 8
BATCH_TRANS, BATCH_ROT = 2.0, np.deg2rad(10.0)


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, evaluate, manager, synth
    return manager, synth, _lib, evaluate


@pytest.fixture(scope="module")
def world(mods):
    _, synth, _, ev = mods
    m = synth.make_map(F, 200, stream=511, spacing=6.0)
    qs = synth.make_queries(m, 2 * NQ, stream=512)
    rows = np.stack([ev.pose_row(*p) for p in m.pose])
    return m, qs, rows


def _new(manager, m, rows, **kw):
    h = manager.STDescManager(**kw)
    h.add_frames(m.xyz, m.label, keep_keypoints=True)
    h.finalize()
    h.set_frame_poses(np.arange(len(rows)), rows)
    return h


def _load(h, b):
    h.set_frame_poses(None, None)
    h.set_frame_poses(b["ids"], b["poses"])


def _rows(h, b, max_trans, max_rot):
    return h.pose_consensus_rows(b["n_cand"], b["cand_frame"], b["score"], b["rel_pose"], max_trans, max_rot)


def _same(h, got, want, where=None):
    """every output of the call against the restatement's"""
    for k in ce.INT_KEYS:
        assert np.array_equal(got[k], want[k]), (where, k, got[k], want[k])
    for k in ce.DBL_KEYS:
        assert np.array_equal(ce.bits(got[k]), ce.bits(want[k])), (where, k)
    for q in range(want["n_set"].size):
        rows, degree, pick = h.consensus_rows(q)
        assert np.array_equal(rows, want["rows"][q]), (where, q, "rows")
        assert np.array_equal(degree, want["degree"][q]) and np.array_equal(pick, want["pick"][q]), (where, q)


def _ranges(h, got, where):
    """result_consensus(first, n) at the last query, over all of them and past the end"""
    nq = got["n_set"].size
    for first, n in ((nq - 1, 1), (0, nq), (nq, 0)):
        part = h.result_consensus(first, n)
        for k in ce.INT_KEYS:
            assert np.array_equal(part[k], got[k][first:first + n]), (where, first, n, k)
        for k in ce.DBL_KEYS:
            assert np.array_equal(ce.bits(part[k]), ce.bits(got[k][first:first + n])), (where, first, n, k)
        assert np.array_equal(ce.bits(part["thresholds"]), ce.bits(got["thresholds"]))


_refs = {}


def _ref(name, b, thr):
    """the restatement's answer, computed once per batch and thresholds and left unchanged"""
    key = (name, float(thr[0]), float(thr[1]))
    if key not in _refs:
        _refs[key] = ce.reference(b, thr[0], thr[1])
    return _refs[key]


def _status(_lib, call, *a, **kw):
    with pytest.raises(_lib.SgtdError) as ei:
        call(*a, **kw)
    return ei.value.status


class Forms:
    """the handles of the rows-form forms, made when first asked for and kept for the module"""

    def __init__(self, mods, world):
        self.mods, self.world = mods, world
        self.h = {}
        self.order = []
        self.verify_bits = None

    def _keep(self, key, h):
        self.h[key] = h
        self.order.append(key)
        return h

    def _make(self, key):
        manager, synth = self.mods[0], self.mods[1]
        m, qs, rows = self.world
        if key == "reused":
            h = manager.STDescManager()
            big = ref.planted_batch(257, 64, seed=7000 + 6400 + 257)
            _load(h, big)
            got = _rows(h, big, 0.5, np.deg2rad(5.0))
            assert got["n_set"].size == 257 and (got["n_set"] >= 5).sum() > 50
            return h
        if key == "view":
            small = synth.make_map(8, 120, stream=3)
            owner = self._keep("owner", manager.STDescManager())
            owner.add_frames(small.xyz, small.label)
            owner.finalize()
            owner.set_frame_poses(np.arange(F), rows)            # the owner's poses are not the view's
            view = manager.STDescManager()
            view.attach_table(owner)
            return view
        if key == "group":
            return manager.STDescManager(devices=[0, 0, 0])
        if key == "behind_batch":
            h = _new(manager, m, rows)
            h.query_frames(qs.xyz[:NQ], qs.label[:NQ])
            h.verify()
            self.verify_bits = self._verify_bits(h)
            return h
        return manager.STDescManager()

    @staticmethod
    def _verify_bits(h):
        return [[ce.bits(x).tolist() for x in h.result_verify(q)] for q in range(NQ)]

    def handle(self, form):
        if form not in self.h:
            self._keep(form, self._make(form))
        return self.h[form]

    def run(self, form, b, max_trans, max_rot):
        """one rows-form call in the form -> (handle, results)"""
        h = self.handle(form)
        _lib = self.mods[2]
        if form == "behind_batch":
            # batch-form results stand behind the pending batch (with whatever poses the last case left) ...
            before = h.pose_consensus(BATCH_TRANS, BATCH_ROT)
            assert before["n_set"].size == NQ and h.search_loop_consensus(1)[3].size == NQ
        _load(h, b)
        got = _rows(h, b, max_trans, max_rot)
        if form == "behind_batch":
            # ... the rows form's replace them: no batch stands behind those, and the batch's own results are untouched
            assert h.result_consensus()["n_set"].size == b["n_cand"].size
            assert _status(_lib, h.search_loop_consensus, 1) == -7
            assert self._verify_bits(h) == self.verify_bits
        return h, got

    def close(self):
        for key in reversed(self.order):          # (the view before its owner)
            self.h[key].close()


@pytest.fixture(scope="module")
def forms(mods, world):
    f = Forms(mods, world)
    yield f
    f.close()


def _case(forms, form, name):
    c = ce.cases()[name]
    b = c["batch"]
    h, got = forms.run(form, b, c["max_trans"], c["max_rot"])
    thr = got["thresholds"]
    assert thr[0] == c["max_trans"] * c["max_trans"], (name, thr)
    want = _ref(name, b, thr)
    if c["noisy"]:
        assert ref.clear_of_thresholds(want, thr[0], thr[1]), (name, want["min_gap_d2"], want["min_gap_tr"])
    _same(h, got, want, (form, name))
    _ranges(h, got, (form, name))
    return h, got, want


# ---- the bitwise rule: pairs on the translation bound ----
@pytest.mark.parametrize("form", FORMS)
def test_knife_pairs(forms, form):
    """every knife pair at every lane placement, as the only query of its call and as the last of five: the pair sits ON
    the bound (tt == d2), the lower index decides it for both rows, and the whole answer is the restatement's"""
    runs = ce.knife_runs()
    assert len(runs) >= 8 * len(ce.PLACEMENTS) * 2
    for name, b, p, (i, j), q in runs:
        h, got = forms.run(form, b, p["max_trans"], ce.KNIFE_ROT)
        thr = got["thresholds"]
        assert thr[0] == p["d2"], (name, thr[0], p["d2"])
        want = _ref(name, b, thr)
        assert want["adj"][q, i, j] and want["adj"][q, j, i]
        rows = h.consensus_rows(q)[0]
        assert (int(rows[i]) >> j) & 1 and (int(rows[j]) >> i) & 1, (form, name)
        _same(h, got, want, (form, name))
    _ranges(h, got, (form, name))


# ---- the constructed cases ----
@pytest.mark.parametrize("group", sorted(ce.CASE_GROUPS))
@pytest.mark.parametrize("form", FORMS)
def test_cases(forms, form, group):
    for name in ce.CASE_GROUPS[group]:
        h, got, want = _case(forms, form, name)
        if name == "quarter_turn":
            # 1 + 2 cos(pi / 2) is the double above 1.0: the quarter turn (tr == 1 exactly) falls short of it
            assert got["thresholds"][1] == 1.0 + 2.0 * np.cos(np.pi / 2) == np.nextafter(1.0, 2.0) and got["n_set"][0] == 1
        if name == "half_turns":
            assert got["thresholds"][1] == -1.0 and got["n_set"].tolist() == [4] * 4
        if name == "zero_rot":
            assert got["thresholds"].tolist() == [4.0, 3.0] and got["n_set"][0] == 3
        if name in ("validity", "validity_rev"):
            assert got["n_valid"].tolist() == [23, 23] and got["n_set"].tolist() == [22, 23] and got["support_score"][1] == np.inf
        if name == "ncand":
            assert got["n_valid"].tolist() == [64, 0, 64]
        if name == "descending":
            assert got["seed"][0] == 63 and h.consensus_rows(0)[2][[10, 20, 30, 40, 63]].tolist() == [4, 3, 2, 1, 0]
        if name == "full_wave":
            assert got["n_set"].tolist() == [64, 63, 63] and int(got["mask"][0]) == 2 ** 64 - 1
        if name in ("chain_high", "chain_low"):
            assert got["n_set"][0] == 63 and h.consensus_rows(0)[2].max() == 62


# ---- every output word is stored by every call ----
@pytest.mark.parametrize("form", FORMS)
def test_stale_outputs(forms, form):
    """a batch whose every output word is non-default, then, on the same handle and at the same offsets, queries with no
    candidate, none valid and one candidate"""
    h, first, want = _case(forms, form, "stale_first")
    assert (first["n_set"] == 64).all() and (first["mask"] == np.uint64(2 ** 64 - 1)).all() and np.isfinite(first["pose"]).all()
    h2, got, want = _case(forms, form, "stale_second")
    assert h2 is h
    assert got["n_set"].tolist()[:3] == [0, 0, 1] and got["seed"].tolist()[:3] == [-1, -1, 0] and np.isnan(got["pose"][:2]).all()
    assert got["support_score"][:2].tolist() == [0.0, 0.0] and (got["mask"][:2] == 0).all()
    for q in (0, 1):
        rows, degree, pick = h.consensus_rows(q)
        assert not rows.any() and (degree == -1).all() and (pick == -1).all()


# ---- the batch form ----
def _stage_arrays(h, nq, which):
    """score (nq, cn) and rel_pose (nq, cn, 12) as the stage's getter gives them"""
    score, rel = [], []
    for q in range(nq):
        s, rot, t = h.result_verify(q)
        if which != "verify":
            r = h.result_refined(q) if which == "refined" else h.result_aligned(q)
            rot, t = r["rot"], r["t"]
        score.append(s)
        rel.append(np.concatenate([rot.reshape(-1, 9), t.reshape(-1, 3)], axis=1))
    return np.stack(score), np.stack(rel)


def _batch_check(h, res, ids, poses, which, where):
    """the batch form against the restatement fed from the getters and against the rows form fed from the same arrays"""
    got = h.pose_consensus(BATCH_TRANS, BATCH_ROT, refined=which == "refined", aligned=which == "aligned")
    per_q = [h.consensus_rows(q) for q in range(NQ)]
    score, rel = _stage_arrays(h, NQ, which)
    b = {"ids": np.asarray(ids, np.uint32), "poses": poses, "n_cand": res.n_cand, "cand_frame": res.cand_frame, "score": score, "rel_pose": rel}
    want = ce.reference(b, *got["thresholds"])
    assert ref.clear_of_thresholds(want, *got["thresholds"]), (where, want["min_gap_d2"], want["min_gap_tr"])
    _same(h, got, want, where)
    again = _rows(h, b, BATCH_TRANS, BATCH_ROT)
    for k in ce.INT_KEYS:
        assert np.array_equal(got[k], again[k]), (where, k)
    for k in ce.DBL_KEYS:
        assert np.array_equal(ce.bits(got[k]), ce.bits(again[k])), (where, k)
    for q in range(NQ):
        for x, y in zip(per_q[q], h.consensus_rows(q)):
            assert np.array_equal(x, y), (where, q)
    return got, per_q, score


@pytest.mark.parametrize("cn", [1, 2, 64])
def test_batch_form(mods, world, cn):
    """candidate_num 1, 2 and 64 (the default is 50).  With one candidate a query no set can have two members: there the
    case asserts that sets of one exist"""
    import torch
    manager = mods[0]
    m, qs, rows = world
    h = _new(manager, m, rows, candidate_num=cn)
    ids = np.arange(F)
    res = h.query_frames(qs.xyz[:NQ], qs.label[:NQ])
    assert res.cand_frame.shape == (NQ, cn)
    h.verify()
    h.refine_poses(1)
    h.align_keypoints(1.0, iterations=5)
    plain = None
    for which in ("verify", "refined", "aligned"):
        got, per_q, score = _batch_check(h, res, ids, rows, which, (cn, which))
        assert (got["n_set"] >= min(cn, 2)).any() and got["n_valid"].max() >= min(cn, 3), (cn, which, got["n_set"])
        if which == "verify":
            plain = (got, per_q)
    # sgtd_verify_masked: some candidates of some queries dropped, every candidate of one
    degree0 = np.stack([p[1] for p in plain[1]])
    q_all = int(np.argmax(plain[0]["n_valid"]))
    keep = np.full(NQ, 2 ** 64 - 1, np.uint64)
    keep[q_all] = 0
    dropped = []
    for q in range(NQ):
        v = np.flatnonzero(degree0[q] >= 0)
        if q != q_all and q % 2 == 0 and v.size:
            k = int(v[-1])
            keep[q] &= ~np.uint64(1 << k)
            dropped.append((q, k))
    assert dropped and plain[0]["n_valid"][q_all] >= 1
    h.verify_masked(torch.from_numpy(keep.view(np.int64)).cuda())
    got, per_q, score = _batch_check(h, res, ids, rows, "verify", (cn, "masked"))
    for q, k in dropped:
        assert score[q, k] == -1.0 and per_q[q][1][k] == -1 and got["n_valid"][q] == plain[0]["n_valid"][q] - 1, (cn, q, k)
    assert got["n_valid"][q_all] == 0 and got["n_set"][q_all] == 0 and (per_q[q_all][1] == -1).all()
    if cn > 1:
        assert (got["n_set"] >= 2).any()
    # a partly stored pose map: a third of the frames dropped, one stored pose holding a NaN
    h.verify()
    used = np.unique(np.concatenate([res.cand_frame[q][np.flatnonzero(degree0[q] >= 0)] for q in range(NQ)]))
    gone = ids[::3]
    bad = int([f for f in used if f % 3 != 0][0])
    poses = rows.astype(np.float32).copy()
    poses[bad, 5] = np.nan
    h.set_frame_poses(gone, None)
    h.set_frame_poses(np.array([bad]), poses[bad:bad + 1])
    left = np.array([i for i in ids if i % 3 != 0])
    got, per_q, score = _batch_check(h, res, left, poses[left], "verify", (cn, "partly stored"))
    lost = np.array([sum(1 for k in np.flatnonzero(degree0[q] >= 0) if res.cand_frame[q, k] % 3 == 0 or res.cand_frame[q, k] == bad)
                     for q in range(NQ)])
    assert lost.sum() >= 1 and np.isin(gone, used).any() and np.array_equal(got["n_valid"], plain[0]["n_valid"] - lost), (cn, lost)
    for q in range(NQ):
        for k in np.flatnonzero(degree0[q] >= 0):
            f = int(res.cand_frame[q, k])
            assert (per_q[q][1][k] == -1) == (f % 3 == 0 or f == bad), (cn, q, k)
    if cn > 1:
        assert (got["n_set"] >= 2).any()
    h.close()
