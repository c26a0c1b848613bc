"""The workloads of tests/test_gpu_verify_edges.py really reach the edges of candidate_verify (oracle only, no GPU):
combinations within ulps of the 3 m threshold on both sides, every decade of margin, the scale ladder, the gates of the
matrix-core vote pass, vote ties, the 4-vote rule and the list lengths around the tiles and skip_len."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _verify_edges as ve  # noqa: E402

EPS = 1.3e-5         # SGTD_VM_EPS of verify_mfma.hip.h


@pytest.fixture(scope="module")
def desc_audit(oracle_mod):
    """per candidate: scenario, oracle answer, its hypotheses and every (hypothesis, pair, vertex) distance"""
    wl = ve.descriptor_workload(oracle_mod)
    o = oracle_mod.OracleManager()
    wl.load(o, oracle_mod)
    acc = oracle_mod.OrcVerifyAudit()
    cands = []
    for qi in range(len(wl.queries)):
        sel = o.select(wl.query_descs(oracle_mod, qi))
        assert len(sel["cand_frame"]) == len(wl.queries[qi])
        for k, f in enumerate(sel["cand_frame"]):
            sc = wl.scen[f]
            n = int(sel["cand_off"][k + 1] - sel["cand_off"][k])
            assert n == sc.n and np.array_equal(sel["q_idx"][sel["cand_off"][k]:sel["cand_off"][k + 1]] - sel["q_idx"][sel["cand_off"][k]], np.arange(n))
            hyps = o.verify_hyp_solutions(k)
            o.audit_verify(k, hyps, acc)
            with np.errstate(invalid="ignore", over="ignore"):
                d = ve.vertex_dists(hyps[:, None, :], sc.qv[None], sc.ev[None])       # [hyp, pair, vertex]
            cands.append(dict(sc=sc, n=n, answer=o.verify(k, n), hyps=hyps, d=d))
    return wl, cands, acc.as_dict()


def test_threshold_is_reached_within_ulps_on_both_sides(desc_audit):
    _, cands, acc = desc_audit
    assert acc["vertex_flips"] == 0 and acc["score_diffs"] == 0          # (own hypotheses: the audit's two sides agree)
    assert acc["near_calls"] >= 500
    assert acc["min_margin"] <= 1e-12
    d = np.concatenate([c["d"].ravel() for c in cands])
    d = d[np.isfinite(d)]
    assert np.sum(d == 3.0) >= 20                                        # d^2 == 9.0 exactly: `<` against `<=`
    m = d - 3.0
    for e in range(-14, 0):
        lo, hi = 10.0 ** e, 10.0 ** (e + 1)
        above = np.sum((m >= lo) & (m < hi))
        below = np.sum((-m >= lo) & (-m < hi))
        assert above >= 16 and below >= 16, (e, above, below)
    for k in (1, 2):                                                     # one and two ulps of 3 m, both sides
        assert np.sum(m == k * ve.ULP3) >= 4 and np.sum(m == -k * ve.ULP3) >= 4


def test_list_lengths_and_selection_edges(desc_audit):
    _, cands, _ = desc_audit
    lengths = {c["n"] for c in cands}
    assert {5, 6, 31, 32, 33, 49, 50, 51, 64, 65} <= lengths and max(lengths) >= 1000
    by = {c["sc"].tag: c for c in cands}
    assert by["votes4"]["answer"][0] == 4 and by["votes4of5"]["answer"][0] == 4 and by["votes3"]["answer"][0] == -1
    long = by["long/n1003/km"]
    skip = long["n"] // 50 + 1
    assert skip > 1 and len(long["hyps"]) > 32 and long["n"] % 32 != 0   # two hypothesis tiles, a tail tile
    # ties: the first maximum (:507-514) decides between hypotheses with equal votes and different (R, t) — at least one
    # of them tied because a decision within 1e-6 of the threshold went one way for one and the other way for the other
    near_ties = 0
    for c in cands:
        with np.errstate(invalid="ignore"):
            inl = np.all(c["d"] < 3.0, axis=2)
        votes = inl.sum(axis=1)
        top = np.flatnonzero(votes == votes.max())
        if len(top) < 2 or votes.max() < 4:
            continue
        h0 = top[0]
        for h in top[1:]:
            if np.array_equal(c["hyps"][h], c["hyps"][h0]):
                continue
            differ = inl[h] != inl[h0]
            with np.errstate(invalid="ignore"):
                edge = np.any(np.abs(c["d"][h] - 3.0) < 1e-6, axis=1) | np.any(np.abs(c["d"][h0] - 3.0) < 1e-6, axis=1)
            if np.any(differ & edge):
                near_ties += 1
                break
    assert near_ties >= 3


def test_gates_and_scales_are_crossed(desc_audit):
    _, cands, _ = desc_audit
    by = {c["sc"].tag: c for c in cands}
    # the scale ladder: coordinates up to 9e5 m (the pair features' scale s below 2^-24)
    for off in (1e2, 1e3, 1e4, 2e5, 9e5):
        c = by["scale/%g/r37" % off]
        V = np.max(np.abs(c["sc"].qv).sum(axis=2))
        s = 2.0 ** np.floor(np.log2(2.9 / (EPS * ((V + np.max(np.abs(c["hyps"][:, 9:]).sum(axis=1)) + V) ** 2 + 16))))
        assert V >= off and (off < 9e5 or s <= 2.0 ** -24)
        assert c["answer"][0] >= 4
    # |t|_1 just below and above 1e5 (cand_exact), and a hypothesis feature |t|^2 >= 2.5e4 (tau = NaN)
    t1 = {tag: np.max(np.abs(by[tag]["hyps"][:, 9:]).sum(axis=1)) for tag in ("t1/99900", "t1/100100", "t1/mixed")}
    assert 0.998e5 < t1["t1/99900"] < 1e5 < t1["t1/100100"] < 1.002e5 and t1["t1/mixed"] >= 1e5
    mixed_t = np.abs(by["t1/mixed"]["hyps"][:, 9:]).sum(axis=1)
    assert np.sum(mixed_t < 10) >= 10                                   # small hypotheses next to the large one
    assert any(np.max(np.sum(c["hyps"][:, 9:] ** 2, axis=1)) >= 2.5e4 for c in cands)
    # the per-pair wild gate: a coordinate >= 1e6, NaN, inf — never at a hypothesis position (skip_len 2)
    for name, pred in (("1e6", lambda x: np.abs(x) >= 1e6), ("2e6", lambda x: np.abs(x) >= 1e6), ("nan", np.isnan), ("inf", np.isinf)):
        c = by["wild/" + name]
        rows = np.flatnonzero(np.any(pred(c["sc"].ev.reshape(c["n"], 9)), axis=1))
        skip = c["n"] // 50 + 1
        assert len(rows) >= 3 and np.all(rows % skip != 0), name
        assert np.all(np.isfinite(c["hyps"])) and c["answer"][0] >= 4
    # the orthogonality defect gate (1e-6): degenerate triangles as hypotheses
    R = by["degenerate"]["hyps"][:, :9].reshape(-1, 3, 3)
    defect = np.abs(np.einsum("hki,hkj->hij", R, R) - np.eye(3)).max(axis=(1, 2))
    assert np.sum(defect > 1e-6) >= 2 and np.sum(defect < 1e-12) >= 2
    # one candidate (>= 1000 pairs) whose combinations lie inside the error band: the per-wave queue fills and
    # drains within the candidate (32 pairs x 47 hypotheses per tile > SGTD_VM_QCAP = 1024)
    c = by["long/n1003/km"]
    V = np.abs(c["sc"].qv).sum(axis=2).max()
    W = np.abs(c["sc"].ev).sum(axis=2).max()
    T = np.abs(c["hyps"][:, 9:]).sum(axis=1)
    band = EPS * ((V + T + W) ** 2 + 16)
    inband = np.abs(c["d"].max(axis=2) ** 2 - 9.0) < band[:, None]
    n_anchor_hyps = -(-200 // skip)                                     # (the first 200 pairs follow the motion)
    assert inband[:n_anchor_hyps].mean() > 0.99
    assert inband[:, :32].sum() > 1024


def test_frame_batch_reaches_the_threshold(oracle_mod):
    """the frame batch: 96 query frames x 50 candidates (the <4> kernel and the ordered dispatch), near-threshold
    combinations from the moved clusters (every fourth query audited)"""
    from sgtd_amd import synth
    m, qx, ql, _ = ve.frame_batch(synth)
    assert qx.shape[0] * 50 >= 4096
    o = oracle_mod.OracleManager()
    o.add_frames(m.xyz, m.label)
    acc = oracle_mod.OrcVerifyAudit()
    n_cand = 0
    for q in range(0, qx.shape[0], 4):
        o.build(qx[q], ql[q], export=False)
        sel = o.select()
        n_cand += len(sel["cand_frame"])
        for k in range(len(sel["cand_frame"])):
            o.audit_verify(k, o.verify_hyp_solutions(k), acc)
    assert n_cand >= 20 * 24
    assert acc.near_calls >= 100 and acc.min_margin <= 1e-9
