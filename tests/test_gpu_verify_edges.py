"""candidate_verify at the 3 m threshold in every dispatch form of the vote pass, against the oracle (bit for bit: score,
R and t, the inlier list, SearchLoop's choice, the fused inlier entries).  Workloads: tests/_verify_edges.py.

  descriptor scenarios  candidate_selector + verify          verify_mfma_kernel<8>
                        search_frame                         <8> with the inlier counts (guarded form)
                        SGTD_VERIFY_FORM=valu                verify_kernel (packed f32 pre-test)
                        SGTD_VERIFY_EXACT=1                  <8>, every combination through the exact test (queue drains)
                        devices=[0, 0, 0]                    multi::verify over three shards
  frame batch (96 x 50) query_frames + verify                verify_mfma_kernel<4> + the frame-ordered dispatch
                        SGTD_VERIFY_ORDER=0 (own process)    <4> as the candidates stand

Run as a script (`python tests/test_gpu_verify_edges.py frame-batch`) it checks the frame batch in a process of its own
(SGTD_VERIFY_ORDER is read once per process).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _verify_edges as ve  # noqa: E402

pytestmark = pytest.mark.gpu


def _oracle_answers(o, sel):
    """per candidate of the last select: (n_pairs, score, t, rot, inlier positions); SearchLoop's choice (:105-146)"""
    out = []
    best_s, best_k = 0.0, -1
    for k in range(len(sel["cand_frame"])):
        n = int(sel["cand_off"][k + 1] - sel["cand_off"][k])
        s, t, rot, idx = o.verify(k, n)
        out.append((n, s, t, rot, idx))
        if s > best_s:
            best_s, best_k = s, k
    return out, (best_k, best_s)


def _check_query(g, res, q, sel, ans, choice, tag, bc=None, bf=None, bs=None):
    """the device's verification of query q of the last batch (result_verify, result_inliers, result_inlier_entries,
    search_loop) against the oracle's answers"""
    n_c = len(ans)
    assert int(res.n_cand[q]) == n_c, tag
    np.testing.assert_array_equal(res.cand_frame[q, :n_c], sel["cand_frame"], err_msg=tag)
    score, rot, t = g.result_verify(q)
    off, iq, ent = g.result_inlier_entries(q, int(res.pair_off[q, n_c]))
    qi_all, de_all = g.result_pairs(q, res)
    voted = 0
    for k, (n, o_s, o_t, o_rot, o_idx) in enumerate(ans):
        where = (tag, q, k, int(sel["cand_frame"][k]))
        assert score[k] == o_s, where
        if o_s < 0:
            assert int(off[k + 1] - off[k]) == 0, where
            continue
        voted += 1
        assert np.array_equal(t[k], o_t) and np.array_equal(rot[k], o_rot), where
        np.testing.assert_array_equal(g.result_inliers(q, k, n), o_idx, err_msg=str(where))
        a, b = int(off[k]), int(off[k + 1])
        assert b - a == len(o_idx), where
        at = int(res.pair_off[q, k]) + np.asarray(o_idx, np.int64)
        np.testing.assert_array_equal(iq[a:b], qi_all[at], err_msg=str(where))
        np.testing.assert_array_equal(ent.frame[a:b], np.full(b - a, sel["cand_frame"][k]), err_msg=str(where))
        want = g.fetch_entries(de_all[at])
        assert np.array_equal(ent.side[a:b], want.side) and np.array_equal(ent.vertex[a:b], want.vertex, equal_nan=True), where
    assert np.all(score[n_c:] == -1), tag
    if bc is not None:
        best_k, best_s = choice
        if best_s > g.icp_threshold_:
            assert (bc[q], bf[q], bs[q]) == (best_k, sel["cand_frame"][best_k], best_s), (tag, q)
        else:
            assert (bc[q], bf[q], bs[q]) == (-1, -1, 0), (tag, q)
    return voted


# ---- descriptor scenarios ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def desc_case():
    from oracle import oracle
    oracle.build_library()
    wl = ve.descriptor_workload(oracle)
    o = oracle.OracleManager()
    wl.load(o, oracle)
    expect = []
    for qi in range(len(wl.queries)):
        sel = o.select(wl.query_descs(oracle, qi))
        assert [wl.scen[f].n for f in sel["cand_frame"]] == list(np.diff(sel["cand_off"]))     # one pair per key
        expect.append((sel,) + _oracle_answers(o, sel))
    return wl, expect


class _One:
    """BatchResult of a one-query call (candidate_selector)"""

    def __init__(self, g):
        self.__dict__.update(g.results().__dict__)


def _run_descriptor_scenarios(g, wl, expect, tag):
    from sgtd_amd import manager
    wl.load(g, manager)
    voted = 0
    for qi, (sel, ans, choice) in enumerate(expect):
        lists = g.candidate_selector(wl.query_descs(manager, qi))
        assert [l.match_id_[1] for l in lists] == list(sel["cand_frame"])
        g.verify()
        bc, bf, bs = g.search_loop()
        voted += _check_query(g, _One(g), 0, sel, ans, choice, tag, bc, bf, bs)
    return voted


@pytest.mark.parametrize("form", ["mfma", "valu", "exact"])
def test_descriptor_scenarios(desc_case, form, monkeypatch):
    from sgtd_amd import manager
    wl, expect = desc_case
    if form == "valu":
        monkeypatch.setenv("SGTD_VERIFY_FORM", "valu")
    if form == "exact":
        monkeypatch.setenv("SGTD_VERIFY_EXACT", "1")
    g = manager.STDescManager()
    voted = _run_descriptor_scenarios(g, wl, expect, form)
    assert voted >= 70
    g.close()


def test_descriptor_scenarios_search_frame(desc_case):
    """sgtd_search_frame: the guarded form (enqueued behind an unwaited batch, inlier counts from the vote kernel)"""
    from sgtd_amd import manager
    wl, expect = desc_case
    g = manager.STDescManager()
    wl.load(g, manager)
    for qi, (sel, ans, choice) in enumerate(expect):
        cap = int(sel["cand_off"][-1])
        out = g.search_frame(wl.query_descs(manager, qi), capacity=cap)
        assert out["status"] == 0 and out["n_cand"] == len(ans)
        np.testing.assert_array_equal(out["cand_frame"][:len(ans)], sel["cand_frame"])
        for k, (n, o_s, o_t, o_rot, o_idx) in enumerate(ans):
            where = ("search_frame", qi, k, int(sel["cand_frame"][k]))
            assert out["score"][k] == o_s, where
            a, b = int(out["inlier_off"][k]), int(out["inlier_off"][k + 1])
            if o_s < 0:
                assert a == b, where
                continue
            assert np.array_equal(out["t"][k], o_t) and np.array_equal(out["rot"][k], o_rot), where
            assert b - a == len(o_idx), where
            lo = int(sel["cand_off"][k])
            np.testing.assert_array_equal(out["inlier_q_idx"][a:b], sel["q_idx"][lo + np.asarray(o_idx, np.int64)], err_msg=str(where))
            np.testing.assert_array_equal(out["entries"].frame[a:b], np.full(b - a, sel["cand_frame"][k]), err_msg=str(where))
    g.close()


def test_descriptor_scenarios_multi_device_handle(desc_case):
    """one handle over three shards on this GPU: the candidates' verification on their owners (multi::verify)"""
    from sgtd_amd import manager
    wl, expect = desc_case
    g = manager.STDescManager(devices=[0, 0, 0])
    assert _run_descriptor_scenarios(g, wl, expect, "multi") >= 70
    g.close()


# ---- the frame batch ---------------------------------------------------------------------------------------------
def frame_batch_check():
    """query_frames + verify of the 96-frame batch against the oracle; returns the candidates with a result"""
    from oracle import oracle
    from sgtd_amd import manager, synth
    oracle.build_library()
    m, qx, ql, _ = ve.frame_batch(synth)
    o = oracle.OracleManager()
    o.add_frames(m.xyz, m.label)
    g = manager.STDescManager()
    g.add_frames(m.xyz, m.label)
    res = g.query_frames(qx, ql)
    assert qx.shape[0] * g.config_setting_["candidate_num"] >= 4096       # the ordered dispatch's size
    g.verify()
    bc, bf, bs = g.search_loop()
    voted = 0
    for q in range(qx.shape[0]):
        o.build(qx[q], ql[q], export=False)
        sel = o.select()
        ans, choice = _oracle_answers(o, sel)
        voted += _check_query(g, res, q, sel, ans, choice, "frames", bc, bf, bs)
    g.close()
    return voted


def test_frame_batch_ordered_dispatch():
    assert frame_batch_check() >= 500


def test_frame_batch_unordered_in_a_process_of_its_own():
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "frame-batch"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, SGTD_VERIFY_ORDER="0"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "frame batch ok" in p.stdout


if __name__ == "__main__":
    if sys.argv[1:] == ["frame-batch"]:
        n = frame_batch_check()
        assert n >= 500, n
        print("frame batch ok: %d candidates with a result" % n)
