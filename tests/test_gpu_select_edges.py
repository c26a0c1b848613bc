"""candidate_selector at cell, slice and gate edges in every form, against the oracle: the full vote vector, M
(stats()["last_M"]), the candidates, their votes, pair_off and every match list's (q_idx, db_entry) in order.
Workloads: tests/_select_edges.py (one handle per rough value).

  configs  shipped (cbits 6, 2 sub bits, u32 keys), res 2 / max_len 15 (4, 4, u32), res 1 / max_len 15 (5, 5, u32),
           res 0.5 / max_len 50 (7, 6, u64), res 0.25 / max_len 50 (8, 4, u64) — u32 keys take small_order_kernel for a
           one-frame call, u64 keys the general ordering
  forms    candidate_selector; search_frame(lists_only=True); SGTD_SELECT_MODE 1 and 2; SGTD_COARSE_AT=0;
           SGTD_WHOLE_AT=0 with a tail segment; SGTD_HOME_SUB_BITS 0 and 6; entries appended after a query (a tail
           segment); a three-shard handle on one GPU; SGTD_SMALL_ORDER=0 (read once per process: a process of its own)

Run as a script (`python tests/test_gpu_select_edges.py small0`) it checks every config with SGTD_SMALL_ORDER=0.
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

import _select_edges as se  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = {
    "shipped": dict(),
    "res2_len15": dict(std_side_resolution=2.0, descriptor_max_len=15.0),
    "res1_len15": dict(std_side_resolution=1.0, descriptor_max_len=15.0),
    "res0.5_len50": dict(std_side_resolution=0.5, descriptor_max_len=50.0),
    "res0.25_len50": dict(std_side_resolution=0.25, descriptor_max_len=50.0),
}
FORMS = {
    "selector": {}, "frame": {}, "mode1": {"SGTD_SELECT_MODE": "1"}, "mode2": {"SGTD_SELECT_MODE": "2"},
    "coarse0": {"SGTD_COARSE_AT": "0"}, "whole0": {"SGTD_COARSE_AT": "0", "SGTD_WHOLE_AT": "0"},
    "sub0": {"SGTD_HOME_SUB_BITS": "0"}, "sub6": {"SGTD_HOME_SUB_BITS": "6"}, "tail": {}, "multi": {},
}
FIELDS = ("side", "label", "frame")

_EXPECT = {}


def expected(rough, stamped=False):
    """(workload, the oracle's answer per query set with its lists' table entries), once per rough value (stamped: one
    frame per call, stamped with the current frame id: the workload of the tail and multi-device forms)"""
    if (rough, stamped) not in _EXPECT:
        from oracle import oracle
        oracle.build_library()
        wl = se.workload(rough, stamped)
        o = oracle.OracleManager(rough_dis_threshold=rough)
        wl.load(o, oracle)
        out = []
        for k in range(len(wl.sets)):
            sel = o.select(wl.query_descs(oracle, k))
            sel.update(votes=o.votes(), M=o.counters()["M"])
            ent = o.fetch_entries(sel["db_entry"])
            sel["entries"] = {f: getattr(ent, f).copy() for f in FIELDS}
            out.append(sel)
        _EXPECT[(rough, stamped)] = (wl, out)
    return _EXPECT[(rough, stamped)]


def _check_votes(g, exp, tag):
    lo, v = g.result_votes(0)
    ov = exp["votes"]
    n = min(len(v), len(ov) - lo)
    np.testing.assert_array_equal(v[:n].astype(np.float64), ov[lo:lo + n], err_msg=tag)
    assert v[n:].sum() == 0 and ov[:lo].sum() == 0 and ov[lo + n:].sum() == 0, tag
    assert g.stats()["last_M"] == exp["M"], tag


def _check_set(g, exp, tag, multi=False):
    res = g.results()
    nc = int(res.n_cand[0])
    assert nc == len(exp["cand_frame"]), tag
    np.testing.assert_array_equal(res.cand_frame[0, :nc], exp["cand_frame"], err_msg=tag)
    np.testing.assert_array_equal(res.cand_votes[0, :nc], exp["cand_votes"], err_msg=tag)
    np.testing.assert_array_equal(res.pair_off[0, :nc + 1], exp["cand_off"], err_msg=tag)
    qi, de = g.result_pairs(0, res)
    np.testing.assert_array_equal(qi, exp["q_idx"], err_msg=tag)
    if multi:       # (the entry ids are the shards' own: the same entries)
        got = g.fetch_entries(de)
        for f in FIELDS:
            np.testing.assert_array_equal(getattr(got, f), exp["entries"][f], err_msg=tag + " " + f)
    else:
        np.testing.assert_array_equal(de, exp["db_entry"], err_msg=tag)
    _check_votes(g, exp, tag)


def _check_frame(g, mod, wl, k, exp, tag):
    """search_frame(lists_only=True): the candidates and every pair of every list with its table entry"""
    cap = max(int(exp["cand_off"][-1]), 1)
    out = g.search_frame(wl.query_descs(mod, k), capacity=cap, lists_only=True)
    assert out["status"] == 0, tag
    nc = len(exp["cand_frame"])
    assert out["n_cand"] == nc, tag
    np.testing.assert_array_equal(out["cand_frame"][:nc], exp["cand_frame"], err_msg=tag)
    np.testing.assert_array_equal(out["cand_votes"][:nc], exp["cand_votes"], err_msg=tag)
    np.testing.assert_array_equal(out["pair_off"][:nc + 1], exp["cand_off"], err_msg=tag)
    np.testing.assert_array_equal(out["inlier_q_idx"], exp["q_idx"], err_msg=tag)
    for f in FIELDS:
        np.testing.assert_array_equal(getattr(out["entries"], f), exp["entries"][f], err_msg=tag + " " + f)
    _check_votes(g, exp, tag)


def run_form(config, form, roughs=se.ROUGHS):
    """every query set of every rough value through one (config, form); returns the number of candidates checked"""
    from sgtd_amd import manager
    n_cand = 0
    for rough in roughs:
        # (a multi-device table takes one frame per call, stamped with the current frame id; a tail segment holds appended
        # frames newer than every frame before them, with the frame ids in insertion order, else the append rebuilds
        # one segment)
        wl, exp = expected(rough, stamped=form in ("tail", "whole0", "multi"))
        kw = dict(CONFIGS[config], rough_dis_threshold=rough)
        g = manager.STDescManager(devices=[0, 0, 0], **kw) if form == "multi" else manager.STDescManager(**kw)
        if form in ("tail", "whole0"):
            h = len(wl.adds) // 2
            wl.load(g, manager, 0, h)
            g.candidate_selector(wl.query_descs(manager, 0))        # (the table is built: what follows goes to a tail)
            wl.load(g, manager, h, None)
        else:
            wl.load(g, manager)
        for k in range(len(wl.sets)):
            tag = "%s/%s/rough%g/set%d/%s" % (config, form, rough, k, wl.sets[k][2])
            if form == "frame":
                _check_frame(g, manager, wl, k, exp[k], tag)
            else:
                g.candidate_selector(wl.query_descs(manager, k))
                _check_set(g, exp[k], tag, multi=form == "multi")
            if k == 0 and form in ("tail", "whole0"):
                assert g.stats()["tail_entries"] > 0, tag
            n_cand += len(exp[k]["cand_frame"])
        g.close()
    return n_cand


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_equals_the_oracle(config, form, monkeypatch):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    assert run_form(config, form) >= 200


def test_small_order_off_in_a_process_of_its_own():
    """SGTD_SMALL_ORDER=0 (read once per process): the one-frame call takes the general ordering in every config"""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "small0"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, SGTD_SMALL_ORDER="0"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "small0 ok" in p.stdout


def test_table_side_past_65535_is_refused():
    """a table entry whose cell does not fit the 16-bit key (side >= 65535.5) is refused (SGTD_ERR_UNSUPPORTED), not
    answered; one ulp below is a table entry like any other"""
    from sgtd_amd import manager
    for side, refused in ((65535.5, True), (float(np.nextafter(65535.5, 0.0)), False)):
        wl = se.Workload(1.0)
        wl.add([[side, 3.0, 4.0]], (1, 9, 1), 0)
        wl.query([[65535.2, 3.0, 4.0]], (1, 9, 1), "refused")
        g = manager.STDescManager(rough_dis_threshold=1.0)
        wl.load(g, manager)
        if refused:
            with pytest.raises(manager.SgtdError) as ei:
                g.candidate_selector(wl.query_descs(manager, 0))
            assert ei.value.status == -6
        else:
            lists = g.candidate_selector(wl.query_descs(manager, 0))
            assert [l.match_id_[1] for l in lists] == [0] and lists[0].votes == 1 + se.BOOST
        g.close()


if __name__ == "__main__":
    if sys.argv[1:] == ["small0"]:
        assert os.environ.get("SGTD_SMALL_ORDER") == "0"
        n = sum(run_form(c, "selector") for c in CONFIGS)
        print("small0 ok: %d candidates" % n)
