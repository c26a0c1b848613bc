"""sgtd_refine_poses at the edges of refine_kernel, in every form after which the call is accepted, against the numpy
restatement (tests/_refine_ref.py) with test_gpu_refine.py's rules (_compare: n_pairs, the moments and rmse_verify bit
for bit, rmse bit for bit at the device's own pose, the pose to 1e-9, a rotation for every candidate).  The workloads
are tests/_refine_edges.py's; tests/test_refine_edges.py shows on the CPU that they reach the edges.  The pose
comparison is waived for _refine_edges.WAIVED alone (rank-1 H) — a fixed list, counted in every run.

  candidate_selector + verify      every family at iterations 1, 2, 3, 8; sgtd_verify's results unchanged after each call
  search_frame                     every family, the same bits
  verify_masked                    the mix query under masks that cut live candidates
  attach_table                     a view on the same table, the same bits
  devices=[0, 0, 0]                three shards, the same bits
  query_frames + verify_masked     8 frames alone (400 workgroups: as the candidates stand) and among 76 filler frames
                                   (4200 workgroups: the frame-ordered dispatch), the same bits, and the restatement's
  reuse                            8 iterations, a shorter batch, a longer one, the first again: the first bits
The dispatch form has no counter of its own: each test asserts the size that selects it (4096 workgroups)."""
import numpy as np
import pytest

import _refine_edges as re_
import _verify_edges as ve
from test_gpu_refine import _bits, _compare, _expected, _same_refined, _snapshot, _stats

pytestmark = pytest.mark.gpu

ITERATIONS = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from sgtd_amd import manager, synth
    oracle.build_library()
    return oracle, manager, synth


@pytest.fixture(scope="module")
def case(mods):
    oracle, manager, _ = mods
    wl = re_.workload(re_.all_scenarios(oracle))
    g = manager.STDescManager()
    wl.load(g, manager)
    g.finalize()
    yield wl, g
    g.close()


def _tags(wl, res, q=0):
    return [wl.scen[int(f)].tag for f in res.cand_frame[q, :int(res.n_cand[q])]]


def _check(g, wl, res, it, where):
    """the refined results of query 0 against the restatement -> {tag: expectation}, the device's results"""
    cn = g.config_setting_["candidate_num"]
    got = g.result_refined(0)
    exp, _ = _expected(g, res, 0, it)
    st = _stats()
    _compare(got, exp, cn, where, st)
    tags = _tags(wl, res)
    by_tag = {tags[k]: e for k, e in exp.items()}
    assert st["collinear"] == sum(t in re_.WAIVED for t in by_tag), where          # the waiver is the fixed list
    return by_tag, got


def _select(g, wl, manager, qi):
    g.candidate_selector(wl.query_descs(manager, qi))
    return g.results()


@pytest.mark.parametrize("family", ["cap", "lanes", "chain", "stop", "solve", "mix", "shell"])
def test_candidate_selector_and_verify(case, mods, family):
    _, manager, _ = mods
    wl, g = case
    qi = wl.family.index(family)
    res = _select(g, wl, manager, qi)
    g.verify()
    before = _snapshot(g, res, 1)
    seen = {}
    for it in ITERATIONS:
        g.refine_poses(it)
        seen[it], _ = _check(g, wl, res, it, (family, it))
        after = _snapshot(g, res, 1)
        assert len(before) == len(after) and all(np.array_equal(a, b) for a, b in zip(before, after)), (family, it)
    live = [wl.scen[s].tag for s in wl.queries[qi] if wl.scen[s].tag not in re_.REJECTED and not wl.scen[s].tag.startswith("mix/dead")]
    assert sorted(seen[8]) == sorted(live)
    e = seen[8]
    if family == "cap":      # which side of the LDS image the last fit is on, and the fall-back after a crossing
        assert [e["cap/all%d" % n]["n_pairs"] for n in (895, 896, 897)] == [895, 896, 897]
        assert (seen[1]["cap/grow"]["n_pairs"], seen[2]["cap/grow"]["n_pairs"], e["cap/grow"]["n_pairs"], e["cap/grow"]["fits"]) == (800, 995, 1000, 3)
        assert (seen[1]["cap/grow897"]["n_pairs"], e["cap/grow897"]["n_pairs"], e["cap/grow897"]["stop"]) == (800, 897, "same")
        assert (seen[1]["cap/shrink"]["n_pairs"], e["cap/shrink"]["n_pairs"], e["cap/shrink"]["stop"]) == (910, 850, "same")
        assert (seen[1]["cap/shrink896"]["n_pairs"], e["cap/shrink896"]["n_pairs"]) == (956, 896)
    if family == "chain":
        assert e["chain/noisy"]["fits"] == 8 and e["chain/noisy"]["stop"] is None and seen[3]["chain/noisy"]["fits"] == 3
        assert (e["chain/swap"]["fits"], e["chain/swap"]["n_pairs"], seen[1]["chain/swap"]["n_pairs"]) == (2, 150, 150)
        assert not np.array_equal(e["chain/swap"]["set"], seen[1]["chain/swap"]["set"])
    if family == "stop":
        assert [(e["stop/next%d" % k]["n_pairs"], e["stop/next%d" % k]["stop"]) for k in (3, 4, 5)] == [(4, "few"), (4, "same"), (5, "same")]
    if family == "shell":
        assert (seen[1]["shell"]["n_pairs"], seen[2]["shell"]["n_pairs"]) == (112, 116)
    if family == "solve":
        assert np.linalg.det(e["solve/mirror"]["H"]) < 0                                   # the K correction ran (det(V U^T) = -1)
        assert not e["solve/planar"]["H"][2].any() and not e["solve/planar"]["H"][:, 2].any()
    if family == "mix":
        score, _, _ = g.result_verify(0)
        n_c = int(res.n_cand[0])
        assert n_c == 7 < g.config_setting_["candidate_num"] and [bool(s >= 0) for s in score[:n_c]].count(False) == 3
        assert [bool(a >= 0) != bool(b >= 0) for a, b in zip(score[:n_c], score[1:n_c])] == [True] * 6       # interleaved


def test_long_lane(mods):
    """one thread owns 102 slots of the LDS image, every other thread none (a list of 25 900 pairs)"""
    _, manager, _ = mods
    wl = ve.Workload(re_.long_lane())
    g = manager.STDescManager()
    wl.load(g, manager)
    g.finalize()
    res = _select(g, wl, manager, 0)
    g.verify()
    for it in (1, 2):
        g.refine_poses(it)
        e, _ = _check(g, wl, res, it, ("long", it))
        pos = np.flatnonzero(e["lanes/res7_long"]["set"])
        assert len(pos) == 102 and set(pos % 256) == {7}
    g.close()


def _refined_of(g, wl, manager, qi, it, how="selector"):
    if how == "selector":
        _select(g, wl, manager, qi)
        g.verify()
    else:
        d = wl.query_descs(manager, qi)
        assert g.search_frame(d, capacity=d.n)["status"] == 0
    g.refine_poses(it)
    return g.result_refined(0)


def test_search_frame_view_and_shards(case, mods):
    """sgtd_search_frame, a view and a three-shard handle give candidate_selector + verify's bits on every family"""
    _, manager, _ = mods
    wl, g = case
    view = manager.STDescManager()
    view.attach_table(g)
    multi = manager.STDescManager(devices=[0, 0, 0])
    wl.load(multi, manager)
    multi.finalize()
    assert multi.device_count == 3
    try:
        for qi, family in enumerate(wl.family):
            for it in (2, 8):
                want = _refined_of(g, wl, manager, qi, it)
                assert (want["n_pairs"] > 0).any()
                _same_refined(want, _refined_of(g, wl, manager, qi, it, "frame"), (family, it, "search_frame"))
                _same_refined(want, _refined_of(view, wl, manager, qi, it), (family, it, "view"))
                _same_refined(want, _refined_of(view, wl, manager, qi, it, "frame"), (family, it, "view, search_frame"))
                _same_refined(want, _refined_of(multi, wl, manager, qi, it), (family, it, "shards"))
    finally:
        view.close()
        multi.close()


def test_verify_masked_on_the_mix_query(case, mods):
    import torch
    _, manager, _ = mods
    wl, g = case
    qi = wl.family.index("mix")
    full = _refined_of(g, wl, manager, qi, 3)
    live = np.flatnonzero(full["n_pairs"] > 0)
    assert live.tolist() == [0, 2, 4, 6]
    for mask in (0b0000001, 0b1000000, 0b0010100, 0b1111011, 0b0101010, 0):
        g.query_descs(wl.query_descs(manager, qi))
        g.verify_masked(torch.tensor([mask], dtype=torch.int64, device="cuda"))
        torch.cuda.synchronize()
        g.refine_poses(3)
        r = g.result_refined(0)
        for k in range(g.config_setting_["candidate_num"]):
            if (mask >> k) & 1 and k in live:
                for key in ("rot", "t", "rmse", "rmse_verify", "moments"):
                    assert np.array_equal(_bits(r[key][k]), _bits(full[key][k])), (mask, k, key)
                assert r["n_pairs"][k] == full["n_pairs"][k]
            else:
                assert r["n_pairs"][k] == 0 and np.isnan(r["rmse"][k]) and np.isnan(r["moments"][k]).all() and not r["rot"][k].any(), (mask, k)


def test_reuse_shorter_then_longer(case, mods):
    """the handle's flag buffer reused by a batch of fewer listed pairs, grown by one of more, and the first batch again"""
    _, manager, _ = mods
    wl, _ = case
    g = manager.STDescManager()
    wl.load(g, manager)
    g.finalize()
    listed = {}
    first = None
    for family in ("cap", "stop", "lanes", "cap"):
        qi = wl.family.index(family)
        res = _select(g, wl, manager, qi)
        listed[family] = int(res.pair_off[0, g.config_setting_["candidate_num"]])
        g.verify()
        g.refine_poses(8)
        _check(g, wl, res, 8, ("reuse", family))
        if first is None:
            first = g.result_refined(0)
    assert listed["stop"] < listed["cap"] < listed["lanes"]
    _same_refined(first, g.result_refined(0), "reuse")
    g.close()


def test_both_dispatch_forms(mods):
    """query_frames + verify: 8 query frames alone (as the candidates stand) and among 76 filler frames (4200 workgroups:
    sorted by candidate frame) — the same bits, and the restatement's; masked candidates (sgtd_verify_masked) and slots
    past n_cand lie between and behind live ones in both.  (The one keypoint map of this file: 24 frames of 120 keypoints, __graft_entry__.smoke's.)"""
    import torch
    _, manager, synth = mods
    m = synth.make_map(24, 120, stream=3)
    qs, fill = synth.make_queries(m, 8, stream=3), synth.make_queries(m, 76, stream=4)
    g = manager.STDescManager()
    g.add_frames(m.xyz, m.label)
    g.finalize()
    cn = g.config_setting_["candidate_num"]
    res = g.query_frames(qs.xyz, qs.label)
    assert 8 * cn < 4096
    # (every candidate of this map is accepted: the candidates without a result between live ones are masked ones)
    keep = torch.tensor([0x2DB6DB6DB6DB6DB6 >> (q % 3) for q in range(8)] + [-1] * 76, dtype=torch.int64, device="cuda")
    g.verify_masked(keep[:8].contiguous())
    torch.cuda.synchronize()
    before = _snapshot(g, res, 8)
    alone = {}
    for it in (1, 3, 8):
        g.refine_poses(it)
        alone[it] = [g.result_refined(q) for q in range(8)]
    after = _snapshot(g, res, 8)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    st = _stats()
    dead = past = 0
    for q in range(8):
        exp, score = _expected(g, res, q, 8)
        _compare(alone[8][q], exp, cn, ("alone", q), st)
        n_c = int(res.n_cand[q])
        dead += int((score[:n_c] < 0).sum())
        past += cn - n_c
    assert st["verified"] >= 8 and st["collinear"] == 0 and dead >= 1 and past >= 1
    big = g.query_frames(np.concatenate([qs.xyz, fill.xyz]), np.concatenate([qs.label, fill.label]))
    assert 84 * cn >= 4096
    assert np.array_equal(big.cand_frame[:8], res.cand_frame) and np.array_equal(big.pair_off[:8], res.pair_off)
    g.verify_masked(keep)
    torch.cuda.synchronize()
    for it in (1, 3, 8):
        g.refine_poses(it)
        for q in range(8):
            _same_refined(alone[it][q], g.result_refined(q), ("sorted", it, q))
    g.close()
