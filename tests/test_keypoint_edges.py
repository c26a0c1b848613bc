"""The keypoint passes' edge workloads (tests/_keypoint_edges.py) on the CPU: OracleManager.verify gives the start poses of
the world of tests/test_gpu_align.py, the numpy restatements (tests/_overlap_ref.py, tests/_align_ref.py) the passes.
Asserted here: every workload keeps its promises; none has a decision within 1e-3 m^2 of its threshold after its first
fit, and none fits a collinear set (so the GPU file has no workload to skip); ordered_sum equals the plain loop on the
order family and three other summation orders give other bits; every mutant of the rule differs from the rule on its
named workloads (the table is printed).  The GPU file (tests/test_gpu_keypoint_edges.py) compares the device with the
same restatements on the same builders, from the device's own poses."""
import numpy as np
import pytest

import _align_ref as al
import _keypoint_edges as ke
import _overlap_ref as ov

F, NQ, SPACING = 300, 96, 12.0


@pytest.fixture(scope="module")
def suite(oracle_mod):
    """{name: (workload, R, t, {run: restatement})}, every workload on a candidate of its own"""
    from sgtd_amd import synth
    m = synth.make_map(F, 200, stream=411, spacing=SPACING)
    qs = synth.make_queries(m, NQ, stream=412)
    o = oracle_mod.OracleManager()
    o.add_frames(m.xyz, m.label)
    bl = ke.builders()
    assert len(bl) <= 80                               # (80 queries of 50 candidates: below the ordered dispatch's 4096 slots)
    poses = {}

    def verified(q):
        o.build(qs.xyz[q], qs.label[q], export=False)
        sel = o.select()
        out = []
        for k in range(len(sel["cand_frame"])):
            score, t, rot, _ = o.verify(k, int(sel["cand_off"][k + 1] - sel["cand_off"][k]))
            if score >= 0:
                poses[(q, k)] = (rot, t)
                out.append((k, int(sel["cand_frame"][k])))
        return out
    slots = ke.place(len(bl), verified, per_query=8)       # (nine queries' candidates: the oracle's select is the slow part)
    out = {}
    for i, ((name, build), (q, k, _)) in enumerate(zip(bl, slots)):
        R, t = poses[(q, k)]
        wl = build(R, t, i)
        assert wl.name == name
        out[name] = (wl, R, t, {run: ke.reference(wl, R, t, *run) for run in wl.runs})
    for q, k, _ in ke.place(16, verified, per_query=4):  # the family around the world's own query keypoints
        R, t = poses[(q, k)]
        wl = ke.own_keypoints(R, t, q, qs.xyz[q], qs.label[q])
        out["own/rigid/%d" % len(out)] = (wl, R, t, {run: ke.reference(wl, R, t, *run) for run in wl.runs})
    return out


def test_every_workload_keeps_its_promises(suite):
    for name, (wl, _, _, res) in suite.items():
        try:
            wl.promise(res)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e)) from e
    assert len(suite) == len(ke.builders()) + 16
    print("%d workloads keep their promises" % len(suite))


def test_no_workload_is_fragile_after_its_first_walk_or_collinear(suite):
    worst = min((e["late_margin"], name) for name, (_, _, _, res) in suite.items() for e in res.values())
    print("smallest margin after a first fit: %.3g m^2 (%s)" % worst)
    for name, (wl, R, t, res) in suite.items():
        for run, e in res.items():
            assert e["late_margin"] >= ke.MARGIN, (name, run, e["late_margin"])
            assert not e["collinear"], (name, run)
            if e["fragile"]:                           # only a planted threshold of the first walk may be that near
                assert ke.margin(R, t, wl, run[0]) < al.FRAGILE and name.startswith("threshold/"), (name, run)


def test_the_sizes_reach_their_edges(suite):
    assert ke.overlap_lds_bytes(ke.MAX_KP) == 83072 and ke.align_lds_bytes(ke.MAX_KP) == 95744      # both above 64 KB
    assert ke.overlap_lds_bytes(3 * ke.TILE + 3) < 65536 and ke.align_lds_bytes(3 * ke.TILE + 3) < 65536
    for nf in ke.FRAME_SIZES:
        wl = suite["sizes/frame%d/last" % nf][0]
        assert len(wl.f_lab) == nf and wl.info["deciding"] == nf - 1
        if nf > 1:
            assert suite["sizes/frame%d/tile0" % nf][0].info["deciding"] == (nf - 1) // ke.TILE * ke.TILE
    for nq in ke.QUERY_SIZES:
        assert len(suite["sizes/query%d" % nq][0].q_lab) == nq
    # the assignment in global memory is read again: three walks over more than SGTD_ALIGN_CAP query keypoints
    wl, _, _, res = suite["stop/flip1025"]
    assert len(wl.q_lab) > ke.CAP and res[(1.0, 5)]["n_fits"] == 2 and res[(1.0, 5)]["stop"] == 2
    assert wl.info["owner"] == (0, 4) and suite["stop/flip1000"][0].info["owner"] == (999 % 256, 3)    # (lane, round); lane 231: the last wave
    assert suite["stop/flip1000"][0].info["owner"][0] >= 192
    for name in ("ties/1020_1022",):
        assert len(suite[name][0].f_lab) % 4 == 3 and suite[name][0].info["lowest"] >= len(suite[name][0].f_lab) // 4 * 4   # in the unroll tail
    print("order family: minima over %s decades" % ", ".join("%.1f" % suite["order/" + k][0].info["decades"] for k in ("alternate", "only255", "midround")))


def test_ordered_sum_on_the_order_family(suite):
    for kind in ("alternate", "only255", "midround"):
        wl = suite["order/" + kind][0]
        m, take = wl.info["m"], wl.info["take"]
        a = ov.ordered_sum(m, take)
        assert a.view(np.uint64) == ov.ordered_sum_loop(m, take).view(np.uint64), kind
        if kind != "only255":                          # (four terms in one accumulator: every order is the sequential one)
            for other, s in ke.other_sums(m, take).items():
                assert s.view(np.uint64) != a.view(np.uint64), (kind, other)
                assert abs(s - a) <= 1e-12 * a, (kind, other)


def test_every_mutant_is_caught(suite):
    rows = []
    for mut, names in ke.MUTANTS.items():
        for name in names:
            wl, R, t, res = suite[name]
            same = all(ke.signature(ke.mutant_align(None, wl, R, t, *run)) == ke.signature(res[run]) for run in wl.runs)
            assert same, ("the unmutated copy differs from the restatement", name)
            caught = [run for run in wl.runs if ke.signature(ke.mutant_align(mut, wl, R, t, *run)) != ke.signature(res[run])]
            rows.append((mut, name, len(caught), len(wl.runs)))
            assert caught, (mut, name)
    print("mutant           workload                      runs that differ")
    for mut, name, c, n in rows:
        print("%-16s %-29s %d of %d" % (mut, name, c, n))
    assert {r[0] for r in rows} == set(ke.MUTANTS) and len(ke.MUTANTS) == 12


def test_the_unmutated_copy_is_the_rule_on_every_small_workload(suite):
    for name, (wl, R, t, res) in suite.items():
        if not wl.large:
            for run in wl.runs:
                assert ke.signature(ke.mutant_align(None, wl, R, t, *run)) == ke.signature(res[run]), (name, run)
