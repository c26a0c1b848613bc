"""The pose refit's edge workloads (tests/_refine_edges.py) on the CPU: OracleManager.verify gives set 0 and the
verification's pose, the numpy restatement (tests/_refine_ref.py) the refit.  Asserted here: every family reaches the
edge it is built for; ordered_sum equals the plain loop on the lane lists; every mutant of the restatement is caught by
a named case.  The GPU file (tests/test_gpu_refine_edges.py) compares the device with the same restatement on the same
workloads.

Not reachable as first stated, and asserted as such below:
  * a list of 4 pairs: candidate_selector takes a frame from 5 votes on (STDesc.cpp:417), the shortest list has 5 pairs;
  * a collinear set along a general direction: the verification's own hypotheses come from the same 3x3 solver, whose
    completion of a rank-1 U is orthogonal only for a line along x; along any other line no hypothesis gets 4 votes and
    the candidate is rejected before the refit.  The collinear sets that reach the refit lie along x;
  * one thread owning 100 slots needs a list of 25 600 pairs and more: lanes/res7_long has a table of its own.
A skipped pair added as +0.0 is NOT visible: an accumulator starts at +0.0 and can only become -0.0 by adding -0.0 to
-0.0, and x + 0.0 == x bit for bit for every other x; test_zero_add_is_equivalent shows it on every lane list."""
import numpy as np
import pytest

import _refine_edges as re_
import _refine_ref as rr
import _verify_edges as ve

IT = 8


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def case(oracle_mod):
    fams = re_.all_scenarios(oracle_mod)
    wl = re_.workload(fams)
    o = oracle_mod.OracleManager()
    wl.load(o, oracle_mod)
    exp = {}
    for qi, name in enumerate(wl.family):
        ex = re_.cpu_expected(oracle_mod, wl, qi, IT, o=o)
        assert ex["n_cand"] == len(fams[name]) - sum(s.tag == "lanes/all4" for s in fams[name]), name
        for k, e in ex.items():
            if isinstance(k, int):
                assert np.array_equal(e["q_idx"], np.arange(len(e["p"]))), e["tag"]       # list position = scenario pair
                e["k"] = k
                e["sets"] = re_.trace(e["p"], e["w"], e["set0"], IT)
                exp[e["tag"]] = e
    return fams, wl, exp


def _sizes(e):
    return [int(s.sum()) for s in e["sets"]]


# ---- reach -----------------------------------------------------------------------------------------------------------
def test_reach_cap(case):
    _, _, exp = case
    for n in (895, 896, 897):
        e = exp["cap/all%d" % n]
        assert _sizes(e) == [n] and e["stop"] == "same" and e["fits"] == 1
    assert _sizes(exp["cap/grow"]) == [800, 995, 1000] and exp["cap/grow"]["stop"] == "same"     # gathered from LDS, then per pass twice
    assert _sizes(exp["cap/grow897"]) == [800, 897] and exp["cap/grow897"]["stop"] == "same"      # LDS, then the smallest set beyond it; falls back there
    assert _sizes(exp["cap/shrink"]) == [910, 850] and exp["cap/shrink"]["stop"] == "same"        # per pass, then LDS; falls back there
    assert _sizes(exp["cap/shrink896"]) == [956, 896] and exp["cap/shrink896"]["stop"] == "same"  # the largest set that fits
    for tag in ("cap/grow", "cap/grow897", "cap/shrink", "cap/shrink896"):
        s = _sizes(exp[tag])
        assert (s[0] <= re_.CAP) != (s[1] <= re_.CAP), tag                                      # crosses between fit 1 and fit 2


def test_reach_lanes(case, oracle_mod):
    fams, _, exp = case
    assert "lanes/all4" not in exp                    # 4 votes: no candidate (reported in the module docstring)
    for n in (5, 255, 256, 257, 511, 512, 513):
        assert _sizes(exp["lanes/all%d" % n]) == [n]
    for sc in fams["lanes"]:
        if sc.tag == "lanes/all4":
            continue
        e = exp[sc.tag]
        assert np.array_equal(np.flatnonzero(e["set"]), sc.info["inliers"]) and e["fits"] == 1 and e["stop"] == "same", sc.tag
    res = lambda tag: set(np.flatnonzero(exp[tag]["set"]) % 256)
    assert res("lanes/res0") == {0} and res("lanes/res255") == {255} and exp["lanes/res0"]["n_pairs"] == 9
    pos = np.flatnonzero(exp["lanes/one_each"]["set"])
    assert sorted(pos % 256) == list(range(256)) and set(pos // 256) == {0, 1}
    assert np.flatnonzero(exp["lanes/first"]["set"]).tolist() == [0, 1, 2, 3]
    assert np.flatnonzero(exp["lanes/last"]["set"]).tolist() == list(range(287, 300))


def test_reach_long_lane(oracle_mod):
    sc = re_.long_lane()[0]
    e = re_.cpu_expected(oracle_mod, ve.Workload([sc]), 0, 2)[0]
    pos = np.flatnonzero(e["set"])
    assert set(pos % 256) == {7} and len(pos) == sc.info["owner_slots"] == 102 and e["stop"] == "same"
    a, b = rr.ordered_sum(e["p"], e["set"]), rr.ordered_sum_loop(e["p"], e["set"])
    assert np.array_equal(_bits(a), _bits(b))


def test_reach_chain(case):
    _, _, exp = case
    e = exp["chain/noisy"]
    assert e["fits"] == IT and e["stop"] is None and len(e["sets"]) == IT         # stops on `iterations` alone
    assert all(not np.array_equal(a, b) for a, b in zip(e["sets"], e["sets"][1:]))
    same_size = [i for i in range(IT - 1) if e["sets"][i].sum() == e["sets"][i + 1].sum()]
    assert same_size                                                               # (and one step keeps the size: 146 -> 146)
    e = exp["chain/swap"]
    assert _sizes(e) == [150, 150] and not np.array_equal(e["sets"][0], e["sets"][1]) and e["fits"] == 2 and e["stop"] == "same"


def test_reach_stop(case):
    _, _, exp = case
    assert (_sizes(exp["stop/next3"]), exp["stop/next3"]["stop"], exp["stop/next3"]["n_pairs"]) == ([4], "few", 4)
    e = exp["stop/next3"]
    R = rr.kabsch(e["H"])
    assert rr.reselect(R, rr.translation(R, e["cp"], e["cw"]), e["p"], e["w"]).sum() == 3
    assert (_sizes(exp["stop/next4"]), exp["stop/next4"]["stop"]) == ([5, 4], "same")
    assert (_sizes(exp["stop/next5"]), exp["stop/next5"]["stop"]) == ([6, 5], "same")


def test_reach_shell(case):
    fams, _, exp = case
    sc, e = fams["shell"][0], exp["shell"]
    j = np.array([p[0] for p in sc.info["probes"]])
    assert not e["sets"][0][j].any()                                   # no probe in set 0: fit 1 does not depend on them
    _, cp, cw, H = rr.moments(e["p"], e["w"], e["sets"][0])
    R = rr.kabsch(H)
    d, dl = re_.shell_distances(sc, dict(rot=R, t=rr.translation(R, cp, cw)))
    print("shell: residual - 3 m", d - 3.0)
    for x, want in zip(d - 3.0, dl):
        if abs(want) >= 1e-4:
            assert abs(x - want) <= 1e-5
        else:
            assert 1e-6 <= abs(x) <= 4e-6 and np.sign(x) == np.sign(want)
    assert np.array_equal(e["sets"][1][j], dl < 0) and _sizes(e)[:2] == [112, 116]


def test_reach_solve(case):
    fams, _, exp = case
    assert "solve/collinear" not in exp               # rejected by the verification (module docstring)
    ranks = {}
    for sc in fams["solve"]:
        if sc.tag in re_.REJECTED:
            continue
        s = np.linalg.svd(exp[sc.tag]["H"], compute_uv=False)
        ranks[sc.tag] = int((s > 1e-12 * s[0]).sum())
        if "rank" in sc.info:
            assert ranks[sc.tag] == sc.info["rank"], sc.tag
    H = exp["solve/planar"]["H"]
    assert not H[2].any() and not H[:, 2].any()                        # a zero row and column
    # reflections before the correction: det(H) < 0 gives det(V U^T) = -1 whatever the SVD
    refl = [tag for tag, e in exp.items() if np.linalg.det(e["H"]) < 0 and np.linalg.svd(e["H"], compute_uv=False)[2] > 1e-9 * np.abs(e["H"]).max()]
    assert "solve/mirror" in refl
    e = exp["solve/far"]
    assert np.linalg.norm(e["cp"]) > 2e4 and np.spacing(np.float32(2e4)) > 1e-3
    assert np.degrees(np.arccos((np.trace(exp["solve/r179.9"]["rot"]) - 1) / 2)) > 179.89


def test_reach_mix(case):
    fams, wl, exp = case
    live = [sc.tag in exp for sc in fams["mix"]]
    assert live == [True, False] * 3 + [True]
    assert [exp[sc.tag]["k"] for sc in fams["mix"][::2]] == [0, 2, 4, 6]          # interleaved in slot order


def test_second_singular_value(case):
    """every scenario but the waived ones has a well-posed rotation: H's second singular value is at least 1e-3 of its first"""
    _, _, exp = case
    for tag, e in exp.items():
        s = np.linalg.svd(e["H"], compute_uv=False)
        if tag in re_.WAIVED:
            assert s[1] < 1e-6 * s[0], tag
        else:
            assert s[1] >= 1e-3 * s[0], tag
            R = e["rot"]
            assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0, tag


# ---- consistency -----------------------------------------------------------------------------------------------------
def test_ordered_sum_equals_the_loop_on_the_lane_lists(case):
    fams, _, exp = case
    for sc in fams["lanes"] + fams["cap"][:3]:
        if sc.tag in exp:
            e = exp[sc.tag]
            terms = (e["p"] - e["cp"])[:, :, :, None] * (e["w"] - e["cw"])[:, :, None, :]
            assert np.array_equal(_bits(rr.ordered_sum(terms, e["set"])), _bits(rr.ordered_sum_loop(terms, e["set"]))), sc.tag


# ---- mutants of the restatement --------------------------------------------------------------------------------------
def _msum(terms, in_set, mut):
    terms = np.asarray(terms, np.float64)
    n = terms.shape[0]
    rows = -(-n // 256)
    acc = np.zeros((256,) + terms.shape[2:])
    for j in range(n):
        if not in_set[j]:
            if mut == "zero_add":
                l = j % 256
                for a in range(3):
                    acc[l] = acc[l] + 0.0
            continue
        l = j // rows if mut == "acc_rows" else j % 256
        for a in range(3):
            acc[l] = acc[l] + terms[j, a]
    if mut == "tree_order":                      # the s = 64 level before the s = 128 level
        for lo in (0, 128):
            acc[lo:lo + 64] = acc[lo:lo + 64] + acc[lo + 64:lo + 128]
        acc[:64] = acc[:64] + acc[128:192]
        levels = (32, 16, 8, 4, 2, 1)
    else:
        levels = (128, 64, 32, 16, 8, 4, 2, 1)
    for s in levels:
        acc[:s] = acc[:s] + acc[s:2 * s]
    return acc[0].copy()


def _mrefine(p, w, set0, iterations, vR, vt, mut=None):
    cur = np.asarray(set0, bool).copy()
    fits, it = 0, 1
    while True:
        n = int(cur.sum())
        d = np.float64(3 * n)
        cset = np.ones(len(cur), bool) if mut == "whole_list" else cur
        cp, cw = _msum(p, cset, mut) / (np.float64(3 * len(cur)) if mut == "whole_list" else d), _msum(w, cset, mut) / (np.float64(3 * len(cur)) if mut == "whole_list" else d)
        H = _msum((p - cp)[:, :, :, None] * (w - cw)[:, :, None, :], cur, mut)
        if mut == "no_K":
            U, _, Vt = np.linalg.svd(H)
            R = Vt.T @ U.T
        else:
            R = rr.kabsch(H)
        t = rr.translation(R, cp, cw)
        fits += 1
        if it >= iterations:
            break
        r2 = rr.r2(R, t, p, w)
        nxt = np.all(r2 <= rr.THR2, axis=1) if mut == "le" else np.all(r2 < rr.THR2, axis=1)
        lo = {"lt5": 5, "lt3": 3}.get(mut, 4)
        if nxt.sum() < lo:
            if mut == "new_count":
                n = int(nxt.sum())
            break
        same = nxt.sum() == cur.sum() if mut == "by_count" else np.array_equal(nxt, cur)
        if mut == "one_half" and it >= 2:
            same = True                          # the next set written over the current one: no flag is seen to change
        if same:
            if mut == "new_count":
                n = int(nxt.sum())
            break
        cur = nxt
        it += 1
    ss = _msum(rr.r2(R, t, p, w), cur, mut)
    return dict(rot=R, t=t, n_pairs=n, moments=np.concatenate([cp, cw, H.reshape(9)]), rmse=np.sqrt(ss / np.float64(3 * cur.sum())), fits=fits)


def _differs(a, e):
    return (a["n_pairs"] != e["n_pairs"] or not np.array_equal(_bits(a["moments"]), _bits(e["moments"]))
            or np.abs(a["rot"] - e["rot"]).max() > 1e-9 or np.linalg.det(a["rot"]) < 0)


MUTANTS = [("tree_order", "lanes/all256"), ("tree_order", "lanes/all513"), ("acc_rows", "lanes/all257"), ("acc_rows", "lanes/res255"),
           ("lt5", "stop/next4"), ("lt3", "stop/next3"), ("by_count", "chain/swap"), ("le", "exact9"), ("one_half", "chain/noisy"),
           ("new_count", "stop/next3"), ("no_K", "solve/mirror"), ("whole_list", "lanes/first"),
           ("whole_list", "lanes/one_each")]


@pytest.mark.parametrize("mut, tag", MUTANTS)
def test_mutant_is_caught(case, mut, tag):
    _, _, exp = case
    if mut == "le":
        # r2 == 9.0 exactly: a vertex 3 m off along x under the identity (integers: every operation is exact); the rule
        # leaves the pair out, `<=` takes it
        p = np.array([[[1.0, 1, 1], [5, 1, 0], [1, 5, 2]]])
        w = p.copy()
        w[0, 0, 0] += 3.0
        r2 = rr.r2(np.eye(3), np.zeros(3), p, w)
        assert r2[0, 0] == 9.0 and not rr.reselect(np.eye(3), np.zeros(3), p, w)[0] and np.all(r2 <= rr.THR2)
        return
    e = exp[tag]
    same = _mrefine(e["p"], e["w"], e["set0"], IT, e["v_rot"], e["v_t"])
    assert not _differs(same, e) and same["fits"] == e["fits"] and np.array_equal(_bits(same["rmse"]), _bits(e["rmse"]))   # the copy itself is right
    assert _differs(_mrefine(e["p"], e["w"], e["set0"], IT, e["v_rot"], e["v_t"], mut), e), (mut, tag)


def test_zero_add_is_equivalent(case):
    fams, _, exp = case
    for sc in fams["lanes"]:
        if sc.tag in exp:
            e = exp[sc.tag]
            m = _mrefine(e["p"], e["w"], e["set0"], 1, e["v_rot"], e["v_t"], "zero_add")
            assert np.array_equal(_bits(m["moments"]), _bits(rr.refine(e["p"], e["w"], e["set0"], 1, e["v_rot"], e["v_t"])["moments"])), sc.tag
