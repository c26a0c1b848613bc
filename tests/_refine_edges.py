"""Workloads at the edges of the pose refit (sgtd_refine_poses, sgtd_amd/csrc/refine_kernels.hip.h): the 896-pair LDS
image, the summation order (256 accumulators, the tree), the two flag halves, the stop rule, the 3 m re-selection and the
3x3 solve.  Plain helper module of tests/test_refine_edges.py (CPU: the workloads reach the edges, against the oracle's
verification and the numpy restatement tests/_refine_ref.py) and tests/test_gpu_refine_edges.py (GPU: every form of the
call equals the restatement on them).

Every scenario is one candidate frame at descriptor level (tests/_verify_edges.py: pair j of the scenario is position j
of the candidate's match list).  The verification takes its hypotheses from the list positions i * skip_len
(skip_len = n / 50 + 1, i < n / skip_len, STDesc.cpp:467-468) and the first hypothesis with the most votes wins, so a
scenario puts a pair of the group that is to win at position 0, or at a sampled position (`sampled`).  A displaced
group is a set of pairs whose table triangle is moved as a whole; an outlier is moved by tens of metres along a
direction of its own, so that no four of them agree.

shell: the probes sit 3 m -+ 1e-3 m and 3 m -+ (1e-6 .. 4e-6) m from the restatement's pose of fit 1 (largest vertex
residual).  The device's pose agrees with numpy's to 1e-9, so both decide these probes alike; nearer
than 1e-6 m is out of scope, because the two SVDs differ in their last bits."""
import numpy as np

import _refine_ref as rr
import _verify_edges as ve

CAP = 896            # SGTD_REFINE_CAP
T0 = np.array([4.0, -6.0, 1.5])


def sampled(n):
    """list positions the verification takes its hypotheses from"""
    skip = n // 50 + 1
    return np.arange(n // skip) * skip


def _far(rng, n):
    """n displacements of 40 m and more, no four of them within metres of each other"""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * (40.0 + 900.0 * rng.random((n, 1)))


def grouped(tag, rng, R, t, n, groups=(), outliers=(), spread=15.0, offset=(0, 0, 0), **info):
    """n rigid pairs (table = f32(R v + t)); groups: (positions, displacement in the table's frame); outliers: positions
    moved far away, each its own way"""
    sc = ve.rigid(tag, rng, R, t, n, offset=offset, n_anchor=n, deltas=[0.0], spread=spread)
    ev = sc.qv @ np.asarray(R).T + np.asarray(t, np.float64)
    for pos, d in groups:
        ev[np.asarray(pos, np.int64)] += np.asarray(d, np.float64)
    out = np.asarray(outliers, np.int64)
    if len(out):
        ev[out] += _far(rng, len(out))[:, None, :]
    sc.ev = ve.f32(ev)
    sc.ec = sc.ev.mean(axis=1)
    sc.info.update(info, outliers=out)
    return sc


def _split(rng, n, sizes):
    """positions 0 .. n-1 dealt at random into groups of the given sizes (the rest: the first group), position 0 in the first"""
    perm = 1 + rng.permutation(n - 1)
    cuts = np.cumsum(sizes[1:])
    parts = np.split(perm[:cuts[-1]], cuts[:-1]) if len(sizes) > 1 else []
    first = np.concatenate([[0], perm[cuts[-1] if len(sizes) > 1 else 0:]])
    assert len(first) == sizes[0]
    return [np.sort(first)] + [np.sort(x) for x in parts]


# ---- cap -------------------------------------------------------------------------------------------------------------
def cap_family():
    rng = np.random.default_rng(101)
    R = ve.ROTATIONS["r37"]
    out = [grouped("cap/all%d" % n, rng, R, T0, n, sizes=[n] * 8, fits=1, stop="same") for n in (CAP - 1, CAP, CAP + 1)]
    # grow: A (exact) and B (+2.9 m in x) vote for each other's hypotheses, C (1.45, 2.9, 0) is more than 3 m from both and
    # less than 3 m from the least-squares shift of A + B (1.45, 0, 0): set 0 = 800, set 1 = 995 (the fit's small rotation
    # leaves five pairs of C out), set 2 = 1000, then unchanged
    a, b, c = _split(rng, 1000, [400, 400, 200])
    out.append(grouped("cap/grow", rng, R, T0, 1000, [(b, (2.9, 0, 0)), (c, (1.45, 2.9, 0))],
                       sizes=[800, 995, 1000], fits=3, stop="same"))
    # shrink: 700 exact, 150 at +2.95 m, 60 at -2.95 m: the fit moves 0.29 m towards the larger group and drops the smaller
    a, b, c = _split(rng, 910, [700, 150, 60])
    out.append(grouped("cap/shrink", rng, R, T0, 910, [(b, (2.95, 0, 0)), (c, (-2.95, 0, 0))],
                       sizes=[910, 850, 850], fits=2, stop="same"))
    # shrink to exactly 896 and grow to exactly 897
    a, b, c = _split(rng, 956, [746, 150, 60])
    out.append(grouped("cap/shrink896", rng, R, T0, 956, [(b, (2.95, 0, 0)), (c, (-2.95, 0, 0))],
                       sizes=[956, 896, 896], fits=2, stop="same"))
    a, b, c = _split(rng, 897, [400, 400, 97])
    out.append(grouped("cap/grow897", rng, R, T0, 897, [(b, (2.9, 0, 0)), (c, (1.45, 2.9, 0))],
                       sizes=[800, 897, 897], fits=2, stop="same"))
    return out


# ---- lanes -----------------------------------------------------------------------------------------------------------
def _sparse(tag, rng, n, inl, **info):
    inl = np.sort(np.asarray(inl, np.int64))
    assert np.intersect1d(inl, sampled(n)).size, tag          # the set's own hypothesis is taken
    mask = np.ones(n, bool)
    mask[inl] = False
    return grouped(tag, rng, ve.ROTATIONS["r37"], T0, n, outliers=np.flatnonzero(mask), inliers=inl,
                   sizes=[len(inl)] * 8, fits=1, stop="same", **info)


def lanes_family():
    rng = np.random.default_rng(202)
    out = [grouped("lanes/all%d" % n, rng, ve.ROTATIONS["r37"], T0, n, sizes=[n] * 8, fits=1, stop="same",
                   inliers=np.arange(n)) for n in (4, 5, 255, 256, 257, 511, 512, 513)]
    out.append(_sparse("lanes/res0", rng, 2049, np.arange(0, 2049, 256)))                       # thread 0 alone: 9 slots
    # residue 255: n = 2520, skip_len 51, position 255 = 5 * 51 is a hypothesis; the last thread alone: 9 slots
    out.append(_sparse("lanes/res255", rng, 2520, np.arange(255, 2520, 256)))
    out.append(_sparse("lanes/one_each", rng, 512, np.arange(256) + 256 * (np.arange(256) % 2)))  # one slot per thread, two rows
    out.append(_sparse("lanes/first", rng, 300, np.arange(4)))
    out.append(_sparse("lanes/last", rng, 300, np.arange(287, 300)))                             # 287 = 41 * 7: the last hypothesis
    out.append(_sparse("lanes/first_one_row", rng, 40, np.arange(5)))
    out.append(_sparse("lanes/last_one_row", rng, 40, np.arange(35, 40)))
    return out


def long_lane():
    """one thread owns 102 slots: a list of 25 900 pairs (skip_len 519), the set = the positions of residue 7 (519 mod 256),
    of which position 519 is a hypothesis.  A table of its own (the keys of tests/_verify_edges.py reach 27 000)."""
    rng = np.random.default_rng(203)
    n = 25900
    return [_sparse("lanes/res7_long", rng, n, np.arange(7, n, 256), owner_slots=102)]


# ---- chain -----------------------------------------------------------------------------------------------------------
def chain_family():
    """chain/noisy: a rigid motion with 1.5 m of noise on every table vertex; the three-point pose of the verification is
    far off, its set small, and the set still changes after eleven fits (n, sigma and seed chosen on the CPU among 72
    combinations for the longest chain; tests/test_refine_edges.py asserts it).  chain/swap: the fit over A + B + D drops
    B (10 pairs) and takes C (10 pairs): a next set of the same size and other members."""
    rng = np.random.default_rng(6)
    R = ve.ROTATIONS["r37"]
    noisy = ve.rigid("chain/noisy", rng, R, T0, 400, n_anchor=400, deltas=[0.0], spread=25.0)
    noisy.ev = ve.f32(noisy.ev + rng.normal(0.0, 1.5, noisy.ev.shape))
    noisy.ec = noisy.ev.mean(axis=1)
    noisy.info["min_fits"] = 8
    rng = np.random.default_rng(303)
    n = 160
    a, b, c, d = _split(rng, n, [100, 10, 10, 40])
    swap = grouped("chain/swap", rng, R, T0, n, [(b, (-2.95, 0, 0)), (c, (3.1, 0, 0)), (d, (1.5, 0, 0))],
                   sizes=[150, 150, 150], fits=2, stop="same", dropped=b, taken=c)
    return [noisy, swap]


# ---- stop ------------------------------------------------------------------------------------------------------------
def _stop_scenario(k, seed):
    """k + 1 pairs within 3 m of pair 0's motion; their least-squares motion leaves the one at -2.9 m out: a next set of
    exactly k pairs (two more pairs far away: a list shorter than 5 pairs is no candidate)"""
    rng = np.random.default_rng(seed)
    n = k + 3
    qv = np.stack([ve.f32(ve._triangle(rng, rng.uniform(-15, 15, 3))) for _ in range(n)])
    shift = np.zeros((n, 3))
    shift[1, 0] = -2.9
    shift[k - 1:k + 1, 0] = 2.9
    shift[k + 1] = [60.0, 40.0, 0]
    shift[k + 2] = [-70.0, 10.0, 5.0]
    return ve.Scenario("stop/next%d" % k, qv, qv + shift[:, None, :], next=k)


def stop_family():
    return [_stop_scenario(k, 1) for k in (3, 4, 5)]      # (seed 1: the first whose residuals all stay 0.2 m off 3 m)


# ---- shell -----------------------------------------------------------------------------------------------------------
SHELL_DELTAS = [1e-3, -1e-3, 2.5e-6, -2.5e-6]      # metres off 3 m


def shell_scenario(oracle, n=120, n_probe=8):
    """56 exact pairs and 56 displaced by 2.9 m in x: set 0 is both groups and fit 1 lies 1.45 m between them.  A probe's
    displaced table vertex sits 3 m + delta from fit 1's pose across x, which is 3.33 m from both groups' hypotheses: no
    probe is in set 0, fit 1 does not depend on where the probes are, and the re-selection under fit 1 decides each at
    3 m + delta.  The vertex is placed in f64 and then moved over the f32 grid (ve.nudge) as near as the grid allows;
    tests/test_refine_edges.py asserts where the probes ended up."""
    rng = np.random.default_rng(404)
    R = ve.ROTATIONS["r37"]
    b = np.arange(1, n - n_probe, 2)
    sc = grouped("shell", rng, R, T0, n, [(b, (2.9, 0, 0))])
    probes = [(n - n_probe + i, i % 3, SHELL_DELTAS[i % len(SHELL_DELTAS)] / 3.0) for i in range(n_probe)]   # (nudge: 3 m * (1 + delta))
    for j, m, _ in probes:
        sc.ev[j, m] += 50.0                              # out of every set until it is placed
    e = cpu_expected(oracle, ve.Workload([sc]), 0, 1)[0]
    assert e["n_pairs"] == n - n_probe
    for i, (j, m, dl) in enumerate(probes):
        x = e["rot"] @ sc.qv[j, m] + e["t"]
        sc.ev[j, m] = ve.f32(x + 3.0 * (1.0 + dl) * np.array([0.0, np.cos(0.8 * i), np.sin(0.8 * i)]))
    sc.info["probes"] = probes
    ve.nudge(sc, np.concatenate([e["rot"].reshape(9), e["t"]])[None], h=-1, reach=6)
    sc.ec = sc.ev.mean(axis=1)
    return sc


def shell_distances(sc, e):
    """largest vertex residual of every probe under the pose of e (a result of the restatement) and its delta"""
    j = np.array([p[0] for p in sc.info["probes"]])
    d = np.sqrt(rr.r2(e["rot"], e["t"], sc.qv[j], sc.ev[j])).max(axis=1)
    return d, 3.0 * np.array([p[2] for p in sc.info["probes"]])


# ---- solve -----------------------------------------------------------------------------------------------------------
WAIVED = ("solve/collinear_x", "solve/identical_collinear_x")      # no pose comparison: H has rank 1
REJECTED = ("lanes/all4", "solve/collinear")                      # never refined (tests/test_refine_edges.py says why)


def solve_family():
    rng = np.random.default_rng(505)
    Rz = ve.ROTATIONS["r37"]
    out = []
    # planar: every vertex at z = 0 on both sides (rotation about z, t_z = 0): H has a zero row and column
    for tag, zn in (("solve/planar", 0.0), ("solve/near_planar", 1e-3)):
        sc = grouped(tag, rng, Rz, (4.0, -6.0, 0.0), 60)
        qv = sc.qv.copy()
        qv[:, :, 2] = rng.normal(0.0, zn, qv.shape[:2]) if zn else 0.0
        sc.qv = ve.f32(qv)
        sc.ev = ve.f32(sc.qv @ Rz.T + np.array([4.0, -6.0, 0.0]))
        sc.qc, sc.ec = sc.qv.mean(axis=1), sc.ev.mean(axis=1)
        sc.info["rank"] = 2 if zn == 0.0 else 3
        out.append(sc)
    # mirror: the table is the query's image under z -> -z (|z| <= 0.5 m, every residual below 3 m): det(H) < 0, so
    # det(V U^T) = -1 for every SVD and the K correction decides the result
    sc = grouped("solve/mirror", rng, np.eye(3), (0, 0, 0), 60)
    qv = sc.qv.copy()
    qv[:, :, 2] = rng.uniform(-0.5, 0.5, qv.shape[:2])
    sc.qv = ve.f32(qv)
    sc.ev = sc.qv * np.array([1.0, 1.0, -1.0])
    sc.qc, sc.ec = sc.qv.mean(axis=1), sc.ev.mean(axis=1)
    sc.info["reflection"] = True
    out.append(sc)
    # collinear: every vertex on one line
    for tag, u in (("solve/collinear", np.array([0.6, 0.8, 0.0])), ("solve/collinear_x", np.array([1.0, 0.0, 0.0]))):
        s = rng.uniform(-20, 20, (24, 3))
        s[:, 1] = s[:, 0] + 3.0 + 2.0 * rng.random(24)
        s[:, 2] = s[:, 1] + 3.0 + 2.0 * rng.random(24)
        qv = s[:, :, None] * u + np.array([1.0, 2.0, 0.5])
        out.append(ve.Scenario(tag, qv, ve.f32(qv) @ Rz.T + T0, rank=1))
    # four identical pairs (a proper triangle: three distinct points, rank 2) and four identical collinear ones
    tri = ve.f32(ve._triangle(rng, np.array([3.0, -2.0, 1.0])))
    qv = np.concatenate([np.repeat(tri[None], 4, axis=0), np.stack([ve._triangle(rng, rng.uniform(-15, 15, 3)) for _ in range(2)])])
    ev = ve.f32(qv) @ Rz.T + T0
    ev[4] += [60.0, 40.0, 0.0]
    ev[5] += [-70.0, 10.0, 5.0]
    out.append(ve.Scenario("solve/identical", qv, ev, rank=2))
    line = np.array([[0.0, 0, 0], [5.0, 0, 0], [11.0, 0, 0]]) + np.array([1.0, 1.0, 1.0])
    qv = np.concatenate([np.repeat(line[None], 4, axis=0), qv[4:]])
    ev = ve.f32(qv) @ Rz.T + T0
    ev[4] += [60.0, 40.0, 0.0]
    ev[5] += [-70.0, 10.0, 5.0]
    out.append(ve.Scenario("solve/identical_collinear_x", qv, ev, rank=1))
    # far from the origin: f32 vertex spacing 1e-3 m at 1e4 m
    out.append(grouped("solve/far", rng, ve.ROTATIONS["r1e-3"], (1.5, -2.0, 0.5), 300, offset=(1e4, -2e4, 50.0), spread=10.0, rank=3))
    out.append(grouped("solve/r179.9", rng, ve.rotation((1, 1, 0.2), np.deg2rad(179.9)), T0, 80, rank=3))
    return out


# ---- mix -------------------------------------------------------------------------------------------------------------
def mix_family():
    """live and rejected candidates in turn (a rejected one: no four pairs agree, score -1); the query's slots past n_cand
    are the rest of candidate_num"""
    rng = np.random.default_rng(606)
    out = []
    for i, n in enumerate((1000, 500, 300, 100, 70, 40, 30)):      # candidates stand by votes: this is their slot order
        if i % 2 == 0:
            out.append(grouped("mix/live%d" % i, rng, ve.ROTATIONS["r37"], T0, n, live=True))
        else:
            out.append(ve.votes_exactly("mix/dead%d" % i, rng, 3, n=n))
    return out


FAMILIES = {"cap": cap_family, "lanes": lanes_family, "chain": chain_family, "stop": stop_family, "solve": solve_family,
            "mix": mix_family}


def all_scenarios(oracle):
    """the suite's scenarios but the long list -> {family: [Scenario]}"""
    out = {name: f() for name, f in FAMILIES.items()}
    out["shell"] = [shell_scenario(oracle)]
    return out


def workload(fams):
    """one table of every family's scenarios, a query per family"""
    scen, queries = [], []
    for name, sc in fams.items():
        queries.append(list(range(len(scen), len(scen) + len(sc))))
        scen += sc
    wl = ve.Workload(scen)
    wl.queries = queries
    wl.family = list(fams)
    return wl


# ---- the restatement on a workload -------------------------------------------------------------------------------
def cpu_expected(oracle, wl, qi, iterations, o=None, refine=rr.refine):
    """OracleManager.verify + the restatement for every candidate of query qi -> {k: result + p, w, set0, tag, score}
    (candidates the verification rejects: no entry); o: a loaded OracleManager to reuse"""
    if o is None:
        o = oracle.OracleManager()
        wl.load(o, oracle)
    qd = wl.query_descs(oracle, qi)
    sel = o.select(qd)
    out = {}
    for k in range(len(sel["cand_frame"])):
        lo, hi = int(sel["cand_off"][k]), int(sel["cand_off"][k + 1])
        score, t, rot, idx = o.verify(k, hi - lo)
        if score < 0:
            continue
        s0 = np.zeros(hi - lo, bool)
        s0[idx] = True
        ent = o.fetch_entries(sel["db_entry"][lo:hi])
        p, w = rr.correspondences(qd.vertex, sel["q_idx"][lo:hi], ent.vertex)
        sc = wl.scen[int(sel["cand_frame"][k])]
        e = refine(p, w, s0, iterations, rot, t)
        out[k] = dict(e, p=p, w=w, set0=s0, tag=sc.tag, score=score, v_rot=rot, v_t=t, frame=int(sel["cand_frame"][k]),
                      q_idx=sel["q_idx"][lo:hi] - (int(wl.key0[int(sel["cand_frame"][k])]) - int(wl.key0[wl.queries[qi][0]])))
    out["n_cand"] = len(sel["cand_frame"])
    out["cand_frame"] = sel["cand_frame"]
    return out


def trace(p, w, set0, iterations):
    """the sets the rule fits, one after the other -> [bool [n_list]] (fit 1's first)"""
    cur = np.asarray(set0, bool)
    sets = []
    for it in range(1, iterations + 1):
        sets.append(cur)
        _, cp, cw, H = rr.moments(p, w, cur)
        R = rr.kabsch(H)
        nxt = rr.reselect(R, rr.translation(R, cp, cw), p, w)
        if it == iterations or np.count_nonzero(nxt) < rr.MIN_PAIRS or np.array_equal(nxt, cur):
            break
        cur = nxt
    return sets
