"""Workloads at the edges of candidate_verify's vote pass (STDesc.cpp:462-547): the 3 m threshold, the gates of the
matrix-core form (sgtd_amd/csrc/verify_mfma.hip.h) and the selection rules.  Plain helper module of
tests/test_verify_edges.py (CPU: the workloads reach the edges) and tests/test_gpu_verify_edges.py (GPU: every dispatch
form equals the oracle on them).

Descriptor scenarios.  A scenario is one candidate frame: n (query triangle, table triangle) pairs.  Selection only looks
at sides and labels, verification only at vertices and centres, so every pair gets a (side, label) key of its own that the
query descriptor and the table entry share exactly: candidate_selector pairs query descriptor j with table entry j of the
scenario's frame and nothing else, and the candidate's match list is the scenario's pairs in order.  Vertices are float32
(the engine stores f32 vertices; the oracle gets the same values in f64), centres are f64.

Frame batch.  Query frames that are rigid images of map frames with clusters of keypoints moved as a whole by
3 m * (1 + delta): triangles inside a cluster keep their sides (selection pairs them) and sit near the threshold under the
global motion.  96 query frames x candidate_num 50 >= 4096: query_frames + verify take verify_mfma_kernel<4> and the
frame-ordered dispatch.
"""
import numpy as np

THR = 3.0
ULP3 = 2.0 ** -51                     # spacing of the doubles in [2, 4)
# delta ladder: 0, a few f64 ulps of 3 m, and the decades 1e-15 ... 1e-1, both signs
LADDER = [0.0, ULP3 / 3, 2 * ULP3 / 3, 5 * ULP3 / 3] + [10.0 ** -e for e in range(15, 0, -1)]
LADDER = LADDER + [-d for d in LADDER[1:]]
DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1],
                 [0.6, 0.8, 0], [0.36, 0.48, 0.8], [-0.48, 0.36, -0.8], [0, -0.8, 0.6]], np.float64)
DIRS /= np.linalg.norm(DIRS, axis=1, keepdims=True)
N_LABEL = 15 ** 3                     # label triples (1..15)^3 per side triple
QUERY_FRAME = 19000                   # frame id of the query descriptors (never a table frame)


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


ROTATIONS = {"r0": np.eye(3), "r1e-3": rotation((0.3, 0.5, 0.8), 1e-3), "r37": rotation((0, 0, 1), 0.65),
             "r90": rotation((0, 0, 1), np.pi / 2), "r180": rotation((1, 1, 0.2), np.pi - 1e-4)}


def key_of(k):
    """(side, label) of key k: label triples in 1..15, side triples 3 m apart in x (the 27 cells selection probes around
    one side never reach another's)"""
    lab = (1 + k % 15, 1 + (k // 15) % 15, 1 + (k // 225) % 15)
    j = k // N_LABEL
    assert j < 8
    return (4.25 + 3.0 * j, 30.25, 45.25), lab


def vertex_dists(rt, v, w):
    """|R v + t - w| per vertex exactly as the reference evaluates it (row sums left to right plus t, then
    sqrt((dx^2 + dy^2) + dz^2)): rt [.., 12] (R row-major, t), v / w [.., 3, 3] -> [.., 3]"""
    R, t = rt[..., :9], rt[..., 9:]
    d2 = 0.0
    for r in range(3):
        p = ((R[..., None, 3 * r] * v[..., 0] + R[..., None, 3 * r + 1] * v[..., 1]) + R[..., None, 3 * r + 2] * v[..., 2]) + t[..., None, r]
        d = p - w[..., r]
        d2 = d * d if r == 0 else d2 + d * d
    return np.sqrt(d2)


class Scenario:
    """one candidate frame: qv / ev [n, 3, 3] (f32 values), centres [n, 3] f64 (default: the vertices' mean)"""

    def __init__(self, tag, qv, ev, qc=None, ec=None, **info):
        self.tag = tag
        self.qv, self.ev = f32(qv), f32(ev)
        self.qc = self.qv.mean(axis=1) if qc is None else np.asarray(qc, np.float64)
        self.ec = np.where(np.isfinite(self.ev), self.ev, 0.0).mean(axis=1) if ec is None else np.asarray(ec, np.float64)
        self.info = info
        self.n = len(self.qv)


class Workload:
    """scenarios (frame f = scenario f) grouped into queries of at most `per_query` candidates"""

    def __init__(self, scenarios, per_query=40):
        self.scen = list(scenarios)
        self.key0 = np.cumsum([0] + [s.n for s in self.scen])
        self.queries = [list(range(i, min(i + per_query, len(self.scen)))) for i in range(0, len(self.scen), per_query)]

    def _descs(self, mod, items):
        n = sum(len(js) for _, js in items)
        d = mod.Descs(n)
        i = 0
        for s, js in items:
            sc = self.scen[s]
            for j in js:
                side, lab = key_of(int(self.key0[s]) + j)
                d.side[i] = side
                d.label[i] = lab
                i += 1
        return d

    def table_descs(self, mod, s):
        sc = self.scen[s]
        d = self._descs(mod, [(s, range(sc.n))])
        d.vertex[:] = sc.ev.reshape(sc.n, 9)
        d.center[:] = sc.ec
        d.frame[:] = s
        return d

    def query_descs(self, mod, qi):
        items = [(s, range(self.scen[s].n)) for s in self.queries[qi]]
        d = self._descs(mod, items)
        d.vertex[:] = np.concatenate([self.scen[s].qv.reshape(-1, 9) for s in self.queries[qi]])
        d.center[:] = np.concatenate([self.scen[s].qc for s in self.queries[qi]])
        d.frame[:] = QUERY_FRAME
        return d

    def load(self, mgr, mod):
        """one AddSTDescs per scenario frame (frame ids 0, 1, ...) into an STDescManager or an OracleManager"""
        for s in range(len(self.scen)):
            d = self.table_descs(mod, s)
            mgr.add(d) if hasattr(mgr, "add") else mgr.AddSTDescs(d)


# ---- scenario builders -------------------------------------------------------------------------------------------
def _triangle(rng, centre, size=8.0):
    while True:
        v = centre + rng.uniform(-size, size, (3, 3))
        s = [np.linalg.norm(v[a] - v[b]) for a, b in ((0, 1), (1, 2), (0, 2))]
        if min(s) > 2.0:
            return v


def rigid(tag, rng, R, t, n, offset=(0, 0, 0), n_anchor=6, deltas=LADDER, spread=15.0, m_cycle=3, **info):
    """n pairs: n_anchor anchors (table = f32(R v + t)), the rest probes (one vertex further moved by 3 m (1 + delta) along
    a direction of DIRS); query vertices within `spread` of `offset`"""
    off = np.asarray(offset, np.float64)
    qv = np.zeros((n, 3, 3))
    ev = np.zeros((n, 3, 3))
    probe = []
    for j in range(n):
        v = f32(_triangle(rng, off + rng.uniform(-spread, spread, 3)))
        w = v @ R.T + t
        if j >= n_anchor:
            k = j - n_anchor
            m, u, dl = k % m_cycle, DIRS[k % len(DIRS)], deltas[(k // len(DIRS) + k) % len(deltas)]
            w[m] = w[m] + THR * (1.0 + dl) * (u @ R.T)
            probe.append((j, m, dl))
        qv[j], ev[j] = v, f32(w)
    return Scenario(tag, qv, ev, R=R, t=np.asarray(t, np.float64), offset=off, probes=probe, **info)


def exact_axis(tag, rng, n, n_anchor=5, deltas=LADDER):
    """R = I and t = 0 EXACTLY for every anchor hypothesis (planar, mirror-symmetric anchor triangles: the covariance is
    diagonal, the Jacobi SVD does no rotation), probes moved along a coordinate axis by a tiny query coordinate, so that
    |d| = 3 + (a few ulps) or exactly 3 (d^2 = 9.0: the `<` of the reference)"""
    qv = np.zeros((n, 3, 3))
    probe = []
    for j in range(n):
        if j < n_anchor:
            c = rng.integers(-12, 12, 3).astype(np.float64)
            a, b = 1.0 + 0.5 * (j % 4), 2.0 + 0.25 * j
            qv[j] = c + np.array([[a, b, 0], [-a, b, 0], [0, -2 * b, 0]])
        else:
            qv[j] = rng.integers(-10, 10, (3, 3)).astype(np.float64)
            while min(np.linalg.norm(qv[j][a] - qv[j][b]) for a, b in ((0, 1), (1, 2), (0, 2))) < 2:
                qv[j] = rng.integers(-10, 10, (3, 3)).astype(np.float64)
    ev = qv.copy()
    for j in range(n_anchor, n):
        k = j - n_anchor
        m, ax, sg = k % 3, (k // 3) % 3, 1.0 if (k // 9) % 2 == 0 else -1.0
        dl = deltas[k % len(deltas)]
        qv[j][m][ax] = np.float32(THR * dl)        # tiny (or 0): exact in f32
        ev[j][m][ax] = -sg * THR                    # |d| = |3 delta + 3 sg|
        probe.append((j, m, dl))
    return Scenario(tag, qv, ev, R=np.eye(3), t=np.zeros(3), probes=probe, exact=True)


def degenerate(tag, rng, n=12):
    """hypotheses from collinear and coincident-vertex triangles (rank-1 covariance: the completed U is not orthogonal,
    the rotation's orthogonality defect crosses the 1e-6 gate) among ordinary rigid pairs"""
    sc = rigid(tag, rng, ROTATIONS["r37"], np.array([3.0, -2.0, 1.0]), n, n_anchor=n, deltas=[0.0])
    for j in range(0, n, 2):
        v = sc.qv[j].copy()
        if j % 4 == 0:
            v[2] = v[0] + 2.0 * (v[1] - v[0])          # collinear
        else:
            v[1] = v[0]                                # coincident
        if j % 8 >= 4:
            v[2] += 1e-4                               # near-collinear / near-coincident
        sc.qv[j] = f32(v)
        sc.ev[j] = f32(sc.qv[j] @ sc.info["R"].T + sc.info["t"])
    sc.qc = sc.qv.mean(axis=1)
    sc.ec = sc.ev.mean(axis=1)
    return sc


def votes_exactly(tag, rng, n_agree, n=6):
    """n_agree pairs follow one motion, the other n - n_agree each a motion of their own: the best hypothesis has
    exactly n_agree votes (4: accepted, 3: rejected, :515)"""
    R, t = ROTATIONS["r37"], np.array([5.0, 1.0, -2.0])
    sc = rigid(tag, rng, R, t, n, n_anchor=n, deltas=[0.0])
    for j in range(n_agree, n):
        R2 = rotation(rng.normal(size=3), 1.0 + j)
        sc.ev[j] = f32(sc.qv[j] @ R2.T + rng.uniform(-60, 60, 3))
    sc.ec = sc.ev.mean(axis=1)
    sc.info["n_agree"] = n_agree
    return sc


def nudge(scen, hyps, h=0, reach=4):
    """move every probe's displaced table vertex over the f32 grid (+-reach ulps per coordinate) so that its f64 distance
    under hypothesis h of the oracle (hyps [use_size, 12], verify_hyp_solutions) is as close as the grid allows to
    3 m (1 + delta)"""
    steps = np.arange(-reach, reach + 1)
    for j, m, dl in scen.info.get("probes", []):
        if scen.info.get("exact") or j == h:
            continue
        w0 = scen.ev[j, m].astype(np.float32)
        grid = []
        for c in range(3):
            x = np.full(len(steps), w0[c], np.float32)
            for i, s in enumerate(steps):
                for _ in range(abs(s)):
                    x[i] = np.nextafter(x[i], np.float32(np.inf if s > 0 else -np.inf))
            grid.append(x.astype(np.float64))
        W = np.stack(np.meshgrid(*grid, indexing="ij"), axis=-1).reshape(-1, 3)
        ev = np.repeat(scen.ev[j][None], len(W), axis=0)
        ev[:, m] = W
        d = vertex_dists(hyps[h], np.repeat(scen.qv[j][None], len(W), axis=0), ev)[:, m]
        best = int(np.argmin(np.abs(d - THR * (1.0 + dl))))
        scen.ev[j, m] = W[best]


def descriptor_workload(oracle, seed=7):
    """the descriptor scenarios: rotations x list lengths, the exact-axis ladder, selection edges, degenerate hypotheses,
    nudged onto the oracle's own hypotheses"""
    rng = np.random.default_rng(seed)
    sc = []
    lengths = [5, 6, 31, 32, 33, 49, 50, 51, 64, 65]
    for i, (name, R) in enumerate(ROTATIONS.items()):
        t = np.array([12.25, -7.5, 2.0]) if i % 2 else np.array([-3.0, 20.5, -1.25])
        for n in lengths:
            sc.append(rigid("rigid/%s/n%d" % (name, n), rng, R, t, n, n_anchor=min(6, n), rotation=name))
    for n in (33, 49, 65, 96, 130):
        sc.append(exact_axis("exact/n%d" % n, rng, n))
    sc.append(degenerate("degenerate", rng))
    sc.append(votes_exactly("votes4", rng, 4))
    sc.append(votes_exactly("votes3", rng, 3))
    sc.append(votes_exactly("votes4of5", rng, 4, n=5))
    # two hypotheses tied by near-edge decisions: two anchors, probes at the ulp level of the f32 grid
    sc.append(rigid("tie", rng, ROTATIONS["r1e-3"], np.array([0.5, 0.25, -0.5]), 24, n_anchor=3,
                    deltas=[1e-7, -1e-7, 3e-7, -3e-7, 0.0]))
    # >= 1000 pairs: skip_len 21, two hypothesis tiles, a tail tile; everything inside the band at 1 km (queue drains)
    sc.append(rigid("long/n1000", rng, ROTATIONS["r37"], np.array([4.0, -6.0, 1.5]), 1000, n_anchor=1000,
                    deltas=[0.0], spread=4.0))
    sc.append(rigid("long/n1003/km", rng, ROTATIONS["r1e-3"], np.array([2.0, 1.0, 0.5]), 1003, offset=(1e3, -1e3, 50),
                    n_anchor=200, spread=4.0))
    sc += scale_ladder(rng)
    _nudge_all(oracle, sc)
    return Workload(sc)


def scale_ladder(rng):
    """query and table vertices about 0 ... 9e5 m from the origin (the scale s of the pair features down to 2^-24 and
    below), |t|_1 just below and above 1e5, table entries with a coordinate >= 1e6, NaN and inf"""
    out = []
    for off in (0.0, 1e2, 1e3, 1e4, 2e5, 9e5):
        o = np.array([off, -0.7 * off, 0.01 * off])
        for name in ("r1e-3", "r37"):
            out.append(rigid("scale/%g/%s" % (off, name), rng, ROTATIONS[name], np.array([1.5, -2.0, 0.5]), 40, offset=o,
                             n_anchor=8, rotation=name, scale=off))
    for tl in (0.999e5, 1.001e5):
        t = np.array([0.5, 0.3, 0.2]) * tl
        out.append(rigid("t1/%g" % tl, rng, ROTATIONS["r1e-3"], t, 40, n_anchor=8, t1=tl))
    # one hypothesis with |t|_1 beyond 1e5 among small ones (pairs whose table triangle sits 1e5 m away)
    sc = rigid("t1/mixed", rng, ROTATIONS["r0"], np.array([1.0, 2.0, 3.0]), 40, n_anchor=20)
    sc.ev[3] = f32(sc.ev[3] + np.array([6e4, 3e4, 2e4]))
    sc.ec[3] = sc.ev[3].mean(axis=0)
    out.append(sc)
    # wild pairs at odd list positions (skip_len 2: never a hypothesis) — the per-pair gate, not the candidate's
    for name, val in (("1e6", 1.0e6), ("2e6", -2.0e6), ("nan", np.nan), ("inf", np.inf)):
        sc = rigid("wild/%s" % name, rng, ROTATIONS["r37"], np.array([2.0, 2.0, 2.0]), 64, n_anchor=16)
        for j in (1, 17, 33, 63):
            sc.ev[j, j % 3, j % 2] = val
        sc.info["wild"] = [1, 17, 33, 63]
        out.append(sc)
    return out


def _nudge_all(oracle, scens):
    """the oracle's own hypotheses of every scenario (a table of its frame alone), then the probes moved onto them"""
    for scen in scens:
        if scen.info.get("exact") or not scen.info.get("probes"):
            continue
        wl = Workload([scen])
        o = oracle.OracleManager()
        wl.load(o, oracle)
        o.select(wl.query_descs(oracle, 0))
        nudge(scen, o.verify_hyp_solutions(0))


# ---- the frame batch -------------------------------------------------------------------------------------------------
def frame_batch(synth, n_map=60, n_kp=120, n_q=96, seed=11):
    """map (synth) + n_q query frames: rigid images (query -> map: R, t) of map frames with two clusters of 12 keypoints
    each moved by 3 m (1 + delta) as a whole"""
    m = synth.make_map(n_map, n_kp, stream=seed)
    rng = np.random.default_rng(seed)
    qx = np.zeros((n_q, n_kp, 3), np.float32)
    ql = np.zeros((n_q, n_kp), np.uint32)
    info = []
    for q in range(n_q):
        f = int(rng.integers(0, n_map))
        R = rotation((0.05 * rng.normal(), 0.05 * rng.normal(), 1.0), rng.uniform(-np.pi, np.pi))
        t = rng.uniform(-20, 20, 3)
        x = (m.xyz[f].astype(np.float64) - t) @ R           # R^T (x - t)
        for c in range(2):
            centre = x[rng.integers(0, n_kp)]
            idx = np.argsort(np.linalg.norm(x - centre, axis=1))[:12]
            dl = LADDER[(q * 2 + c) % len(LADDER)]
            x[idx] -= THR * (1.0 + dl) * DIRS[(q + c) % len(DIRS)]
        qx[q] = x.astype(np.float32)
        ql[q] = m.label[f]
        info.append(dict(frame=f, R=R, t=t))
    return m, qx, ql, info
