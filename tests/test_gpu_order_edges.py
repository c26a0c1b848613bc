"""The batch ordering (order_kernels.hip.h: one-sweep radix passes, fused group index) at its edges, in both forms of the
call: SGTD_ORDER_FORM=0, the launch train, and =1, the new chain.  Workloads: tests/_order_edges.py (tests/test_order_edges.py
shows that they reach their edges).  Every case is checked with exact equality: candidates, votes, pair_off, every match list
in order and the vote vector against the oracle; last_P, last_M, last_D against the oracle; last_P, last_P_swept, last_M and
last_cand_pairs between the two forms (last_P_swept depends on which descriptors share a pass: the witness that the order
is the same).  order_giveups_total stays 0 except under SGTD_ORDER_POLLS=0, the forced fallback.

A one-frame call of at most SMALL_SLOTS descriptors reaches the general ordering only under SGTD_SMALL_ORDER=0, which is
read once per process: run as a script (`python tests/test_gpu_order_edges.py small0`) this file checks those cases.
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

import _order_edges as oe  # noqa: E402
import _overflow_edges as ov  # noqa: E402
import _select_edges as se  # noqa: E402
from test_gpu_sweep_setup import _check  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL_SLOTS = 8192            # SGTD_SMALL_SLOTS of probe_kernels.hip.h: a one-frame call above it takes the general ordering
WITNESS = ("last_P", "last_P_swept", "last_M", "last_cand_pairs")
TOTALS = ("order_giveups_total", "reruns_total", "overflow_launches_total")


@pytest.fixture(scope="module")
def mods():
    from oracle import oracle
    from sgtd_amd import manager, synth
    oracle.build_library()
    return oracle, manager, synth


class _Env:
    """monkeypatch's two calls, for the script"""

    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k):
        del os.environ[k]


def _new(manager, mp, env, **kw):
    """a handle created under the hooks `env` (each is read once per handle, in sgtd_create)"""
    for k, v in env.items():
        mp.setenv(k, str(v))
    try:
        return manager.STDescManager(**kw)
    finally:
        for k in env:
            mp.delenv(k)


def _sizes():
    T, G = oe.tiles()
    return T, G


def _n(name):
    T, G = _sizes()
    return oe.case(name, T, G)[1]


def _descs_case(mods, mp, name, form="plain", env={}, order_forms=(0, 1), batch_env={}):
    """one case through a handle per ordering form -> {form: (stats, the counters' movement)}"""
    oracle, manager, _ = mods
    T, G = _sizes()
    wl, n = oe.case(name, T, G)
    frame = se.QUERY_FRAME
    if form == "frames":          # the query carries the id of a frame the table holds (the sweep's FRAMES variant)
        plain = oe.expected(oracle, name, T, G)
        frame = int(plain["cand_frame"][0]) if len(plain["cand_frame"]) else 0
    ans = oe.expected(oracle, name, T, G, frame)
    out = {}
    for of in order_forms:
        tag = "%s/%s/form %d %s %s" % (name, form, of, env, batch_env)
        g = _new(manager, mp, dict(env, SGTD_ORDER_FORM=of), rough_dis_threshold=oe.ROUGH)
        if form == "tail":
            h = len(wl.adds) // 2
            wl.load(g, manager, 0, h)
            g.finalize()                                   # (the table is built: what follows goes to a tail segment)
            wl.load(g, manager, h, None)
        else:
            wl.load(g, manager)
        before = {t: g.stats()[t] for t in TOTALS}
        for k, v in batch_env.items():                     # (read when the batch is planned)
            mp.setenv(k, str(v))
        try:
            g.query_descs(oe.query_descs(wl, manager, frame))
            _check(g, ans, tag)
        finally:
            for k in batch_env:
                mp.delenv(k)
        st = g.stats()
        assert st["last_M"] == ans["M"] and st["last_D"] == ans["D"] == n and st["last_P"] == ans["P"], (tag, st["last_P"], ans["P"])
        assert st["last_cand_pairs"] == ans["T"], tag
        if form == "tail":
            assert st["tail_entries"] > 0, tag
        out[of] = (st, {t: int(st[t] - before[t]) for t in TOTALS})
        g.close()
    if len(out) == 2:
        for w in WITNESS:
            assert out[0][0][w] == out[1][0][w], (name, form, w, out[0][0][w], out[1][0][w])
    return out


def _quiet(out):
    for of, (st, d) in out.items():
        assert d["order_giveups_total"] == 0 and d["reruns_total"] == 0 and st["overflowed"] == 0, (of, d)


def _small_names():
    T, G = _sizes()
    return [name for name in oe.CASES if oe.case(name, T, G)[1] <= SMALL_SLOTS]


@pytest.mark.parametrize("form", ["plain", "tail"])
@pytest.mark.parametrize("name", oe.CASES)
def test_descriptor_cases(mods, monkeypatch, name, form):
    if _n(name) <= SMALL_SLOTS:      # (in this process such a call is small_order_kernel's: the case runs in the process below)
        assert name in _small_names()
        return
    _quiet(_descs_case(mods, monkeypatch, name, form))


def test_small_cases_in_a_process_of_their_own():
    """the cases of at most SMALL_SLOTS descriptors (1 and the counts around the smaller tile), plain and tail, under
    SGTD_SMALL_ORDER=0"""
    assert len(_small_names()) >= 4
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "small0"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, SGTD_SMALL_ORDER="0"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    assert "small0 ok" in p.stdout


def test_frames_form(mods, monkeypatch):
    T, G = _sizes()
    _quiet(_descs_case(mods, monkeypatch, oe.deep(T, G), "frames"))


@pytest.mark.parametrize("mode", [1, 2])
def test_select_modes(mods, monkeypatch, mode):
    T, G = _sizes()
    out = _descs_case(mods, monkeypatch, oe.deep(T, G), env={"SGTD_SELECT_MODE": mode})
    _quiet(out)
    assert out[1][0]["select_form"] == (0 if mode == 1 else out[0][0]["select_form"])


@pytest.mark.parametrize("name", ["deep", "markers"])
def test_wide_keys_take_the_launch_train(mods, monkeypatch, name):
    """SGTD_HOME_SUB_BITS=4: 34 key bits — both forms of the call run the launch train, and the results hold"""
    T, G = _sizes()
    _quiet(_descs_case(mods, monkeypatch, oe.deep(T, G) if name == "deep" else name, batch_env={"SGTD_HOME_SUB_BITS": oe.WIDE_SUB_BITS}))


def test_forced_fallback(mods, monkeypatch):
    """SGTD_ORDER_POLLS=0: every tile but the first gives up its look-back at once (an ordinary early exit), the batch is
    flagged, sgtd_sync runs it again with the launch train — once — and the results are exact"""
    T, G = _sizes()
    name = oe.deep(T, G)
    ref = _descs_case(mods, monkeypatch, name, order_forms=(0,))
    out = _descs_case(mods, monkeypatch, name, env={"SGTD_ORDER_POLLS": 0}, order_forms=(1,))
    st, d = out[1]
    assert d["order_giveups_total"] == 1 and d["reruns_total"] == 1 and st["overflowed"] == 1, d
    assert d["overflow_launches_total"] == 1, d
    for w in WITNESS:
        assert st[w] == ref[0][0][w], w
    _quiet(ref)


def _keypoint_batch(mods, mp, run, n_q, expect):
    """a batch built from keypoints on the device through a handle per ordering form; expect(q) -> the oracle's answer"""
    _, manager, _ = mods
    wit = {}
    for of in (0, 1):
        g = _new(manager, mp, {"SGTD_ORDER_FORM": of})
        before = {t: g.stats()[t] for t in TOTALS}
        run(g)
        res = g.results()
        for q in range(n_q):
            _check(g, expect(q), "keypoints/form %d/frame %d" % (of, q), q=q, res=res)
        st = g.stats()
        assert all(st[t] == before[t] for t in TOTALS) and st["overflowed"] == 0, of
        wit[of] = {w: st[w] for w in WITNESS + ("last_D",)}
        g.close()
    assert wit[0] == wit[1], wit
    return wit[1]


def test_ragged_frames_batch(mods, monkeypatch):
    """query frames without a descriptor between full ones: the descriptor slots are several times the live descriptors"""
    oracle, _, synth = mods
    m, xyz, label, off = oe.ragged_world(synth)
    o = oracle.OracleManager()
    for f in range(m.xyz.shape[0]):
        o.build(m.xyz[f], m.label[f], export=False)
        o.add_last()
    sels, D = [], 0
    for q in range(len(oe.RAGGED)):
        D += o.build(xyz[off[q]:off[q + 1]], label[off[q]:off[q + 1]], export=False)
        sels.append(ov._answer(o, o.select(), 0, with_rough=False, with_entries=False))

    def run(g):
        g.add_frames(m.xyz, m.label)
        g.query_frames(xyz, label, kp_off=off, fetch=False)

    wit = _keypoint_batch(mods, monkeypatch, run, len(oe.RAGGED), lambda q: sels[q])
    assert wit["last_D"] == D and wit["last_M"] == sum(s["M"] for s in sels)


def test_empty_batch(mods, monkeypatch):
    """0 live descriptors: every query frame has too few keypoints for a descriptor"""
    oracle, _, synth = mods
    m = synth.make_map(12, 60, stream=9)
    qs = synth.make_queries(m, 3, stream=9)
    xyz, label = qs.xyz[:, :4].copy(), qs.label[:, :4].copy()
    empty = dict(cand_frame=np.zeros(0, np.int32), cand_votes=np.zeros(0, np.int32), cand_off=np.zeros(1, np.int64),
                 q_idx=np.zeros(0, np.int32), db_entry=np.zeros(0, np.int64), votes=np.zeros(se.MAX_FRAME_N))

    def run(g):
        g.add_frames(m.xyz, m.label)
        g.query_frames(xyz, label, fetch=False)

    wit = _keypoint_batch(mods, monkeypatch, run, 3, lambda q: empty)
    assert wit["last_D"] == 0 and wit["last_M"] == 0 and wit["last_P"] == 0


def test_loop_batch(mods, monkeypatch):
    """sgtd_loop_frames in one chunk: the oracle's sequential loop"""
    oracle, _, synth = mods
    m, ses, sels = ov.loop_expected(oracle, synth, 0)
    n = ses.xyz.shape[0]

    def run(g):
        g.add_frames(m.xyz, m.label)
        g.loop_frames(ses.xyz, ses.label, skip_near=0, batch=n, fetch=False)

    wit = _keypoint_batch(mods, monkeypatch, run, n, lambda q: sels[q])
    assert wit["last_M"] == sum(s["M"] for s in sels)


if __name__ == "__main__":
    if sys.argv[1:] == ["small0"]:
        assert os.environ.get("SGTD_SMALL_ORDER") == "0"
        from oracle import oracle
        from sgtd_amd import manager, synth
        oracle.build_library()
        ms = (oracle, manager, synth)
        for nm in _small_names():
            for fm in ("plain", "tail"):
                _quiet(_descs_case(ms, _Env(), nm, fm))
        print("small0 ok")
