"""The device side of the multi-GPU step at its edges (tests/_exchange_edges.py) in every form of the calls:
sgtd_merge_candidates_dev against the reference's loop on every case (word for word: frames, votes, n_cand, src, keep,
flags; my_table 0, last and -1; on stream 0, on a stream of the test's own, with the gathered tables at an offset inside a
larger allocation; every output pre-filled with a sentinel and one row longer than the call may write), its refusals,
sgtd_gather_verified_dev as bit patterns, the export of real batches (sgtd_set_candidate_export / sgtd_export_wait /
sgtd_export_release) and the whole step end to end against a single table.  tests/test_exchange_edges.py shows on the CPU
that these tables tell every mutant of the rule apart."""
import numpy as np
import pytest

import _exchange_edges as xe

pytestmark = pytest.mark.gpu

SENT = -77
INVALID, CAPACITY, UNSUPPORTED = -1, -4, -6


@pytest.fixture(scope="module")
def mods():
    from sgtd_amd import _lib, manager, synth
    return manager, synth, _lib


@pytest.fixture(scope="module")
def handles(mods):
    """one manager per candidate_num, made when first asked for and kept for the module"""
    made = {}

    def get(cn):
        if cn not in made:
            made[cn] = mods[0].STDescManager(candidate_num=cn)
        return made[cn]

    yield get
    for h in made.values():
        h.close()


@pytest.fixture(scope="module")
def own_stream():
    import torch
    return torch.cuda.Stream()


def _status(_lib, call, *a, **kw):
    with pytest.raises(_lib.SgtdError) as ei:
        call(*a, **kw)
    return ei.value.status


class Outputs:
    """the merge's output tensors, one row longer than nq and filled with a sentinel"""

    def __init__(self, nq, cn):
        import torch
        dev = torch.device("cuda", 0)
        self.nq, self.cn = nq, cn
        self.frame = torch.full((nq + 1, cn), SENT, dtype=torch.int32, device=dev)
        self.votes = torch.full((nq + 1, cn), SENT, dtype=torch.int32, device=dev)
        self.src = torch.full((nq + 1, cn), SENT, dtype=torch.int32, device=dev)
        self.n = torch.full((nq + 1,), SENT, dtype=torch.int32, device=dev)
        self.keep = torch.full((nq + 1,), SENT, dtype=torch.int64, device=dev)
        self.flags = torch.full((4,), SENT, dtype=torch.int32, device=dev)

    def args(self):
        return self.frame, self.votes, self.n, self.src, self.keep, self.flags

    def host(self):
        """-> dict of OUT_KEYS (the rows the call may write); asserts that nothing behind them was written"""
        import torch
        torch.cuda.synchronize()
        a = {k: getattr(self, k).cpu().numpy() for k in ("frame", "votes", "src", "n", "keep", "flags")}
        for k in ("frame", "votes", "src", "n", "keep"):
            assert (a[k][self.nq:] == SENT).all(), k
        assert (a["flags"][1:] == SENT).all()
        return {"frame": a["frame"][:self.nq], "votes": a["votes"][:self.nq], "n_cand": a["n"][:self.nq], "src": a["src"][:self.nq],
                "keep": a["keep"][:self.nq].view(np.uint64), "flags": int(a["flags"][0])}

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((getattr(self, k) == SENT).all()) for k in ("frame", "votes", "src", "n", "keep", "flags"))


def _on_device(arr, offset=0):
    """the int32 array on the device, `offset` ints into a larger allocation whose other words are a sentinel"""
    import torch
    host = np.full(arr.size + 2 * offset, SENT, np.int32)
    host[offset:offset + arr.size] = arr
    whole = torch.from_numpy(host).cuda()
    return whole, whole[offset:offset + arr.size]


def _merge(h, gathered, n_tables, my, nq, cn, stream=None):
    import torch
    out = Outputs(nq, cn)
    torch.cuda.synchronize()                           # (the fills, before a call on another stream)
    h.merge_candidates_dev(0 if stream is None else stream.cuda_stream, gathered, n_tables, my, nq, *out.args())
    return out.host()


def _same(got, want, where, keys=xe.OUT_KEYS):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (where, k, got[k], want[k])


# ---- the merge kernel on every case ----
@pytest.mark.parametrize("name", [n for n in sorted(xe.cases()) if n != "equal_keys"])
def test_merge_cases(handles, own_stream, name):
    for t in xe.cases()[name]:
        n_tables, nq, cn = t["frames"].shape
        h = handles(cn)
        arr = xe.packed_of(t)
        _, plain = _on_device(arr)
        whole, inside = _on_device(arr, offset=3)
        for my in xe.my_tables(n_tables):
            want = xe.expected(t, my)
            for form, gathered, stream in (("stream 0", plain, None), ("own stream", plain, own_stream), ("offset", inside, None)):
                _same(_merge(h, gathered, n_tables, my, nq, cn, stream), want, (name, t["note"], my, form))
        assert (whole[:3] == SENT).all() and (whole[-3:] == SENT).all()
        if name == "query_counts" and nq == 0:
            assert xe.expected(t, 0)["flags"] == 0 and xe.expected(t, 0)["frame"].shape == (0, cn)
        if name == "keep_bits":
            assert int(xe.expected(t, 0)["keep"][1]) == 2 ** 64 - 1 and int(xe.expected(t, 0)["keep"][0]) >> 63 == 1


def test_equal_keys(handles):
    """equal (frame, votes) pairs from two tables: ONE merged candidate, its src names one of the slots that hold it, and
    keep has its bit on that table only"""
    t, = xe.cases()["equal_keys"]
    n_tables, nq, cn = t["frames"].shape
    _, gathered = _on_device(xe.packed_of(t))
    got = {my: _merge(handles(cn), gathered, n_tables, my, nq, cn) for my in (0, 1, -1)}
    want = xe.expected(t, -1)
    for my in (0, 1, -1):
        _same(got[my], want, ("equal_keys", my), ("frame", "votes", "n_cand", "flags"))
        assert np.array_equal(got[my]["src"], got[0]["src"])
    for q in range(nq):
        at = np.flatnonzero(got[0]["frame"][q] == 500)
        assert at.size == 1 and got[0]["votes"][q, at[0]] == 20
        s = int(got[0]["src"][q, at[0]])
        tb, slot = s >> 8, s & 255
        assert tb * cn + slot in t["holders"][q] and t["frames"][tb, q, slot] == 500 and t["votes"][tb, q, slot] == 20
        bit = [int(got[my]["keep"][q]) >> slot_of & 1 for my, slot_of in ((0, t["holders"][q][0] % cn), (1, t["holders"][q][1] % cn))]
        assert sum(bit) == 1 and bit[tb] == 1 and int(got[-1]["keep"][q]) == 0
        # every other candidate is the rule's, src and keep included
        others = [k for k in range(cn) if k != at[0]]
        for my in (0, 1):
            assert np.array_equal(got[my]["src"][q, others], xe.expected(t, my)["src"][q, others])
            mask = ~(1 << (t["holders"][q][my] % cn)) & (2 ** 64 - 1)
            assert int(got[my]["keep"][q]) & mask == int(xe.expected(t, my)["keep"][q]) & mask


# ---- refusals ----
def test_refusals(mods, handles):
    import torch
    manager, _, _lib = mods
    dev = torch.device("cuda", 0)
    for n_tables, cn in ((25, 41), (1025, 1)):
        h = manager.STDescManager(candidate_num=cn) if cn == 41 else handles(cn)
        nq = 2
        gathered = torch.zeros(n_tables * (2 * nq * cn + 4), dtype=torch.int32, device=dev)
        out = Outputs(nq, cn)
        assert xe.per_of(n_tables * cn) is None and n_tables * cn == 1025
        assert _status(_lib, h.merge_candidates_dev, 0, gathered, n_tables, 0, nq, *out.args()) == UNSUPPORTED
        assert out.untouched()
        if cn == 41:
            h.close()
    t, = xe.cases()["ties"]
    n_tables, nq, cn = t["frames"].shape
    h = handles(cn)
    _, gathered = _on_device(xe.packed_of(t))
    out = Outputs(nq, cn)
    for tables, my in ((n_tables, n_tables), (n_tables, -2), (0, 0), (0, -1)):
        assert _status(_lib, h.merge_candidates_dev, 0, gathered, tables, my, nq, *out.args()) == INVALID, (tables, my)
    assert out.untouched()
    # ... and the handle still merges
    _same(_merge(h, gathered, n_tables, 0, nq, cn), xe.expected(t, 0), "after the refusals")
    # a multi-device handle merges on the host: none of the exchange calls is available
    g = manager.STDescManager(devices=[0, 0], candidate_num=cn)
    buf = torch.zeros(64, dtype=torch.int32, device=dev)
    score = torch.zeros((nq, cn), dtype=torch.float64, device=dev)
    pose = torch.zeros((nq, cn, 12), dtype=torch.float64, device=dev)
    vg = torch.zeros(n_tables * nq * cn * 13, dtype=torch.float64, device=dev)
    assert _status(_lib, g.set_candidate_export, buf) == UNSUPPORTED
    assert _status(_lib, g.export_wait, 0) == UNSUPPORTED
    assert _status(_lib, g.export_release, 0) == UNSUPPORTED
    assert _status(_lib, g.merge_candidates_dev, 0, gathered, n_tables, 0, nq, *out.args()) == UNSUPPORTED
    assert _status(_lib, g.gather_verified_dev, 0, vg, n_tables, out.src, nq, score, pose) == UNSUPPORTED
    assert out.untouched()
    g.close()


# ---- the verification results of the merged candidates ----
@pytest.mark.parametrize("name", sorted(xe.gather_cases()))
def test_gather_verified(handles, own_stream, name):
    import torch
    c = xe.gather_cases()[name]
    n_tables, nq, cn = c["n_tables"], c["nq"], c["cn"]
    dev = torch.device("cuda", 0)
    want_s, want_p = xe.gather_ref(c["gathered"], c["src"], nq, cn)
    gathered = torch.from_numpy(c["gathered"].reshape(-1).view(np.int64).copy()).to(dev).view(torch.float64)
    if gathered.numel() == 0:
        gathered = torch.zeros(8, dtype=torch.float64, device=dev)
    assert name in ("nq0",) or np.array_equal(gathered.cpu().view(torch.int64).numpy().view(np.uint64), c["gathered"].reshape(-1))
    src = torch.from_numpy(np.concatenate([c["src"].reshape(-1), np.full(cn, SENT, np.int32)])).to(dev)
    pattern = np.array([0x7FF8000000000BAD]).view(np.int64)[0]              # a NaN no case holds
    for stream in (None, own_stream):
        score = torch.full(((nq + 1) * cn,), int(pattern), dtype=torch.int64, device=dev)
        pose = torch.full(((nq + 1) * cn * 12,), int(pattern), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        handles(cn).gather_verified_dev(0 if stream is None else stream.cuda_stream, gathered, n_tables, src, nq, score.view(torch.float64), pose.view(torch.float64))
        torch.cuda.synchronize()
        got_s, got_p = score.cpu().numpy().view(np.uint64), pose.cpu().numpy().view(np.uint64)
        assert np.array_equal(got_s[:nq * cn].reshape(nq, cn), want_s), name
        assert np.array_equal(got_p[:nq * cn * 12].reshape(nq, cn, 12), want_p), name
        assert (got_s[nq * cn:] == np.uint64(0x7FF8000000000BAD)).all() and (got_p[nq * cn * 12:] == np.uint64(0x7FF8000000000BAD)).all(), name


# ---- the export, on real batches ----
F_MAP, KP, NQ = 45, 140, 9
QUERY_FRAMES = [3, 10, 20, 30, 44, 40, 12, 25, 37]
NO_LABEL = 13          # the map's labels are 3 .. 11: a keypoint labelled 13 gives label codes that no table entry has


@pytest.fixture(scope="module")
def world(mods):
    _, synth, _ = mods
    big = synth.make_map(120, KP, stream=611)
    qs = [synth.make_queries(big, NQ, stream=612 + k, frames=QUERY_FRAMES) for k in range(3)]
    for q in qs:
        assert q.label.min() >= 3 and q.label.max() <= 11
        q.label[6:] = NO_LABEL                   # the last three queries match nothing: no votes, no candidate
    return big, qs


def _table_handle(manager, big, lo=0, hi=F_MAP, **kw):
    h = manager.STDescManager(first_frame_id=lo, **kw)
    if hi > lo:
        h.add_frames(big.xyz[lo:hi], big.label[lo:hi])
        h.finalize()
    return h


def _exported(packed, nq, cn):
    import torch
    torch.cuda.synchronize()
    a = packed.cpu().numpy()
    return a[:nq * cn].reshape(nq, cn), a[nq * cn:2 * nq * cn].reshape(nq, cn), a[2 * nq * cn:2 * nq * cn + 4], a[2 * nq * cn + 4:]


def _is_the_batch(packed, res, nq, cn, serial, where):
    f, v, words, tail = _exported(packed, nq, cn)
    assert np.array_equal(f, res.cand_frame) and np.array_equal(v, res.cand_votes), where
    assert words[:3].tolist() == [0, nq, cn] and (words[3] >= 1 if serial is None else words[3] == serial), (where, words, serial)
    assert (tail == SENT).all(), where
    for q in range(nq):                                                     # (unused slots included: they are -1 / 0)
        assert (f[q, res.n_cand[q]:] == -1).all() and (v[q, res.n_cand[q]:] == 0).all(), where


@pytest.mark.parametrize("cn", [1, 50])
def test_export_of_real_batches(mods, world, cn):
    import torch
    manager, _, _lib = mods
    big, qs = world
    dev = torch.device("cuda", 0)
    h = _table_handle(manager, big, candidate_num=cn)
    ints = int(h._L.sgtd_candidate_export_ints(NQ, cn))
    assert ints == 2 * NQ * cn + 4

    def buffer(n):
        return torch.full((n,), SENT, dtype=torch.int32, device=dev)

    # a buffer of exactly the size: three batches, the serial rises by one per batch
    exact = buffer(ints)
    h.set_candidate_export(exact)
    first = None
    for k in range(3):
        h.query_frames(qs[k].xyz, qs[k].label, fetch=False)
        res = h.results()
        serial = int(_exported(exact, NQ, cn)[2][3])
        first = serial if first is None else first
        _is_the_batch(exact, res, NQ, cn, first + k, ("exact", k))
        assert (res.n_cand[:6] > 0).any() and (res.n_cand[6:] == 0).all()
    serial = first + 2
    # a longer buffer keeps its tail
    longer = buffer(ints + 5)
    h.set_candidate_export(longer)
    res = h.query_frames(qs[0].xyz, qs[0].label)
    serial += 1
    _is_the_batch(longer, res, NQ, cn, serial, "longer")
    assert _exported(longer, NQ, cn)[3].size == 5
    # one int short: the batch is refused, nothing is written; a large enough buffer works again
    short = buffer(ints - 1)
    h.set_candidate_export(short)
    assert _status(_lib, h.query_frames, qs[1].xyz, qs[1].label) == CAPACITY
    torch.cuda.synchronize()
    assert (short == SENT).all()
    exact.fill_(SENT)
    h.set_candidate_export(exact)
    res = h.query_frames(qs[1].xyz, qs[1].label)
    serial += 1
    _is_the_batch(exact, res, NQ, cn, serial, "after the short buffer")
    # fewer ints than the flag words
    assert _status(_lib, h.set_candidate_export, buffer(3)) == INVALID
    res = h.query_frames(qs[2].xyz, qs[2].label)                            # (the registered buffer stays)
    serial += 1
    _is_the_batch(exact, res, NQ, cn, serial, "after the refused buffer")
    # None stops the writes
    exact.fill_(SENT)
    h.set_candidate_export(None)
    res = h.query_frames(qs[0].xyz, qs[0].label)
    torch.cuda.synchronize()
    assert (exact == SENT).all() and (res.n_cand > 0).any()
    h.close()


GRID_PASS_FRAMES, GRID_PASS_KP = 2049, 10          # descriptor_near_num = 10: a frame of 9 keypoints gives no descriptor


def test_export_takes_a_second_grid_pass(mods, world):
    """candidate_num 64 and 2049 query frames: nq * cn = 131 136 > 512 * 256, the last query's row is written in the
    kernel's second pass.  The frames are cut to their first 10 keypoints, the fewest that still give descriptors (19 to 81
    per frame on the first sixteen, none at 9), the first and the last two are whole, so that candidates stand at both ends"""
    import torch
    manager, synth, _ = mods
    big, _ = world
    cn, nq = 64, GRID_PASS_FRAMES
    assert nq * cn == 131136 > 512 * 256
    qs = synth.make_queries(big, nq, stream=640, frames=np.arange(nq) % F_MAP)
    n_kp = np.full(nq, GRID_PASS_KP, np.int64)
    n_kp[[0, 1, nq - 2, nq - 1]] = KP
    off = np.concatenate([[0], np.cumsum(n_kp)])
    xyz = np.concatenate([qs.xyz[q, :n_kp[q]] for q in range(nq)]).astype(np.float32)
    label = np.concatenate([qs.label[q, :n_kp[q]] for q in range(nq)])
    h = _table_handle(manager, big, candidate_num=cn)
    assert h.config_setting_["descriptor_near_num"] == GRID_PASS_KP
    for q in (2, 700, nq - 3):
        assert h.BuildSingleScanSTD(qs.xyz[q, :GRID_PASS_KP], qs.label[q, :GRID_PASS_KP]).n > 0
        assert h.BuildSingleScanSTD(qs.xyz[q, :GRID_PASS_KP - 1], qs.label[q, :GRID_PASS_KP - 1]).n == 0
    ints = int(h._L.sgtd_candidate_export_ints(nq, cn))
    packed = torch.full((ints + 2,), SENT, dtype=torch.int32, device=torch.device("cuda", 0))
    h.set_candidate_export(packed)
    res = h.query_frames(xyz, label, off)
    _is_the_batch(packed, res, nq, cn, None, "2049 frames")
    assert res.n_cand[0] > 0 and res.n_cand[nq - 1] > 0 and (res.n_cand[2:nq - 2] > 0).any(), (res.n_cand[[0, nq - 1]], int((res.n_cand > 0).sum()))
    h.close()


def test_export_read_on_a_side_stream(mods, world):
    """two consecutive batches, each read on a side stream between sgtd_export_wait and sgtd_export_release with no host
    wait in between, give the tables that reading them on the handle's stream gives"""
    import torch
    manager, _, _ = mods
    big, qs = world
    cn = 50
    main, side = torch.cuda.Stream(), torch.cuda.Stream()
    h = manager.STDescManager(candidate_num=cn)
    h.set_stream(main.cuda_stream)
    h.add_frames(big.xyz[:F_MAP], big.label[:F_MAP])
    h.finalize()
    packed = torch.full((2 * NQ * cn + 4,), SENT, dtype=torch.int32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    h.set_candidate_export(packed)
    on_main = []
    for k in (0, 1):
        h.query_frames(qs[k].xyz, qs[k].label, fetch=False)
        with torch.cuda.stream(main):
            on_main.append(packed.clone())
    torch.cuda.synchronize()
    on_side = []
    for k in (0, 1):
        h.query_frames(qs[k].xyz, qs[k].label, fetch=False)
        h.export_wait(side.cuda_stream)
        with torch.cuda.stream(side):
            on_side.append(packed.clone())
        h.export_release(side.cuda_stream)
    torch.cuda.synchronize()
    res = h.results()
    for k in (0, 1):
        a, b = on_main[k].cpu().numpy(), on_side[k].cpu().numpy()
        assert np.array_equal(a[:-1], b[:-1]) and b[-1] == a[-1] + 2, k           # (the serial: two batches later)
        assert a[-4:-1].tolist() == [0, NQ, cn]
    assert not np.array_equal(on_side[0].cpu().numpy()[:-4], on_side[1].cpu().numpy()[:-4])
    assert np.array_equal(on_side[1].cpu().numpy()[:NQ * cn].reshape(NQ, cn), res.cand_frame)
    h.close()


# ---- end to end ----
def _through_the_kernels(shards, q, cn, where):
    """the step over the shards' handles in one process: export -> merge kernel on every shard -> lists and verification of
    the winners only -> the results out of the owners' tables.  The merged list is merge_ref's over the exported tables"""
    import torch
    dev = torch.device("cuda", 0)
    n_tables = len(shards)
    ints = 2 * NQ * cn + 4
    packed = []
    for m in shards:
        p = torch.full((ints,), SENT, dtype=torch.int32, device=dev)
        m.set_candidate_export(p)
        m.set_deferred_lists(True)
        m.query_frames(q.xyz, q.label, fetch=False)
        packed.append(p)
    torch.cuda.synchronize()
    gathered = torch.cat(packed).contiguous()
    frames, votes, words = xe.unpacked(gathered.cpu().numpy(), n_tables, NQ, cn)
    assert (words[:, :3] == [0, NQ, cn]).all(), where
    v_all = torch.empty((n_tables, NQ * cn * 13), dtype=torch.float64, device=dev)
    outs = []
    for r, m in enumerate(shards):
        out = Outputs(NQ, cn)
        m.merge_candidates_dev(0, gathered, n_tables, r, NQ, *out.args())
        got = out.host()
        want = dict(zip(xe.OUT_KEYS, xe.merge_ref(frames, votes, cn, r) + (0,)))
        _same(got, want, (where, r))
        keep = out.keep[:NQ].contiguous()
        m.finish_lists(keep)
        m.verify_masked(keep)
        m.export_verify(v_all[r, :NQ * cn], v_all[r, NQ * cn:])
        outs.append((got, out))
    torch.cuda.synchronize()
    score = torch.empty((NQ, cn), dtype=torch.float64, device=dev)
    pose = torch.empty((NQ, cn, 12), dtype=torch.float64, device=dev)
    src = outs[0][1].src[:NQ].contiguous()
    shards[0].gather_verified_dev(0, v_all.reshape(-1), n_tables, src, NQ, score, pose)
    torch.cuda.synchronize()
    want_s, want_p = xe.gather_ref(v_all.cpu().numpy().view(np.uint64), outs[0][0]["src"], NQ, cn)
    assert np.array_equal(xe.bits(score.cpu().numpy()), want_s) and np.array_equal(xe.bits(pose.cpu().numpy()), want_p), where
    return outs[0][0], score.cpu().numpy(), pose.cpu().numpy(), frames


@pytest.mark.parametrize("mode", ["1", "2"])
@pytest.mark.parametrize("cn", [1, 64])
def test_every_form_gives_the_single_tables_answer(mods, world, monkeypatch, cn, mode):
    """a single table, a devices=[0, 0, 0] handle, one shard through the kernels, three shards, and three shards of which
    the middle one holds no frame (its two frames were removed again: the form of an empty table that a frames batch is known to
    run on): the same merged list and the same verification"""
    manager, _, _ = mods
    monkeypatch.setenv("SGTD_SELECT_MODE", mode)
    big, qs = world
    q = qs[0]
    single = _table_handle(manager, big, candidate_num=cn)
    want = single.query_frames(q.xyz, q.label)
    single.verify()
    w_verify = [single.result_verify(k) for k in range(NQ)]
    assert (want.n_cand[6:] == 0).all() and (want.n_cand[:6] > 0).any() and (cn == 1 or (want.n_cand > 1).any())

    def is_the_single_tables(n_cand, frame, votes, verify_of, where):
        assert np.array_equal(n_cand, want.n_cand), where
        for k in range(NQ):
            nc = int(want.n_cand[k])
            assert np.array_equal(frame[k, :nc], want.cand_frame[k, :nc]) and np.array_equal(votes[k, :nc], want.cand_votes[k, :nc]), (where, k)
            score, rot, t = verify_of(k)
            assert np.array_equal(score, w_verify[k][0]), (where, k)
            assert np.array_equal(rot, w_verify[k][1]) and np.array_equal(t, w_verify[k][2]), (where, k)

    multi = manager.STDescManager(devices=[0, 0, 0], candidate_num=cn)
    multi.add_frames(big.xyz[:F_MAP], big.label[:F_MAP])
    multi.finalize()
    res = multi.query_frames(q.xyz, q.label)
    multi.verify()
    is_the_single_tables(res.n_cand, res.cand_frame, res.cand_votes, multi.result_verify, "devices=[0, 0, 0]")
    multi.close()

    cut = [0, 15, 30, F_MAP]
    forms = {"one shard": [(0, F_MAP)], "three shards": list(zip(cut[:-1], cut[1:])), "empty middle": [(0, 22), None, (22, F_MAP)]}
    for where, ranges in forms.items():
        shards = []
        for r in ranges:
            if r is None:
                m = _table_handle(manager, big, 22, 24, candidate_num=cn)
                assert m.remove_frames([22, 23]) > 0 and m.stats()["n_entries"] == 0
            else:
                m = _table_handle(manager, big, r[0], r[1], candidate_num=cn)
            shards.append(m)
        merged, score, pose, frames = _through_the_kernels(shards, q, cn, where)
        if where == "empty middle":
            assert (frames[1] == -1).all()
        if where == "three shards" and cn > 1:
            assert len({int(s) >> 8 for s in merged["src"].reshape(-1) if s >= 0}) > 1       # winners from more than one shard
        is_the_single_tables(merged["n_cand"], merged["frame"], merged["votes"],
                             lambda k: (score[k], pose[k, :, :9].reshape(cn, 3, 3), pose[k, :, 9:]), where)
        for m in shards:
            m.close()
    single.close()
