"""The workloads of tests/test_gpu_table_edges.py, checked without a GPU: the plain restatement of the table's structure
(tests/_table_edges.py) equals the oracle on every small workload — dump, census rough list, census votes — in its loop
and its vectorised form; every workload reaches the count it exists for; and wrong builds of the restatement (mutants)
are told apart by at least one workload."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _select_edges as se  # noqa: E402
import _table_edges as te  # noqa: E402

NAMES = list(te.cases())


@pytest.fixture(scope="module")
def oracle_of(oracle_mod):
    """name -> (oracle manager with the workload added call by call, its dump), built once"""
    memo = {}

    def get(name):
        if name not in memo:
            c = te.cases()[name]
            o = oracle_mod.OracleManager(**{k: v for k, v in c.cfg.items() if k in oracle_mod.DEFAULTS})
            for lo, hi in c.call_bounds():
                o.add(c.descs(oracle_mod, lo, hi))
            memo[name] = (o, o.table_dump())
        return memo[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_oracle(name, oracle_of, oracle_mod):
    c = te.cases()[name]
    o, dump = oracle_of(name)
    vec = c.structure()
    for a, b, what in zip(vec, dump, ("keys", "bucket_off", "entry ids")):
        np.testing.assert_array_equal(a, b, err_msg="%s %s" % (name, what))
    for a, b, what in zip(te.structure_loop(c.side, c.label, c.frame), vec, ("keys", "bucket_off", "entry ids")):
        np.testing.assert_array_equal(a, b, err_msg="%s loop %s" % (name, what))
    ref = None
    for k, (qs, ql) in enumerate(c.census()):
        o.select(c.query_descs(oracle_mod, k))
        theirs = o.rough_matches()
        if ref is None:
            ref = te.RefTable()
            ref.add(c.side, c.label, c.frame)
        rq, rc, re_ = te.ref_rough(ref, qs, ql, c.qframe, te.ROUGH)
        for a, key in ((rq, "q_idx"), (rc, "cell"), (re_, "db_entry")):
            np.testing.assert_array_equal(a, theirs[key], err_msg="%s census %d %s" % (name, k, key))
        votes = np.bincount(c.frame[re_].astype(np.int64), minlength=c.cfg["max_frame_n"]).astype(np.float64)
        np.testing.assert_array_equal(votes, o.votes(), err_msg="%s census %d votes" % (name, k))
        if k == 0 and c.E:                               # every bucket's descriptor finds its whole bucket
            keys, off, ids = vec
            n_b = min(len(keys), te.CENSUS_MAX)
            found = np.zeros(n_b, np.int64)
            own = rq < n_b
            np.add.at(found, rq[own], 1)
            assert np.all(found >= (off[1:] - off[:-1])[:n_b]), name


# ---- reach ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", te.SORT_E)
def test_sort_counts_reach(E):
    c = te.cases()["sort_counts/E%d" % E]
    assert c.E == E
    code, x, y, z = te.key_fields(c.side, c.label)
    k = te.pack_key(code, x, y, z)
    if E >= 4095:                                        # all seven whole key bytes and the top nibble vary
        for b in range(8):
            assert len(np.unique((k >> np.uint64(8 * b)) & np.uint64(255))) > (8 if b == 7 else 100), b
    keys, off, ids = c.structure()
    if E >= 255:                                         # buckets of several frames and several of one frame
        multi = sum(1 for u in range(len(keys)) if len(set(c.frame[ids[off[u]:off[u + 1]]])) > 1
                    and len(c.frame[ids[off[u]:off[u + 1]]]) > len(set(c.frame[ids[off[u]:off[u + 1]]])))
        assert multi >= len(keys) // 2
    passes = te.radix_passes(c)
    for at in (te.RS_ROUND, te.RS_TILE):                 # equal keys straddle the round / tile boundary of the input ...
        if E > at:
            assert k[at - 1] == k[at], at
            # ... and of the input of a later pass
            assert any(kk[at - 1] == kk[at] for _, kk in passes[:-1]), at
    if E > 1:
        assert len(passes) == 8 or E < 64


def test_digit_skip_reach():
    cs = te.cases()
    assert te.radix_passes(cs["digit_skip/all_equal"]) == [] and len(cs["digit_skip/all_equal"].structure()[0]) == 1
    for b in range(8):
        c = cs["digit_skip/one_differs_byte%d" % b]
        assert [p[0] for p in te.radix_passes(c)] == [b]
        code, x, y, z = te.key_fields(c.side, c.label)
        d = (te.pack_key(code, x, y, z) >> np.uint64(8 * b)) & np.uint64(255)
        assert np.unique(d, return_counts=True)[1].max() == c.E - 1
    assert [p[0] for p in te.radix_passes(cs["digit_skip/top_byte_only"])] == [7]
    assert [p[0] for p in te.radix_passes(cs["digit_skip/code_all_bits"])] == [6, 7]
    assert set(cs["digit_skip/code_all_bits"].structure()[0][:, 3]) == {0, 0xFFF}
    k = cs["digit_skip/cells_0_and_65535"].structure()[0]
    assert len(k) == 8 and all(set(k[:, a]) == {0, 65535} for a in range(3))


@pytest.mark.parametrize("E, kind", te.SCAN_CASES)
def test_scan_counts_reach(E, kind):
    c = te.cases()["scan_counts/E%d_%s" % (E, kind)]
    keys, off, ids = c.structure()
    assert c.E == E and -(-E // te.SCAN_BLOCK) == {2048: 1, 2049: 2, 32768: 16, 32769: 17}[E]
    tiles = -(-E // te.RS_TILE)
    assert 256 * tiles == {2048: 256, 2049: 256, 32768: 2048, 32769: 2304}[E]
    if kind == "U1":
        assert len(keys) == 1
    elif kind == "UE":
        assert len(keys) == E
    else:
        heads = set(off[:-1].tolist())
        assert 1 < len(keys) < E and te.SCAN_BLOCK - 1 in heads
        assert (E < 2049 or te.SCAN_BLOCK in heads) and (E < 2050 or te.SCAN_BLOCK + 1 in heads)


def test_partition_counts_reach():
    c = te.cases()["partition_counts/sizes"]
    spread = te.slice_spread(c)
    got = sorted((n, tuple(sorted(s))) for n, s in spread.values())
    want = []
    for n in te.PART_SIZES:
        want.append((n, (se.sub_cell(te.DELTA),)))
        if n > 1:
            want += [(n, (0, 1, 2, 3, 4, 5, 6)), (n, (6,))]
    assert got == sorted(want)
    m = te.cases()["partition_counts/many_buckets"]
    keys, off, _ = m.structure()
    W = te.WAVES_MI355X
    size = off[1:] - off[:-1]
    assert len(keys) == 2 * W and (size[0], size[W - 1], size[W], size[-1]) == (65, 200, 64, 129)
    assert np.all(np.delete(size, [0, W - 1, W, 2 * W - 1]) == 1)


def test_hash_counts_reach():
    cs = te.cases()
    for U, cap in ((511, 1024), (512, 1024), (513, 2048), (1024, 2048), (1025, 4096)):
        c = cs["hash_counts/U%d" % U]
        assert len(c.structure()[0]) == U and te.hash_slots(c)[2] == cap
    c = cs["hash_counts/chain"]
    home, used, cap, _ = te.hash_slots(c)
    assert cap == 1024 and len(home) == 512
    slot, n = np.unique(home, return_counts=True)
    h = int(slot[np.argmax(n)])
    assert n.max() >= 40 and all((h + d) % cap in used for d in range(40))
    qs, ql = c.extra[0]                                  # the absent key: home inside the chain, nothing found
    code, x, y, z = te.key_fields(qs[None], ql[None])
    ah = int(te.hash_key(te.pack_key(code, x, y, z))[0]) & (cap - 1)
    assert h < ah < h + 40
    assert not any(tuple(k) == (x[0], y[0], z[0], code[0]) for k in c.structure()[0])
    ref = te.RefTable()
    ref.add(c.side, c.label, c.frame)
    s, l = c.census()[0]
    assert len(s) == 513 and 512 not in te.ref_rough(ref, s, l, c.qframe, te.ROUGH)[0]
    home, used, cap, wrapped = te.hash_slots(cs["hash_counts/wrap"])
    assert cap == 1024 and wrapped >= 1 and np.sum(home >= cap - 3) >= 6 and {cap - 3, cap - 2, cap - 1, 0, 1} <= used


def test_id_bits_reach():
    cs = te.cases()
    for n, bits, tail in ((8192, 13, 8192), (8193, 14, 0)):
        c = cs["id_bits/frame_of_%d" % n]
        assert np.unique(c.frame, return_counts=True)[1].max() == n and te.rank_bits(c.frame) == bits
        assert te.rank_bits(c.frame[:c.cut_entry()]) == 13 and c.expected_tail() == tail
    c = cs["id_bits/span_600000"]
    assert te.rank_bits(c.frame) == 12 and np.unique(c.frame, return_counts=True)[1].max() <= 4096
    c = cs["id_bits/span_2p20m2"]
    assert int(c.frame.max() - c.frame.min()) + 1 == 2 ** 20 - 2 and te.rank_bits(c.frame) == 12
    c = cs["id_bits/span_2p20m1_refused"]
    assert int(c.frame.max() - c.frame.min()) + 1 == 2 ** 20 - 1 and te.rank_bits(c.frame) is None


@pytest.mark.parametrize("E", (te.RS_TILE, te.RS_TILE + 1))
def test_frame_order_reach(E):
    c = te.cases()["frame_order/E%d" % E]
    assert c.E == E and not c.monotone and c.expected_tail() == 0
    assert any(len(set(f.tolist())) == 2 for _, _, f, _ in c.calls)
    runs = [int(c.frame[lo]) for lo, _ in c.run_bounds()]
    assert runs == [900, 41, 40, 3, 40, 17]              # descending, A B A, gaps
    np.testing.assert_array_equal(te.ids_round_trip(c.frame, te.rank_bits(c.frame)), np.arange(E))


def test_cold_store_reach():
    cs = te.cases()
    assert [lo for lo, _ in cs["cold_store/offsets"].call_bounds()] == [0, 1, 2, 3, 5, 4097]
    c = cs["cold_store/null_fields"]
    opt = c.optional()
    assert c.bare[5:12].all() and not c.bare[:5].any() and not c.bare[12:].any()
    assert all(not v[5:12].any() and v[:5].all() and v[12:].all() for v in opt.values())
    lo, hi = te.block_switch_sizes()
    assert te.desc_block_total(lo) <= te.BLOCK_MAX < te.desc_block_total(hi) and hi == lo + 1
    assert [b - a for a, b in cs["cold_store/block_switch"].call_bounds()] == [lo, hi]


def test_degenerate_reach():
    c = te.cases()["degenerate/cell_zero"]
    k = c.structure()[0]
    assert np.sum(c.side < 0) >= 7 and k.min() == 0 and np.all(np.trunc(c.side + 0.5) >= 0)


def test_optional_fields_are_distinct_bit_patterns():
    c = te.cases()["sort_counts/E4097"]
    for v in c.optional().values():
        assert len(np.unique(v)) == v.size


# ---- mutants --------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("mutant, caught_by", [
    ("unstable", "sort_counts/E257"), ("tile_drop", "sort_counts/E4096"), ("low48", "digit_skip/top_byte_only"),
    ("heads_shifted", "scan_counts/E2049_between")])
def test_mutants_of_the_sort_are_caught(mutant, caught_by, oracle_of):
    c = te.cases()[caught_by]
    _, dump = oracle_of(caught_by)
    assert not _differs(c.structure(), dump)
    assert _differs(te.structure_vec(c.side, c.label, c.frame, mutant), dump)
    caught = [n for n in NAMES if te.cases()[n].E <= 9000 and
              _differs(te.structure_vec(te.cases()[n].side, te.cases()[n].label, te.cases()[n].frame, mutant), te.cases()[n].structure())]
    assert caught_by in caught and len(caught) >= 2


def test_rank_bits_fixed_at_13_are_caught(oracle_of, oracle_mod):
    """the census' rough and match lists name entries through their 32-bit ids: with the ids built from 13 rank bits whatever the
    table needs, the lists of the id_bits workloads name other entries than the oracle's"""
    caught = []
    for n in NAMES:
        c = te.cases()[n]
        if c.E == 0 or n in te.REFUSED or not (n.startswith("id_bits") or c.E <= 300):
            continue
        o, _ = oracle_of(n)
        o.select(c.query_descs(oracle_mod, 0))
        want = o.rough_matches()["db_entry"]
        assert len(want) > 0, n
        np.testing.assert_array_equal(te.ids_round_trip(c.frame, te.rank_bits(c.frame))[want], want, err_msg=n)
        if not np.array_equal(te.ids_round_trip(c.frame, 13)[want], want):
            caught.append(n)
    assert {"id_bits/frame_of_8193", "id_bits/span_600000", "id_bits/span_2p20m2"} <= set(caught)
    assert "id_bits/frame_of_8192" not in caught
