"""The workloads of tests/_order_edges.py reach their edges: shown on the CPU with the restatement of the ordering
(home keys, stable order, group heads) and with the oracle alone.  The GPU side is tests/test_gpu_order_edges.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _order_edges as oe  # noqa: E402


@pytest.fixture(scope="module")
def tg():
    T, G = oe.tiles()
    assert T >= 1024 and G >= 1024 and T % 64 == 0 and G % 64 == 0
    return T, G


@pytest.fixture(scope="module")
def oracle_mod():
    from oracle import oracle
    oracle.build_library()
    return oracle


def _model(name, T, G):
    wl, n = oe.case(name, T, G)
    side, label, _ = wl.sets[0]
    assert len(side) == n
    return oe.model(side, label), n


def test_the_keys_are_32_bits_and_the_wide_setting_is_not():
    assert 12 + 3 * oe.CBITS + oe.SUB_BITS == 32 and 12 + 3 * oe.CBITS + oe.WIDE_SUB_BITS > 32


def test_counts_sit_around_both_tiles(tg):
    T, G = tg
    want = (1, T - 1, T, T + 1, 3 * T + 1, G - 1, G, G + 1, 3 * G + 1)
    assert tuple(oe.count_of(c, T, G) for c in oe.COUNTS) == want
    for c, n in zip(oe.COUNTS, want):
        assert "count " + c in oe.CASES
        m, got = _model("count " + c, T, G)
        assert got == n and (n == 1 or 1 < m["n_groups"] < n)
        assert not np.array_equal(m["order"], np.arange(n)) or n == 1      # (the slots are not handed in sorted)
    assert oe.count_of(oe.deep(T, G).split()[1], T, G) > 3 * max(T, G)


def test_one_cell_and_own_cells(tg):
    T, G = tg
    m, n = _model("one cell", T, G)
    assert n > 2 * G and n > T and m["n_groups"] == 1 and len(set(m["keys"].tolist())) == 1
    m, n = _model("own cells", T, G)
    assert n > 2 * G and n > T and m["n_groups"] == n and not m["marker"].any()


@pytest.mark.parametrize("b", [-1, 0, 1])
def test_group_boundary_on_the_tile_boundary(tg, b):
    T, G = tg
    m, n = _model("boundary %d" % b, T, G)
    for stop in (G + b, T + b):
        assert n > stop + 1 and m["heads"][stop] and not m["heads"][stop + 1]
    assert not m["marker"].any()


def test_marker_keys_straddle_both_boundaries(tg):
    T, G = tg
    m, n = _model("markers", T, G)
    k = len(oe.MARKER_SIDES)
    for at in sorted({T, G}):
        run = slice(at - 3, at - 3 + k)
        assert m["marker"][run].all() and m["heads"][run].all() and m["heads"][at - 3 + k]
        assert not m["marker"][at - 4] and not m["marker"][at - 3 + k]
        assert m["sorted"][at - 1] == m["sorted"][at]                       # equal keys on both sides of the boundary
        assert m["sorted"][at + 1] == m["sorted"][at + 2] == m["sorted"][at + 3]   # ... and adjacent behind it
    # a side of at least 2^cbits - 1 cells and a side whose side - 1 truncates below 0 both take the marker
    assert oe.home_coord(70.3) == oe.CMASK and oe.home_coord(0.0) == oe.CMASK and oe.home_coord(1e-17) == oe.CMASK
    assert oe.home_coord(0.4) == 0 and oe.home_coord(62.9) == 62


def test_single_digit_keys(tg):
    T, G = tg
    m, n = _model("top digit", T, G)
    assert n > T and len(set((m["keys"] & np.uint64(0xFFFFFF)).tolist())) == 1 and len(set((m["keys"] >> np.uint64(24)).tolist())) == 64
    m, n = _model("low digit", T, G)
    assert n > T and len(set((m["keys"] >> np.uint64(8)).tolist())) == 1 and len(set((m["keys"] & np.uint64(255)).tolist())) == 240
    # many equal keys: the stable order keeps them in slot order
    eq = m["sorted"][1:] == m["sorted"][:-1]
    assert eq.sum() > n // 2 and (m["order"][1:][eq] > m["order"][:-1][eq]).all()


def test_every_case_has_candidates_and_matches(tg, oracle_mod):
    T, G = tg
    for name in oe.CASES:
        ans = oe.expected(oracle_mod, name, T, G)
        wl, n = oe.case(name, T, G)
        assert ans["D"] == n and ans["M"] > 0 and ans["P"] >= ans["M"], name
        assert len(ans["cand_frame"]) >= 1 or n == 1, name


def test_ragged_batch_has_empty_frames_between_full_ones(oracle_mod):
    from sgtd_amd import synth
    m, xyz, label, off = oe.ragged_world(synth)
    o = oracle_mod.OracleManager()
    counts = [o.build(xyz[off[i]:off[i + 1]], label[off[i]:off[i + 1]], export=False) for i in range(len(oe.RAGGED))]
    assert counts[0] > 0 and counts[1] == 0 and counts[2] == 0 and counts[3] > 0 and counts[4] == 0 and counts[6] == 0
    assert len(counts) * max(counts) >= 2 * sum(counts)          # the descriptor slots are several times the descriptors
