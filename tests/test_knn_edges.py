"""The frames of tests/test_gpu_knn_edges.py, checked without a GPU: the numpy restatement of the neighbour selection
(tests/_knn_edges.knn_ref) and the oracle agree on every generated frame — the descriptors that follow from the
restatement's neighbour lists (tests/_build_edges.ref_build, whose own selection is checked against knn_ref here) equal
the oracle's bit for bit — and the frames hold the ties and the sizes they are named after."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _build_edges as be  # noqa: E402
import _knn_edges as ke  # noqa: E402


def _frames(K):
    """every different frame of K's two batches"""
    seen, out = set(), []
    for form in ("lds", "global"):
        for n, kind, fr in ke.all_batches()[(K, form)]:
            if id(fr) not in seen:
                seen.add(id(fr))
                out.append((n, kind, fr))
    return out


@pytest.mark.parametrize("K", ke.KS)
def test_restatement_and_oracle_agree_on_every_frame(K, oracle_mod):
    cfg = ke.cfg_of(K)
    o = oracle_mod.OracleManager(**cfg)
    n_desc = 0
    for n, kind, (xyz, lab) in _frames(K):
        assert len(xyz) == n
        r = be.ref_build(xyz, lab, cfg)
        if n >= K:
            assert np.array_equal(r.nn, ke.knn_ref(xyz, K)[0]), (K, n, kind)
        assert be.desc_bits_equal(r, o.build(xyz, lab)) == "", (K, n, kind)
        assert n >= K or r.n == 0, (K, n, kind)
        n_desc += r.n
    assert n_desc > 100 * K


@pytest.mark.parametrize("K", ke.KS)
def test_frames_hold_their_sizes_and_ties(K):
    by_kind = {}
    for n, kind, (xyz, _) in _frames(K):
        by_kind.setdefault(kind, []).append((n, xyz))
    want = set(ke.sizes(K))
    assert want == {K, K + 1, 2 * K - 1, 2 * K, 2 * K + 1, 4 * K + 3, 41, 200} and len(want) >= 7
    assert {n for n, _ in by_kind["random"]} >= want | {K - 1}
    for kind in ("lattice", "duplicates"):
        assert {n for n, _ in by_kind[kind]} == want
    assert {n for n, _ in by_kind["collinear"]} == want - {ke.LARGE}
    assert {n for n, _ in by_kind["kth_tie"]} == want - {K, ke.LARGE}
    for n, xyz in by_kind["random"]:
        if K <= n <= ke.LARGE:
            assert ke.tie_stats(xyz, K) == (0, 0), n
    for kind in ("lattice", "collinear", "duplicates"):
        for n, xyz in by_kind[kind]:
            assert ke.tie_stats(xyz, K)[0] >= (2 if kind == "duplicates" else n // 2), (kind, n)
    # a tie exactly at the K-th place: in every kth_tie frame, and in the lattices (n > K)
    for n, xyz in by_kind["kth_tie"]:
        assert ke.tie_stats(xyz, K)[1] >= 1, n
    assert sum(ke.tie_stats(xyz, K)[1] for n, xyz in by_kind["lattice"] if n > K) >= 20
    # tied neighbours in different quarters of the candidate range (the kernel's four threads per keypoint)
    if be.parts_of(K) == 4:
        split = 0
        for n, xyz in by_kind["lattice"] + by_kind["kth_tie"]:
            idx, near = ke.knn_ref(xyz, K)
            for i in range(n):
                for k in range(1, K):
                    if near[i, k] == near[i, k - 1] and be.quarter_of(int(idx[i, k]), n) != be.quarter_of(int(idx[i, k - 1]), n):
                        split += 1
        assert split >= 50


@pytest.mark.parametrize("K", ke.KS)
def test_both_dedup_forms_have_small_frames_in_a_larger_batch(K):
    b = ke.all_batches()
    switch = be.lds_switch(K)
    for form, past in (("lds", False), ("global", True)):
        ns = [n for n, _, _ in b[(K, form)]]
        assert (max(ns) > switch) == past
        assert min(ns) == K - 1 and K in ns and sum(1 for n in ns if n < max(ns)) >= 20
        assert be.lds_bytes(max(ns), K, past is False) <= be.LDS_LIMIT
