"""build_frames_kernel's neighbour selection at its edges, against the oracle, bit for bit: descriptors and counts of
every frame of tests/_knn_edges.py — n = K, K + 1, 2K - 1, 2K, 2K + 1, 4K + 3, 41, 200 and K - 1 keypoints; exact ties
from lattices, collinear points, duplicates, and a tie exactly at the K-th place — for every descriptor_near_num that
selects another network size (4, 8, 10, 12, 16) and in both dedup forms.  A batch is one launch whose largest frame
decides the form for all its frames, so every frame is far smaller than its batch's largest.  That the oracle equals the
numpy restatement on these frames, and that the frames hold their ties, is tests/test_knn_edges.py (no GPU)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _build_edges as be  # noqa: E402
import _knn_edges as ke  # noqa: E402

pytestmark = pytest.mark.gpu

_EXPECT = {}


def expected(K, fr):
    """the oracle's descriptors of one frame, once (the two forms share most frames)"""
    from oracle import oracle
    oracle.build_library()
    if (K, id(fr)) not in _EXPECT:
        _EXPECT[(K, id(fr))] = oracle.OracleManager(**ke.cfg_of(K)).build(*fr)
    return _EXPECT[(K, id(fr))]


@pytest.mark.parametrize("form", ("lds", "global"))
@pytest.mark.parametrize("K", ke.KS)
def test_batch_equals_the_oracle(K, form):
    """one sgtd_add_frames call; the table's entries in insertion order are the frames' descriptors, frame ids 0, 1, ..."""
    from sgtd_amd import manager
    cases = ke.all_batches()[(K, form)]
    frames = [fr for _, _, fr in cases]
    want = [expected(K, fr) for fr in frames]
    g = manager.STDescManager(**ke.cfg_of(K))
    xyz, lab, off = be.batch_of(frames)
    g.add_frames(xyz, lab, kp_off=off)
    total = sum(d.n for d in want)
    assert total > 100 * K
    assert g.stats()["n_entries"] == total, (K, form)
    ent = g.fetch_entries(np.arange(total, dtype=np.int64))
    at = 0
    for k, ((n, kind, _), d) in enumerate(zip(cases, want)):
        got = ent.take(np.arange(at, at + d.n))
        fields = tuple(f for f in be.RefBuild.FIELDS if f != "frame")
        assert be.desc_bits_equal(got, d, fields) == "", "K=%d %s frame %d: n=%d %s" % (K, form, k, n, kind)
        assert np.all(got.frame[:got.n] == k), (K, form, k)
        at += d.n
    g.close()


@pytest.mark.parametrize("K", (10, 16))
def test_one_frame_at_a_time(K):
    """sgtd_build: a launch per frame, the frame its own batch's largest"""
    from sgtd_amd import manager
    g = manager.STDescManager(**ke.cfg_of(K))
    for n, kind, fr in ke.all_batches()[(K, "global")]:
        got, d = g.BuildSingleScanSTD(*fr), expected(K, fr)
        fields = tuple(f for f in be.RefBuild.FIELDS if f != "frame")
        assert be.desc_bits_equal(got, d, fields) == "", "K=%d n=%d %s" % (K, n, kind)
    g.close()
