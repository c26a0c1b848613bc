"""The inputs of tests/test_gpu_thin_edges.py, checked without a GPU: the constants tests/_thin_edges.py restates are the
sources'; every input reaches the count or boundary it exists for; the device pipeline restated in numpy (thin_model)
equals the rule restated (tests/_thin_ref.py) on every input; every wrong version of the pipeline (mutant) is caught by the
cases the table names, and every case but count-1 catches one; every perturbation of a long cell's index order changes the
output's bits; the closed form of `deep` equals the rule at a reduced size; and the rule restated equals
ingest.voxel_downsample cloud by cloud."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _thin_edges as te  # noqa: E402
import _thin_ref as tr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(te.cases())


def _src(*path):
    return open(os.path.join(ROOT, *path)).read()


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(.+?)\s*(?://.*|/\*.*)?$" % name, text, re.M)
    assert m, name
    return m.group(1).strip()


def test_constants_are_the_sources():
    table, thin = _src("sgtd_amd", "csrc", "table_kernels.hip.h"), _src("sgtd_amd", "csrc", "thin_kernels.hip.h")
    common, header, accel = _src("sgtd_amd", "csrc", "common.hip.h"), _src("include", "sgtd_accel.h"), _src("sgtd_amd", "csrc", "sgtd_accel.hip")
    assert int(_define(table, "SGTD_RS_THREADS")) == te.RS_ROUND
    assert int(_define(table, "SGTD_RS_ROUNDS")) * te.RS_ROUND == te.RS_TILE and _define(table, "SGTD_RS_TILE") == "(SGTD_RS_THREADS * SGTD_RS_ROUNDS)"
    assert int(_define(table, "SGTD_SCAN_THREADS")) * int(_define(table, "SGTD_SCAN_ITEMS")) == te.SCAN_BLOCK
    assert "(u32)(k >> shift) & 255u" in table and "shift += 8" in accel and te.DIGIT == 8
    assert int(_define(common, "SGTD_WAVE")) == te.WAVE
    assert _define(header, "SGTD_REG_MAX_CLOUDS") == "(1 << 16)" and te.MAX_CLOUDS == 1 << 16
    assert _define(header, "SGTD_THIN_MAX_CELL") == "(1 << 20)" and te.MAX_CELL == 1 << 20 == tr.MAX_CELL
    assert int(_define(thin, "SGTD_THIN_CELL_BITS")) == te.CELL_BITS and _define(thin, "SGTD_THIN_DROP_KEY") == "0x7FFFFFFFFFFFFFFFull"
    assert te.DROP_KEY == 0x7FFFFFFFFFFFFFFF
    assert "key = (ux << (2 * SGTD_THIN_CELL_BITS)) | (uy << SGTD_THIN_CELL_BITS) | uz;" in thin
    # the thin kernels: 256 threads a workgroup, but thin_offsets_kernel, which is launched with 256
    assert len(re.findall(r"__launch_bounds__\(256\) void thin_\w+_kernel", thin)) == 5 and te.THIN_BLOCK == 256
    assert len(re.findall(r"blockIdx\.x \* 256u? \+ threadIdx\.x", thin)) == 5 and "grid_for(S + 1, 256), 256" in accel
    # what thin_run hands the sorts and the scans
    assert "radix_sort_pairs<u64>(e, kin, kout, vin, vout, P, 3 * SGTD_THIN_CELL_BITS, false)" in accel
    assert "radix_sort_pairs<u32>(e, ckin, ckout, vin, vout, P, key_bits((u64)S), false)" in accel
    assert "device_scan(e, flags, excl, P + 1)" in accel and "device_scan(e, first, first_excl, P + 1)" in accel
    assert "int key_bits(u64 v) { int b = 0; while (v) { b++; v >>= 1; } return std::max(b, 1); }" in accel
    assert [te.key_bits(v) for v in (0, 1, 255, 256, 65535, 65536)] == [1, 1, 8, 9, 16, 17]


def test_the_cases_the_issue_names_are_there():
    want = ["count-%d" % n for n in (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)]
    want += ["digit-%d" % d for d in range(8)] + ["cloud-digit-%d" % b for b in range(3)] + ["clouds-%d" % s for s in (255, 256, 257, 65535, 65536)]
    want += ["empties-300", "empties-max", "boundary-4096", "boundary-2048", "long-cell-4097", "long-cell-8193", "long-cell-12289"]
    want += ["drops-" + k for k in ("all-1", "all-3", "first", "last-live", "live-4096-then", "live-8192-then", "then-live-4096", "then-live-8192", "corner")]
    assert sorted(want) == sorted(NAMES)
    assert set(te.EVERY_FORM) <= set(NAMES) and {"count-4097", "clouds-256", "long-cell-8193"} <= set(te.EVERY_FORM)
    assert any(n.startswith("drops-") for n in te.EVERY_FORM)
    assert {n.split("-")[0] for n in te.EVERY_FORM} == {n.split("-")[0] for n in NAMES}      # one of each family
    assert [n for n, _ in te.SEQUENCE] == ["count-8193", "count-63", "drops-all-3", "count-4097", "long-cell-4097", None, "count-8193"]


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_edge_and_the_pipeline_is_the_rule(name):
    c = te.cases()[name]
    pts, off, leaf, stride = c.input()
    assert pts.dtype == np.float32 and pts.shape == (off[-1], stride) and len(pts) <= 70000
    assert c.reaches(), name + " no longer reaches what it is for"
    want = c.want()
    got = te.thin_model(pts, off, leaf)
    assert te.same(got, want), name
    assert want["points"].shape[1] == stride and want["pt_off"][-1] == len(want["points"])


@pytest.mark.parametrize("name", te.MUTANTS)
def test_mutant_is_caught_by_its_cases(name):
    names = te.caught_by()[name]
    assert names, "no case is named for " + name
    for n in names:
        c = te.cases()[n]
        pts, off, leaf, _ = c.input()
        assert not te.same(te.thin_model(pts, off, leaf, **te.mutant(name)), c.want()), "%s does not catch %s" % (n, name)


def test_every_case_but_one_catches_a_mutant():
    assert set(te.caught_by()) == set(te.MUTANTS) and len(te.MUTANTS) == 23
    assert [n for n, c in te.cases().items() if not c.catches] == ["count-1"]


@pytest.mark.parametrize("N", te.LONG_N)
def test_long_cell_perturbations_change_the_bits(N):
    c = te.cases()["long-cell-%d" % N]
    pts, off, leaf, _ = c.input()
    want = c.want()
    assert len(te.long_run(pts)) == N
    for p in te.PERTURBATIONS:
        q = te.perturbation(p, N)
        assert sorted(q.tolist()) == list(range(N)) and (q != np.arange(N)).any(), p
        other = tr.thin(te.perturbed(pts, p), off, leaf)
        assert other["points"].shape == want["points"].shape, p
        assert not np.array_equal(te.bits(other["points"][:, 3]), te.bits(want["points"][:, 3])), "%s leaves the bits of long-cell-%d" % (p, N)


DEEP_SMALL = 141      # stands for SCAN_BLOCK: 141^2 points are about 20 000


@pytest.mark.parametrize("P", [DEEP_SMALL * DEEP_SMALL - 1, DEEP_SMALL * DEEP_SMALL])
def test_deep_closed_form_is_the_rule_at_a_reduced_size(P):
    (pts, off, leaf, stride), want = te.deep(P, scan_block=DEEP_SMALL, tile=283)
    assert te.deep_reaches(P, DEEP_SMALL) and len(pts) == P and off.size == 4
    ref = tr.thin(pts, off, leaf)
    assert te.same(want, ref)
    assert ref["n_dropped"][[0, 2]].min() > 0 and 1.5 < P / len(ref["points"]) < te.DEEP_PER_CELL      # (the clouds split cells)
    assert te.same(te.thin_model(pts, off, leaf), ref)


def test_deep_sizes_reach_the_second_level_of_the_scan():
    assert te.DEEP_P == (te.SCAN_BLOCK ** 2 - 1, te.SCAN_BLOCK ** 2) == ((1 << 22) - 1, 1 << 22)
    assert all(te.deep_reaches(P) for P in te.DEEP_P)
    assert (te.DEEP_P[1] + te.THIN_BLOCK - 1) // te.THIN_BLOCK == 16384      # the thin kernels' grids


def test_the_rule_restated_is_the_host_function_on_the_cases():
    from sgtd_amd import ingest
    seen = 0
    for name, c in te.cases().items():
        if c.has_out_of_range():
            continue
        pts, off, leaf, _ = c.input()
        want = c.want()
        for s in np.flatnonzero(np.diff(off)):
            host = ingest.voxel_downsample(pts[off[s]:off[s + 1]], leaf)
            a, b = want["pt_off"][s], want["pt_off"][s + 1]
            assert host.shape == want["points"][a:b].shape and np.array_equal(te.bits(host), te.bits(want["points"][a:b])), (name, s)
        empty = np.diff(off) == 0
        assert (np.diff(want["pt_off"])[empty] == 0).all(), name
        seen += 1
    assert seen >= 30
