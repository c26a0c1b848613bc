"""sgtd_scan_keypoints without a device: the declarations, the default config, the argument checks, and the properties
of the rule's numpy restatement against a literal restatement of the reference's sweep (tests/_scan_ref.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _scan_ref as ref
from sgtd_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLS = {
    "sgtd_scan_config_check": ["const sgtd_scan_config *cfg", "const char **why"],
    "sgtd_scan_keypoints": ["sgtd_handle h", "const sgtd_scan_config *cfg", "const float *points", "int stride_floats",
                            "const uint32_t *labels", "const int64_t *pt_off", "int n_scans", "int device_ptrs"],
    "sgtd_result_scan_keypoints": ["sgtd_handle h", "int64_t *kp_off", "float *xyz", "uint32_t *label", "int32_t *n_points",
                                   "int64_t capacity", "int64_t *n_keypoints"],
    "sgtd_result_scan_point_clusters": ["sgtd_handle h", "int scan", "int32_t *cluster", "int64_t capacity", "int64_t *n"],
    "sgtd_result_scan_grids": ["sgtd_handle h", "int scan", "int32_t *grid", "double *range"],
    "sgtd_scan_device_view": ["sgtd_handle h", "const float **d_xyz", "const uint32_t **d_label"],
}

SCENES = [(3, 600), (4, 900), (5, 1500), (6, 2500)]      # (stream, points): random blob scenes of this file


def header():
    return open(os.path.join(ROOT, "include", "sgtd_accel.h")).read()


def test_header_declares_the_calls():
    h = header()
    for name, want in DECLS.items():
        m = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, h)
        assert m, name + " is not declared"
        text = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
        assert [" ".join(a.split()) for a in text.split(",")] == want, name
    assert re.search(r"void\s+sgtd_default_scan_config\s*\(\s*sgtd_scan_config \*cfg\s*\)\s*;", h)
    assert re.search(r"void\s+sgtd_scan_tiles\s*\(\s*int \*point_tile\s*\)\s*;", h)
    assert re.search(r"^#define\s+SGTD_SCAN_MAX_CLASSES\s+32\b", h, re.M)
    body = re.search(r"typedef struct sgtd_scan_config \{(.*?)\} sgtd_scan_config;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["int32_t node_label[SGTD_SCAN_MAX_CLASSES]", "int32_t min_seg[SGTD_SCAN_MAX_CLASSES]", "int32_t min_instance_points",
                      "int32_t reserved", "double start_r, delta_r, delta_p, delta_a", "double min_range, max_range"]


def test_binding_declares_the_calls():
    for name in list(DECLS) + ["sgtd_default_scan_config", "sgtd_scan_tiles"]:
        assert name in _lib.SYMBOLS, name
    L = _lib.lib()
    for name, want in DECLS.items():
        assert len(getattr(L, name).argtypes) == len(want), name
        assert getattr(L, name).restype is ctypes.c_int
    assert ctypes.sizeof(_lib.ScanConfig) == 32 * 4 * 2 + 8 + 6 * 8
    tile = ctypes.c_int(0)
    L.sgtd_scan_tiles(ctypes.byref(tile))
    assert tile.value > 0 and tile.value % 64 == 0


def test_default_config():
    c = _lib.ScanConfig()
    _lib.lib().sgtd_default_scan_config(ctypes.byref(c))
    want = ref.default_cfg()
    assert list(c.node_label) == want["node_label"].tolist() == [0] * 10 + list(range(3, 12)) + [0] * 13
    assert list(c.min_seg) == want["min_seg"].tolist()
    assert [c.min_seg[s] for s in (15, 17, 18)] == [5, 5, 5] and sum(1 for v in c.min_seg if v == 300) == 29
    assert c.min_instance_points == 20 and c.reserved == 0
    assert (c.start_r, c.delta_r, c.delta_p, c.delta_a, c.min_range, c.max_range) == (0.35, 0.0004, 1.2, 1.2, 0.5, 120.0)


def cfg_with(**kw):
    c = _lib.ScanConfig()
    _lib.lib().sgtd_default_scan_config(ctypes.byref(c))
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(c, k)[v[0]] = v[1]
        else:
            setattr(c, k, v)
    return c


BAD_CONFIGS = [dict(start_r=0.0), dict(start_r=float("nan")), dict(start_r=float("inf")), dict(delta_r=-1e-6), dict(delta_r=float("nan")),
               dict(delta_p=0.0), dict(delta_p=-1.2), dict(delta_a=0.0), dict(delta_a=float("inf")), dict(min_range=0.0),
               dict(max_range=float("inf")), dict(min_range=120.0), dict(min_range=130.0), dict(node_label=(3, -1)),
               dict(min_seg=(15, -1)), dict(min_instance_points=-1)]


@pytest.mark.parametrize("kw", BAD_CONFIGS, ids=lambda kw: "%s=%s" % next(iter(kw.items())))
def test_invalid_configs_return_without_a_device(kw):
    L = _lib.lib()
    c = cfg_with(**kw)
    assert L.sgtd_scan_config_check(ctypes.byref(c), None) == -1
    # ... and so does the call itself, whatever else it was given (no handle exists without a device)
    off = np.zeros(1, np.int64)
    assert L.sgtd_scan_keypoints(None, ctypes.byref(c), None, 3, None, off.ctypes.data_as(ctypes.c_void_p), 0, 0) == -1


def test_null_handle_and_bad_arguments_are_invalid():
    L = _lib.lib()
    off = np.array([0, 4, 2], np.int64)
    po = off.ctypes.data_as(ctypes.c_void_p)
    n = ctypes.c_int64(0)
    assert L.sgtd_scan_keypoints(None, None, None, 3, None, po, 0, 0) == -1
    assert L.sgtd_scan_keypoints(None, None, None, 3, None, po, -1, 0) == -1
    assert L.sgtd_scan_keypoints(None, None, None, 5, None, po, 0, 0) == -1
    assert L.sgtd_scan_keypoints(None, None, None, 3, None, None, 0, 0) == -1
    assert L.sgtd_scan_keypoints(None, None, None, 3, None, po, 2, 0) == -1
    assert L.sgtd_result_scan_keypoints(None, None, None, None, None, 0, ctypes.byref(n)) == -1
    assert L.sgtd_result_scan_point_clusters(None, 0, None, 0, ctypes.byref(n)) == -1
    assert L.sgtd_result_scan_grids(None, 0, None, None) == -1
    assert L.sgtd_scan_device_view(None, None, None) == -1


def test_ring_envelope():
    L = _lib.lib()
    why = ctypes.c_char_p()
    assert L.sgtd_scan_config_check(None, ctypes.byref(why)) == 0 and why.value == b""
    assert L.sgtd_scan_config_check(ctypes.byref(cfg_with()), None) == 0
    # the defaults need 466 rings: the increments 0.35 - s * 0.0004 sum to max_range - min_range = 119.5 m there (470 reach 120 m)
    inc = 0.35 - np.arange(1, 1025) * 0.0004
    assert int(np.argmax(np.cumsum(inc) >= 119.5)) + 1 == 466 and np.all(inc[:470] > 0.0)
    # delta_r = 0.01: the increments turn negative at s = 35, long before they cover the range
    assert L.sgtd_scan_config_check(ctypes.byref(cfg_with(delta_r=0.01)), ctypes.byref(why)) == -6 and b"rings" in why.value
    assert L.sgtd_scan_config_check(ctypes.byref(cfg_with(delta_r=0.0)), None) == 0            # 342 rings of 0.35 m
    assert L.sgtd_scan_config_check(ctypes.byref(cfg_with(start_r=0.1, delta_r=0.0)), None) == -6   # 1195 rings
    assert L.sgtd_scan_config_check(ctypes.byref(cfg_with(delta_a=0.3)), ctypes.byref(why)) == -6 and b"azimuth" in why.value
    assert L.sgtd_scan_config_check(ctypes.byref(cfg_with(delta_p=0.1)), ctypes.byref(why)) == -6 and b"pitch" in why.value


def scene(stream, n, **kw):
    p, l, _ = synth.make_scans(1, n, stream=stream, n_blobs=12, stray=0.0, **kw)
    assert ref.clear_of_boundaries(p, l)
    return p, l


def partition(labels):
    """a labelling as a set of frozensets of point indices"""
    return {frozenset(np.nonzero(labels == v)[0].tolist()) for v in np.unique(labels)}


@pytest.mark.parametrize("stream,n", SCENES)
def test_sweep_refines_the_components(stream, n):
    p, l = scene(stream, n, sigma=(0.3, 0.9))
    for cls in np.unique(l & 0xFFFF):
        m, vox, dims = ref.voxel_mode_points(p, l, int(cls))
        comp = ref.components(vox, *dims)
        sw = ref.sweep(vox, dims)
        for v in np.unique(sw):
            assert len(np.unique(comp[sw == v])) == 1, "a sweep cluster spans two components"
        assert len(np.unique(sw)) >= len(np.unique(comp))


def planted_three_voxels():
    """three voxels of one ring and pitch layer at the azimuth seam, cells A = 1, C = 300, B = 0 in that order.  B's
    neighbours include C (ax < 0 -> width - 1, :376) but C's do not include B (:377).  The sweep centres A and labels A
    and B, centres C and finds no one, and never expands B, which an earlier centre labelled (:288): {A, B}, {C}."""
    az = np.deg2rad(np.array([1.2, 0.0, 0.3]))
    r = 19.85
    pts = np.stack([r * np.cos(az), r * np.sin(az), np.zeros(3)], axis=1).astype(np.float32)
    lab = np.full(3, 15, np.uint32)
    return pts, lab


SEAM_ORDER = np.array([2, 0, 1])      # B first: it reaches A and C, the sweep finds the one cluster


def test_planted_scene_splits_under_the_sweep():
    p, l = planted_three_voxels()
    assert ref.clear_of_boundaries(p, l)
    m, vox, dims = ref.voxel_mode_points(p, l, 15)
    assert vox[:, 2].tolist() == [1, 300, 0] and dims[1] == 301 and len(set(map(tuple, vox[:, :2]))) == 1
    assert len(np.unique(ref.components(vox, *dims))) == 1
    sw = ref.sweep(vox, dims)
    assert sw[0] == sw[2] != sw[1]
    order = SEAM_ORDER
    assert len(np.unique(ref.sweep(vox[order], dims))) == 1
    cfg = ref.default_cfg()
    cfg["min_seg"] = cfg["min_seg"].copy()
    cfg["min_seg"][15] = 3
    assert ref.scan_rule(p, l, cfg)["n_points"].tolist() == [3]


@pytest.mark.parametrize("stream,n", SCENES[:2])
def test_rule_is_permutation_invariant(stream, n):
    p, l = scene(stream, n, sigma=(0.3, 0.9))
    cfg = ref.default_cfg()
    cfg["min_seg"] = np.full(32, 1, np.int64)
    base = ref.scan_rule(p, l, cfg)
    perm = np.random.default_rng(stream).permutation(n)
    again = ref.scan_rule(p[perm], l[perm], cfg)
    back = np.empty(n, np.int64)
    back[perm] = np.arange(n)
    mine = {(int(base["label"][c]), frozenset(np.nonzero(base["cluster"] == c)[0].tolist())) for c in range(len(base["label"]))}
    theirs = {(int(again["label"][c]), frozenset(perm[np.nonzero(again["cluster"] == c)[0]].tolist())) for c in range(len(again["label"]))}
    assert mine == theirs and len(mine) > 0


def test_sweep_depends_on_the_order():
    p, l = planted_three_voxels()
    m, vox, dims = ref.voxel_mode_points(p, l, 15)
    a = partition(ref.sweep(vox, dims))
    order = SEAM_ORDER
    b = {frozenset(int(order[i]) for i in s) for s in partition(ref.sweep(vox[order], dims))}
    assert a != b
    comp = lambda v: partition(ref.components(v, *dims))
    assert comp(vox) == {frozenset(int(order[i]) for i in s) for s in comp(vox[order])}


def test_fixed_sum_is_the_256_accumulator_fold():
    v = np.random.default_rng(1).normal(0.0, 30.0, 1000)
    acc = [0.0] * 256
    for k, x in enumerate(v):
        acc[k % 256] = acc[k % 256] + x
    w = 128
    while w >= 1:
        for i in range(w):
            acc[i] = acc[i] + acc[i + w]
        w //= 2
    assert ref.fixed_sum(v) == acc[0]


def test_read_scan_round_trip(tmp_path):
    from sgtd_amd import ingest
    p, l, _ = synth.make_scans(1, 100, stream=2)
    p.tofile(tmp_path / "a.bin")
    l.tofile(tmp_path / "a.label")
    q, m = ingest.read_scan(str(tmp_path / "a.bin"), str(tmp_path / "a.label"))
    assert np.array_equal(p, q) and np.array_equal(l, m) and q.shape == (100, 4)
    l[:50].tofile(tmp_path / "b.label")
    with pytest.raises(ValueError):
        ingest.read_scan(str(tmp_path / "a.bin"), str(tmp_path / "b.label"))
