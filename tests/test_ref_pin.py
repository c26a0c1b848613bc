"""The pin against the reference's own code (CPU, no GPU): oracle/_ref/libsgtd_ref_pin.so holds
Combinatorial_Binary_Encoding (STDesc.cpp:3-16), VOXEL_LOC / STDesc_LOC with their operator==
and std::hash (STDesc.h:126-154,217-250) and the constants (STDesc.h:31-33), cut out of the
reference by line range and compiled verbatim (oracle/Makefile, oracle/ref_pin.cpp).  Its answers
for the inputs below are stored in tests/golden/ref_pin/answers.npz (tests/golden/make_ref_pin.py),
so the pin holds where the reference checkout is not readable.  Checked here: the oracle's
restatements AND the product's key helpers (the inline functions the kernels use,
include/sgtd_accel.h) agree with it — rows a7, a5, a8 and a12's constants of SURVEY.md §8a — and,
where the library is built, the stored answers are still its answers.
The rest of the reference's path cannot be compiled in this image (Eigen/PCL/ROS/Ceres)."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np

from oracle import oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_spec = importlib.util.spec_from_file_location("make_ref_pin", os.path.join(HERE, "golden", "make_ref_pin.py"))
pin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pin)
GOLD = dict(np.load(pin.PATH))
REF = orc.ref_pin()         # the reference's code itself, where oracle/_ref was built


def _product():
    from sgtd_amd import _lib
    _lib.build_library()
    L = C.CDLL(_lib.LIB_PATH)     # the key helpers need no device
    L.sgtd_label_code.argtypes = [C.c_int] * 3
    L.sgtd_label_code.restype = C.c_uint32
    L.sgtd_table_key.argtypes = [C.c_uint32] * 4
    L.sgtd_table_key.restype = C.c_uint64
    L.sgtd_dedup_key.argtypes = [C.c_uint64] * 3
    L.sgtd_dedup_key.restype = C.c_uint64
    return L


def _reference_source():
    """the reference file oracle/Makefile builds the pin from (its REF, which the environment may override)"""
    ref = os.environ.get("REF") or re.search(r"^REF \?= (.*)$", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M).group(1)
    return os.path.join(ref.strip(), "src", "STDesc.cpp")


def test_ref_pin_is_built_where_the_reference_is():
    if os.path.exists(_reference_source()):
        assert REF is not None, "run `make -C oracle` (or __graft_entry__.build())"
    if REF is not None:
        live = pin.answers(REF, GOLD)
        for k, v in live.items():
            np.testing.assert_array_equal(v, GOLD[k], err_msg="%s: rerun tests/golden/make_ref_pin.py" % k)


def test_constants_are_the_references():
    assert tuple(GOLD["constants"]) == (116101, 10000000000, 20000)
    from sgtd_amd import _lib
    cfg = _lib.Config()
    _product().sgtd_default_config(C.byref(cfg))
    assert cfg.max_frame_n == GOLD["constants"][2]


def test_label_code_all_inputs_and_wraps():
    P, O = _product(), orc.lib()
    # every (a, b, c) in 0..15, the known answers of SURVEY §8c, and wrap cases: negative labels,
    # labels beyond 15 (the wild label map), INT_MIN / INT_MAX
    cases = GOLD["labels"]
    assert len(cases) == 16 ** 3 + 2000 + 10 ** 3
    for (a, b, c), r in zip(cases.tolist(), GOLD["label_code"].tolist()):
        assert O.orc_label_code(a, b, c) == r, (a, b, c)
        assert P.sgtd_label_code(a, b, c) == r, (a, b, c)
    assert O.orc_label_code(3, 10, 11) == P.sgtd_label_code(3, 10, 11) == 939
    assert O.orc_label_code(17, 5, -1) == P.sgtd_label_code(17, 5, -1) == 351


def test_table_key_equality_and_hash():
    """STDesc_LOC: equality on (x, y, z, a) only — b, c never matter (STDesc.h:235)"""
    P, O = _product(), orc.lib()
    n = len(GOLD["loc_k1"])
    ps, qs = pin.loc_pairs(GOLD)
    for p, q, r in zip(ps, qs, GOLD["loc_eq"].tolist()):
        p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
        assert O.orc_cell_key_eq(p.ctypes.data, q.ctypes.data) == r
        same = P.sgtd_table_key(int(p[3]), int(p[0]), int(p[1]), int(p[2])) == P.sgtd_table_key(int(q[3]), int(q[0]), int(q[1]), int(q[2]))
        assert int(same) == r, (p, q)
    assert int(GOLD["loc_eq"].sum()) > n // 4 + n
    for p, h in zip(pin.loc_keys(GOLD), GOLD["loc_hash"].tolist()):
        p = np.ascontiguousarray(p)
        assert O.orc_cell_key_hash(p.ctypes.data) == h, p
    # the code field is Combinatorial_Binary_Encoding of the ordered labels (STDesc.cpp:161,365)
    for (la, lb, lc), code in zip(GOLD["loc_labels"].tolist(), GOLD["loc_label_code"].tolist()):
        assert P.sgtd_table_key(P.sgtd_label_code(la, lb, lc), 1, 2, 3) == P.sgtd_table_key(code, 1, 2, 3)


def test_dedup_key_equality_and_hash():
    """VOXEL_LOC of the millimetre sides (STDesc.cpp:244-251)"""
    P, O = _product(), orc.lib()
    ps, qs = pin.voxel_pairs(GOLD)
    for p, q, r, h in zip(ps, qs, GOLD["voxel_eq"].tolist(), GOLD["voxel_hash"].tolist()):
        p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
        assert O.orc_milli_key_eq(p.ctypes.data, q.ctypes.data) == r
        same = P.sgtd_dedup_key(int(p[0]), int(p[1]), int(p[2])) == P.sgtd_dedup_key(int(q[0]), int(q[1]), int(q[2]))
        assert int(same) == r, (p, q)
        assert O.orc_milli_key_hash(p.ctypes.data) == h, p
