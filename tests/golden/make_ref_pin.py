#!/usr/bin/env python3
"""Generates tests/golden/ref_pin/answers.npz: what the reference's own code answers for the inputs of tests/test_ref_pin.py.

oracle/_ref/libsgtd_ref_pin.so (oracle/Makefile, oracle/ref_pin.cpp) can only be built where the reference checkout is
readable.  This file stores its answers (the constants, Combinatorial_Binary_Encoding, STDesc_LOC's and VOXEL_LOC's
operator== and std::hash) beside the inputs they were computed for, so that the tests pin the oracle and the product
against the reference everywhere.  Where the library is built, the tests also check it against this file.

    make -C oracle && python tests/golden/make_ref_pin.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HERE = os.path.dirname(os.path.abspath(__file__))
# (a directory of its own: tests/golden/*.npz are the fixtures of tests/test_golden.py)
PATH = os.path.join(HERE, "ref_pin", "answers.npz")
# the corners of the 21-bit envelope of a VOXEL_LOC coordinate: every pair of them is compared
VOXEL_EDGE = np.array([[0, 0, 0], [2097151, 2097151, 2097151], [2097151, 0, 0], [0, 2097151, 0], [0, 0, 2097151]], np.int64)


def inputs():
    """the stored inputs, in the smallest integer type that holds them"""
    x = {}
    # label code: every (a, b, c) in 0..15, random triples with negative labels and labels beyond 15 (the wild label
    # map), and every triple of the wild values, INT_MIN / INT_MAX among them
    cases = [(a, b, c) for a in range(16) for b in range(16) for c in range(16)]
    rng = np.random.default_rng(7)
    wild = [-2147483648, -17, -16, -1, 16, 17, 31, 255, 4096, 2147483647]
    cases += [(int(a), int(b), int(c)) for a, b, c in rng.integers(-40, 60, size=(2000, 3))]
    cases += [(a, b, c) for a in wild for b in wild for c in wild]
    x["labels"] = np.array(cases, np.int32)
    # STDesc_LOC keys (x, y, z, a, b, c): small ranges (many equal pairs; a quarter equal in x, y, z, a with b, c
    # differing), and the envelope's cells; label triples whose code goes into the key's code field
    rng = np.random.default_rng(11)
    n = 20000
    k1 = rng.integers(0, 6, size=(n, 6))
    k2 = rng.integers(0, 6, size=(n, 6))
    k2[: n // 4, :4] = k1[: n // 4, :4]
    big = rng.integers(0, 65536, size=(n, 6))
    big[:, 3] = rng.integers(0, 4096, size=n)
    x["loc_k1"], x["loc_k2"], x["loc_big"] = k1.astype(np.int8), k2.astype(np.int8), big.astype(np.uint16)
    x["loc_labels"] = rng.integers(0, 16, size=(500, 3)).astype(np.int8)
    # VOXEL_LOC keys of millimetre sides (side <= 50 m) against a copy with one coordinate moved by 1 or 2 (or none)
    rng = np.random.default_rng(13)
    a = rng.integers(0, 50001, size=(n, 3))
    b = a.copy()
    flip = rng.integers(0, 4, size=n)
    for i in range(n):
        if flip[i] < 3:
            b[i, flip[i]] += int(rng.integers(1, 3))
    x["vox_a"], x["vox_step"] = a.astype(np.uint16), (b - a).astype(np.int8)
    return x


def loc_pairs(x):
    """(p, q) int64 key pairs: k1 against k2, every envelope cell against its neighbour and against itself"""
    k1, k2, big = (np.asarray(x[k], np.int64) for k in ("loc_k1", "loc_k2", "loc_big"))
    return np.concatenate([k1, big, big]), np.concatenate([k2, np.roll(big, 1, axis=0), big])


def loc_keys(x):
    """the distinct keys hashed: k1 and the envelope's cells"""
    return np.concatenate([np.asarray(x["loc_k1"], np.int64), np.asarray(x["loc_big"], np.int64)])


def voxel_pairs(x):
    """(p, q) int64 key pairs: a against a + step, then every pair of the envelope's corners"""
    e = len(VOXEL_EDGE)
    a = np.asarray(x["vox_a"], np.int64)
    return (np.concatenate([a, np.repeat(VOXEL_EDGE, e, axis=0)]),
            np.concatenate([a + np.asarray(x["vox_step"], np.int64), np.tile(VOXEL_EDGE, (e, 1))]))


def pairwise(fn, p, q):
    p, q = np.ascontiguousarray(p, np.int64), np.ascontiguousarray(q, np.int64)
    return np.array([fn(p[i].ctypes.data, q[i].ctypes.data) for i in range(len(p))], np.int8)


def keywise(fn, p):
    p = np.ascontiguousarray(p, np.int64)
    return np.array([fn(p[i].ctypes.data) for i in range(len(p))], np.int64)


def label_codes(fn, triples):
    return np.array([fn(int(a), int(b), int(c)) for a, b, c in triples], np.int64)


def answers(ref, x):
    """the reference library's answers for the inputs x, as stored in ref_pin/answers.npz"""
    vp, vq = voxel_pairs(x)
    return dict(constants=np.array([ref.ref_hash_p(), ref.ref_max_n(), ref.ref_max_frame_n()], np.int64),
                label_code=label_codes(ref.ref_label_code, x["labels"]),
                loc_eq=pairwise(ref.ref_loc_eq, *loc_pairs(x)), loc_hash=keywise(ref.ref_loc_hash, loc_keys(x)),
                loc_label_code=label_codes(ref.ref_label_code, x["loc_labels"]),
                voxel_eq=pairwise(ref.ref_voxel_eq, vp, vq), voxel_hash=keywise(ref.ref_voxel_hash, vp))


if __name__ == "__main__":
    from oracle import oracle as orc
    ref = orc.ref_pin()
    if ref is None:
        sys.exit("oracle/_ref/libsgtd_ref_pin.so is not built: run `make -C oracle` where the reference checkout is readable")
    x = inputs()
    os.makedirs(os.path.dirname(PATH), exist_ok=True)
    np.savez_compressed(PATH, **x, **answers(ref, x))
    print("->", PATH, "%.1f KB" % (os.path.getsize(PATH) / 1024.0))
