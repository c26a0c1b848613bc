"""what the device tests of sgtd_register_clouds share: packing clouds for the call, one run through every getter, and the
bit-for-bit comparison with the restatement (tests/_register_ref.py)."""
import numpy as np

import _register_ref as g

FIELDS = ("pose", "fitness", "cost", "n_matched", "iterations", "status")


def pack(clouds, stride=3):
    """-> points (total, stride) f32 (the fourth column, when there is one, holds a value the rule must not read), offsets"""
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    pts = np.zeros((int(off[-1]), stride), np.float32)
    if stride == 4:
        pts[:, 3] = 1e30
    for k, c in enumerate(clouds):
        pts[off[k]:off[k + 1], :3] = np.asarray(c, np.float32)[:, :3]
    return pts, off


def run(h, clouds, src, tgt, init=None, dev=False, stride=3, **opt):
    """one register_clouds call on manager h and every getter -> register_clouds' dict plus cov {cloud: [n, 3, 3]} of
    every cloud and matches [(j, d2)] of every pair"""
    pts, off = pack(clouds, stride)
    if dev:
        import torch
        pts = torch.from_numpy(pts).cuda()
    out = h.register_clouds(pts, off, src, tgt, init, **opt)
    out["cov"] = {c: h.register_covariances(c) for c in range(len(clouds))}
    out["matches"] = [h.register_matches(k) for k in range(len(src))]
    return out


def compare(got, ref, what=""):
    for k in FIELDS:
        assert g.same(got[k], ref[k]), "%s: %s differs\n%r\n%r" % (what, k, got[k], ref[k])
    named = set(ref["cov"])
    for c, cov in got["cov"].items():
        if c in named:
            assert g.same(cov, ref["cov"][c]), "%s: covariances of cloud %d differ" % (what, c)
        else:
            assert cov.shape == (0, 3, 3), "%s: cloud %d is no pair's and has covariances" % (what, c)
    for k, ((j, d2), (rj, rd2)) in enumerate(zip(got["matches"], ref["matches"])):
        assert np.array_equal(j, rj), "%s: matches of pair %d differ" % (what, k)
        assert g.same(d2, rd2), "%s: d2 of pair %d differs" % (what, k)


def check(h, clouds, src, tgt, init=None, what="", dev=False, stride=3, **opt):
    """run on the device, restate, compare everything -> (got, ref)"""
    got = run(h, clouds, src, tgt, init, dev=dev, stride=stride, **opt)
    ref = g.register(clouds, src, tgt, init, **opt)
    compare(got, ref, what)
    return got, ref


def surfaces(ns, nt, seed):
    """a source of ns and a target of nt points of the planted scene (drawn at 1200 points, shuffled, cut), the truth"""
    s, t, R, tm = g.planted_scene(1200, seed)
    rng = np.random.default_rng(seed + 1000)
    return s[rng.permutation(len(s))[:ns]], t[rng.permutation(len(t))[:nt]], R, tm
