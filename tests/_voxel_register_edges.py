"""helpers of the sgtd_register_voxels device tests: one call with every getter, and the comparison with the restatement
(tests/_voxel_register_ref.py) bit for bit"""
import numpy as np

import _register_edges as rx
import _register_ref as g
import _voxel_register_ref as v

FIELDS = ("pose", "fitness", "cost", "n_matched", "n_corr", "iterations", "status")
MAP_FIELDS = ("coord", "n_points", "mean", "cov")
EYE = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])


def run(h, clouds, map_off, map_cloud, map_pose, src, tgt, init=None, dev=False, stride=3, **opt):
    """one register_voxels call on manager h and every getter -> register_voxels' dict plus maps [voxel_map(m)] of every
    map and matches [voxel_matches(k)] of every pair"""
    pts, off = rx.pack(clouds, stride)
    if dev:
        import torch
        pts = torch.from_numpy(pts).cuda()
    out = h.register_voxels(pts, off, map_off, map_cloud, map_pose, src, tgt, init, **opt)
    out["maps"] = [h.voxel_map(m) for m in range(len(map_off) - 1)]
    out["matches"] = [h.voxel_matches(k) for k in range(len(src))]
    return out


def same_maps(a, b):
    return all(g.same(a[f], b[f]) for f in MAP_FIELDS)


def compare(got, ref, what=""):
    for k in FIELDS:
        assert g.same(got[k], ref[k]), "%s: %s differs\n%r\n%r" % (what, k, got[k], ref[k])
    assert len(got["maps"]) == len(ref["maps"])
    for m, (a, b) in enumerate(zip(got["maps"], ref["maps"])):
        for f in MAP_FIELDS:
            assert g.same(a[f], b[f]), "%s: %s of map %d differs" % (what, f, m)
    for k, (a, b) in enumerate(zip(got["matches"], ref["matches"])):
        assert np.array_equal(a, b), "%s: matches of pair %d differ" % (what, k)


def check(h, clouds, map_off, map_cloud, map_pose, src, tgt, init=None, what="", dev=False, stride=3, **opt):
    """run on the device, restate, compare everything -> (got, ref)"""
    got = run(h, clouds, map_off, map_cloud, map_pose, src, tgt, init, dev=dev, stride=stride, **opt)
    ref = v.register(clouds, map_off, map_cloud, map_pose, src, tgt, init, **opt)
    compare(got, ref, what)
    return got, ref


def pose_row(axis, angle, t):
    return np.concatenate([g.rot_axis(axis, angle).reshape(9), np.asarray(t, np.float64)])
