"""what the device tests of sgtd_register_stored_voxels share: one stored voxel call through every getter, the
sgtd_register_voxels call it stands for ([the call's clouds] + [the members' stored clouds], member j being cloud
n_clouds + j), and the bit-for-bit comparison with that call and with the restatement (tests/_voxel_register_ref.py)."""
import numpy as np

import _register_edges as rx
import _stored_edges as sx
import _voxel_register_edges as vx
import _voxel_register_ref as v

FIELDS = vx.FIELDS
store = sx.store


def getters(h, out, n_maps):
    out["maps"] = [h.stored_voxel_map(m) for m in range(n_maps)]
    out["matches"] = [h.stored_voxel_matches(k) for k in range(len(out["status"]))]
    return out


def run(h, clouds, map_off, map_frame, map_pose, src, tgt, init=None, dev=False, stride=3, **opt):
    """one register_stored_voxels call on manager h and every getter -> register_voxels' dict plus maps and matches"""
    pts, off = rx.pack(clouds, stride)
    if dev:
        import torch
        pts = torch.from_numpy(pts).cuda()
    out = h.register_stored_voxels(pts, off, map_off, map_frame, map_pose, src, tgt, init, **opt)
    return getters(h, out, len(map_off) - 1)


def as_clouds(clouds, stored, map_frame):
    """the register_voxels call the stored call stands for -> (clouds, map_cloud)"""
    every = list(clouds) + [stored[int(f)] for f in map_frame]
    return every, np.arange(len(clouds), len(every), dtype=np.int32)


def check(h, clouds, stored, map_off, map_frame, map_pose, src, tgt, init=None, what="", restate=True, dev=False, stride=3, **opt):
    """a stored voxel call against a direct register_voxels call on the same handle and (restate) the numpy restatement
    -> (got, direct)"""
    got = run(h, clouds, map_off, map_frame, map_pose, src, tgt, init, dev=dev, stride=stride, **opt)
    every, map_cloud = as_clouds(clouds, stored, map_frame)
    direct = vx.run(h, every, map_off, map_cloud, map_pose, src, tgt, init, **opt)
    vx.compare(got, direct, what + " (register_voxels)")
    if restate:
        vx.compare(got, v.register(every, map_off, map_cloud, map_pose, src, tgt, init, **opt), what + " (restatement)")
    return got, direct
