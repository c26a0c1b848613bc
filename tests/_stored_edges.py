"""what the device tests of the cloud store (sgtd_set_frame_clouds, sgtd_register_stored, sgtd_register_stored_loops) share:
packing, one stored call through every getter, and the bit-for-bit comparison with the restatement
(tests/_register_ref.py) on [the call's clouds] + [the stored clouds]."""
import numpy as np

import _register_edges as rx
import _register_ref as g

FIELDS = rx.FIELDS


def store(h, clouds, stride=3, dev=False, **kw):
    """set_frame_clouds of {frame: cloud} in one call, as packed points (stride 4: a fourth float the rule must not read)"""
    frames = list(clouds)
    pts, off = rx.pack([clouds[f] for f in frames], stride)
    if dev:
        import torch
        pts = torch.from_numpy(pts).cuda()
    h.set_frame_clouds(frames, (pts, off), **kw)


def run(h, clouds, src, tgt_frame, init=None, dev=False, stride=3, **opt):
    """one register_stored call on manager h and every getter -> register_clouds' dict plus cov {cloud: [n, 3, 3]} of
    every cloud of the call and matches [(j, d2)] of every pair"""
    pts, off = rx.pack(clouds, stride)
    if dev:
        import torch
        pts = torch.from_numpy(pts).cuda()
    out = h.register_stored(pts, off, src, tgt_frame, init, **opt)
    return getters(h, out, len(clouds))


def getters(h, out, n_clouds):
    out["cov"] = {c: h.stored_covariances(c) for c in range(n_clouds)}
    out["matches"] = [h.stored_matches(k) for k in range(len(out["status"]))]
    return out


def as_clouds(clouds, stored, src, tgt_frame):
    """the register_clouds call the stored call stands for: the call's clouds, then the named frames' stored clouds
    -> (clouds, src, tgt)"""
    frames = sorted(set(int(f) for f in tgt_frame))
    every = list(clouds) + [stored[f] for f in frames]
    return every, [int(s) for s in src], [len(clouds) + frames.index(int(f)) for f in tgt_frame]


def compare(got, ref, src, what=""):
    """every field, every match and d2, and the covariances of the call's clouds: the ones some pair names equal the
    reference's, the others have none"""
    for k in FIELDS:
        assert g.same(got[k], ref[k]), "%s: %s differs\n%r\n%r" % (what, k, got[k], ref[k])
    named = set(int(s) for s in src)
    for c, cov in got["cov"].items():
        if c in named:
            assert g.same(cov, ref["cov"][c]), "%s: covariances of cloud %d differ" % (what, c)
        else:
            assert cov.shape == (0, 3, 3), "%s: cloud %d is no pair's source and has covariances" % (what, c)
    assert len(got["matches"]) == len(ref["matches"])
    for k, ((j, d2), (rj, rd2)) in enumerate(zip(got["matches"], ref["matches"])):
        assert np.array_equal(j, rj), "%s: matches of pair %d differ" % (what, k)
        assert g.same(d2, rd2), "%s: d2 of pair %d differs" % (what, k)


def check(h, clouds, stored, src, tgt_frame, init=None, what="", restate=True, dev=False, stride=3, **opt):
    """a stored call against a direct register_clouds call on the same handle and (restate) the numpy restatement
    -> (got, direct)"""
    got = run(h, clouds, src, tgt_frame, init, dev=dev, stride=stride, **opt)
    every, s, t = as_clouds(clouds, stored, src, tgt_frame)
    direct = rx.run(h, every, s, t, init, **opt)
    compare(got, direct, src, what + " (register_clouds)")
    if restate:
        compare(got, g.register(every, s, t, init, **opt), src, what + " (restatement)")
    return got, direct


def same_cloud(h, frame, cloud, cov=None):
    """frame_cloud() returns the stored points and, where given, the covariances"""
    got = h.frame_cloud(frame)
    assert got is not None, "frame %d has no cloud" % frame
    want = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    assert g.same(got[0], want), "points of frame %d differ" % frame
    if cov is not None:
        assert g.same(got[1], cov), "covariances of frame %d differ" % frame
    return got
