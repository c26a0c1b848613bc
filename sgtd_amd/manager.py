"""Host-side mirror of the reference's operator API for the hot path.

`STDescManager` keeps the reference class's method names and argument meaning
(src/sgtd/include/desc/STDesc.h:342-440):

    BuildSingleScanSTD(cloud)  -> descriptors          STDesc.cpp:174-315
    AddSTDescs(descriptors)                            STDesc.cpp:149-172
    candidate_selector(descs)  -> [STDMatchList]       STDesc.cpp:318-460

plus the batched, device-resident forms the GPU wants (`add_frames`,
`query_frames`).  Everything computes in libsgtd_accel.so (HIP, gfx950); this
file only marshals numpy / torch buffers through the C ABI.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (Config, DescSoa, LocalMapOptions, RegisterOptions, RelaxOptions, RelaxReport, ScanConfig, SgtdError, Stats,
                   VoxelRegisterOptions)

DEFAULTS = dict(descriptor_near_num=10, candidate_num=50, max_frame_n=20000, device_id=0,
                descriptor_min_len=0.5, descriptor_max_len=50.0, std_side_resolution=1.0,
                rough_dis_threshold=0.03, first_frame_id=0)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _rows34(poses):
    """(n, 12) rows of the row-major 3x4 [R | t] or (n, 4, 4) -> (R [n, 3, 3], t [n, 3]) in f64"""
    p = np.asarray(poses, np.float64)
    if p.ndim == 3 and p.shape[1:] == (4, 4):
        p = p[:, :3, :]
    p = p.reshape(-1, 3, 4)
    return p[:, :, :3].copy(), p[:, :, 3].copy()


def relax_graph(frame_ids, poses, edges, in_set=None, held=None, w_loop=(1.0, 1.0)):
    """The pose graph relax_session hands to sgtd_relax_poses, in host code (no device): nodes = the session's frames in
    order, then (held=(map_ids, map_poses)) the map frames the chosen loops name, held, in the order the loops first name
    them; edges = the odometry edges Z = inv(A_k) A_k+1 (weight 1), then the chosen loops (frame_a, frame_b, T) as
    i = frame_b's node, j = frame_a's node, Z = T (weights w_loop).  frame_a is always a session frame id.  frame_b is a
    session frame id when held is None and a map frame id otherwise: the two id spaces are independent and may overlap
    (a map numbers its frames from 0 as a session does).  loop_edges() after query_frames stamps every query with the one
    current frame id: the caller then sets frame_a = frame_ids[edges["query"]] first (after loop_frames the ids are the
    frames' own).  A session of no frames gives an empty graph.
    -> dict(pose0, fixed, node_i, node_j, meas, w_trans, w_rot, n_session)"""
    ids = np.asarray(frame_ids).reshape(-1)
    R, t = _rows34(poses)
    F = ids.size
    if R.shape[0] != F:
        raise ValueError("poses: one per frame id")
    session = {int(f): k for k, f in enumerate(ids)}
    fa = np.asarray(edges["frame_a"]).reshape(-1)
    fb = np.asarray(edges["frame_b"]).reshape(-1)
    rel = np.asarray(edges["rel_pose"], np.float64).reshape(-1, 12)
    if fb.size != fa.size or rel.shape[0] != fa.size:
        raise ValueError("edges: frame_a, frame_b and rel_pose rows, one per edge")
    keep = np.ones(fa.size, bool) if in_set is None else np.asarray(in_set).reshape(-1) != 0
    if keep.size != fa.size:
        raise ValueError("in_set: one flag per edge")
    chosen = np.flatnonzero(keep)
    for e in chosen:
        if int(fa[e]) not in session:
            raise ValueError("loop edge %d: frame_a %d is not a frame of the session" % (e, int(fa[e])))
    Rt = np.swapaxes(R, 1, 2)
    ni = list(range(max(F - 1, 0)))
    nj = list(range(1, F))
    meas = [np.concatenate([(Rt[k] @ R[k + 1]).reshape(9), Rt[k] @ (t[k + 1] - t[k])]) for k in range(F - 1)]
    n_odo = len(ni)
    R0, t0 = R, t
    n_map = 0
    if held is None:
        for e in chosen:
            if int(fb[e]) not in session:
                raise ValueError("loop edge %d: frame_b %d is not a frame of the session" % (e, int(fb[e])))
        b_node = session
    else:
        map_ids, map_poses = held
        mR, mt = _rows34(map_poses)
        where = {int(f): k for k, f in enumerate(np.asarray(map_ids).reshape(-1))}
        if mR.shape[0] != len(where):
            raise ValueError("held: (map_ids, map_poses), one pose per distinct map frame id")
        b_node, used = {}, []      # the map frames have nodes of their own, whatever ids the session uses
        for e in chosen:
            f = int(fb[e])
            if f not in where:
                raise ValueError("loop edge %d names map frame %d, which has no held pose" % (e, f))
            if f not in b_node:
                b_node[f] = F + len(used)
                used.append(where[f])
        n_map = len(used)
        if chosen.size:
            # the session in the map's world: P = mul(B, T) at the first chosen loop's frame, carried by the odometry
            e = chosen[0]
            a, b = session[int(fa[e])], where[int(fb[e])]
            Ra = mR[b] @ rel[e, :9].reshape(3, 3)
            ta = mR[b] @ rel[e, 9:] + mt[b]
            S = Ra @ Rt[a]                                   # P_k = P_a inv(A_a) A_k
            R0 = S @ R
            t0 = (S @ (t - t[a])[:, :, None])[:, :, 0] + ta
        R0 = np.concatenate([R0, mR[used]])
        t0 = np.concatenate([t0, mt[used]])
    for e in chosen:
        ni.append(b_node[int(fb[e])])
        nj.append(session[int(fa[e])])
        meas.append(rel[e])
    n = F + n_map
    fixed = np.zeros(n, np.uint8)
    if held is None:
        fixed[:1] = 1
    else:
        fixed[F:] = 1
    m = len(ni)
    w = np.ones((2, m))
    w[0, n_odo:] = w_loop[0]
    w[1, n_odo:] = w_loop[1]
    return {"pose0": np.concatenate([R0, t0[:, :, None]], 2).reshape(n, 12), "fixed": fixed,
            "node_i": np.array(ni, np.int32), "node_j": np.array(nj, np.int32),
            "meas": np.array(meas, np.float64).reshape(m, 12), "w_trans": w[0].copy(), "w_rot": w[1].copy(), "n_session": F}


class Descs:
    """descriptor structure-of-arrays (layout of sgtd_desc_soa), numpy backed"""

    FIELDS = (("side", np.float64, 3), ("angle", np.float64, 3), ("center", np.float64, 3),
              ("vertex", np.float32, 9), ("label", np.int32, 3), ("frame", np.uint32, 1),
              ("node_id", np.int32, 3))

    def __init__(self, n):
        self.n = int(n)
        for name, dt, w in self.FIELDS:
            setattr(self, name, np.zeros((self.n, w) if w > 1 else (self.n,), dtype=dt))

    def soa(self):
        s = DescSoa()
        for name, _, _ in self.FIELDS:
            setattr(s, name, _p(getattr(self, name)))
        return s

    def head(self, n):
        out = Descs(0)
        out.n = int(n)
        for name, _, _ in self.FIELDS:
            setattr(out, name, np.ascontiguousarray(getattr(self, name)[:n]))
        return out

    def take(self, idx):
        out = Descs(0)
        out.n = len(idx)
        for name, _, _ in self.FIELDS:
            setattr(out, name, np.ascontiguousarray(getattr(self, name)[idx]))
        return out


def pack_frame_rows(allowed, frame_lo=None, n_frames=None):
    """the rows of sgtd_set_frame_filter from `allowed` -> (frame_lo, n_frames, rows: uint64 [n_rows, ceil(n_frames / 64)]).
    `allowed`: a 1-D array of frame ids shared by the batch; a list of such arrays, one per query; or a boolean matrix
    [n_queries, n_frames] whose column c is frame frame_lo + c (frame_lo defaults to 0).  Bit f - frame_lo of a row
    (word (f - frame_lo) >> 6, bit (f - frame_lo) & 63, little-endian bit order) is set for an allowed frame f.  For ids,
    frame_lo / n_frames default to the span of the ids given; ids outside [frame_lo, frame_lo + n_frames) are dropped.
    An empty set allows nothing.  ValueError: ids outside [0, 2^32)."""
    a = np.asarray(allowed) if not isinstance(allowed, (list, tuple)) else None
    if a is not None and a.dtype == np.bool_ and a.ndim == 2:
        lo = 0 if frame_lo is None else int(frame_lo)
        n = a.shape[1] if n_frames is None else int(n_frames)
        bits = np.zeros((a.shape[0], max(n, 1)), np.bool_)
        k = min(n, a.shape[1])
        bits[:, :k] = a[:, :k]
    else:
        if a is not None:
            sets = [a]
        elif len(allowed) > 0 and any(np.ndim(x) >= 1 for x in allowed):
            sets = list(allowed)
        else:
            sets = [np.asarray(allowed)]
        sets = [np.asarray(x, dtype=np.int64).reshape(-1) for x in sets]
        ids = np.concatenate(sets) if sets else np.zeros(0, np.int64)
        if ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF):
            raise ValueError("frame ids must lie in [0, 2^32)")
        lo = (int(ids.min()) if ids.size else 0) if frame_lo is None else int(frame_lo)
        n = (int(ids.max()) - lo + 1 if ids.size else 1) if n_frames is None else int(n_frames)
        n = max(n, 1)
        bits = np.zeros((len(sets), n), np.bool_)
        for r, x in enumerate(sets):
            d = x - lo
            bits[r, d[(d >= 0) & (d < n)]] = True
    if not (0 <= lo <= 0xFFFFFFFF and 1 <= n <= 0xFFFFFFFF):
        raise ValueError("frame_lo and n_frames must lie in [0, 2^32)")
    words = (n + 63) // 64
    packed = np.packbits(bits, axis=1, bitorder="little")
    out = np.zeros((bits.shape[0], words * 8), np.uint8)
    out[:, :packed.shape[1]] = packed
    return lo, n, np.ascontiguousarray(out.view("<u8").astype(np.uint64))


class STDMatchList:
    """STDMatchList (STDesc.h:120-124): match_id_ = (query frame id, map frame id);
    match_list_ as (query descriptor index, table entry index) pairs in order"""

    def __init__(self, query_frame, map_frame, votes, q_idx, db_entry):
        self.match_id_ = (int(query_frame), int(map_frame))
        self.votes = int(votes)
        self.q_idx = q_idx
        self.db_entry = db_entry

    def __len__(self):
        return len(self.q_idx)


class BatchResult:
    """candidate_selector output of a batch of query frames (host copies)"""

    def __init__(self, n_cand, cand_frame, cand_votes, pair_off, query_frame_id):
        self.n_cand = n_cand
        self.cand_frame = cand_frame
        self.cand_votes = cand_votes
        self.pair_off = pair_off
        self.query_frame_id = query_frame_id

    def top1(self):
        """map frame with the most votes per query (-1 if no candidate)"""
        return np.where(self.n_cand > 0, self.cand_frame[:, 0], -1)


class DevicePoints:
    """borrowed device memory of the library holding (count, stride) f32 points, in the form the manager's
    device-pointer paths take a torch.cuda tensor: thin_clouds(fetch=False) returns one.  Valid until the manager's next
    thin_clouds call (or one of the leaf= forms, or set_frame_scans) or close()."""
    is_cuda = True
    ndim = 2

    def __init__(self, ptr, stride, count):
        self.ptr, self.stride, self.count = int(ptr or 0), int(stride), int(count)
        self.shape = (self.count, self.stride)

    def data_ptr(self):
        return self.ptr

    def is_contiguous(self):
        return True

    def __len__(self):
        return self.count


class STDescManager:
    def __init__(self, **kw):
        """devices=[ids]: one handle over several GPUs of this process (sgtd_create_multi: the
        table sharded by frame blocks, host-side merge of the per-device candidate tables)"""
        cfg = dict(DEFAULTS)
        self.icp_threshold_ = float(kw.pop("icp_threshold", 0.4))   # SG_localization.yaml:89
        devices = kw.pop("devices", None)
        cfg.update(kw)
        self.config_setting_ = cfg
        self._L = _lib.lib()
        c = Config(**cfg)
        h = C.c_void_p()
        self._h = None
        if devices is None:
            self._check(self._L.sgtd_create(C.byref(c), C.byref(h)))
        else:
            ids = (C.c_int * len(devices))(*[int(d) for d in devices])
            self._check(self._L.sgtd_create_multi(C.byref(c), ids, len(devices), C.byref(h)))
        self._h = h
        self._keep = None

    @property
    def device_count(self):
        return self._L.sgtd_device_count(self._h)

    def close(self):
        if self._h is not None:
            st = self._L.sgtd_destroy(self._h)
            if st != 0:       # (an owner whose table other managers still borrow: close them first)
                raise SgtdError(st, self._L.sgtd_last_error(self._h).decode())
            self._h = None
            self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status):
        if status != 0:
            detail = ""
            if self._h is not None:
                detail = self._L.sgtd_last_error(self._h).decode()
            raise SgtdError(status, detail)

    # ---- plumbing -------------------------------------------------------
    def set_stream(self, stream_ptr):
        self._check(self._L.sgtd_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_timing(self, on):
        self._check(self._L.sgtd_set_timing(self._h, int(bool(on))))

    @property
    def current_frame_id_(self):
        v = C.c_uint32(0)
        self._check(self._L.sgtd_current_frame_id(self._h, C.byref(v)))
        return v.value

    def stats(self):
        s = Stats()
        self._check(self._L.sgtd_get_stats(self._h, C.byref(s)))
        return {f[0]: getattr(s, f[0]) for f in Stats._fields_}

    def sync(self):
        self._check(self._L.sgtd_sync(self._h))

    def max_batch(self, n_keypoints):
        """largest safe number of query frames (of n_keypoints keypoints each) per query_frames call"""
        n = C.c_int64(0)
        self._check(self._L.sgtd_max_batch(self._h, int(n_keypoints), C.byref(n)))
        return n.value

    # ---- BuildSingleScanSTD ----------------------------------------------
    def BuildSingleScanSTD(self, xyz, label):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        label = np.ascontiguousarray(label, dtype=np.uint32)
        n = xyz.shape[0]
        cap = self._L.sgtd_max_descs(self._h, n)
        d = Descs(cap)
        s = d.soa()
        n_out = C.c_int64(0)
        self._check(self._L.sgtd_build(self._h, _p(xyz), _p(label), n, C.byref(s), cap, C.byref(n_out)))
        return d.head(n_out.value)

    # ---- AddSTDescs -------------------------------------------------------
    def AddSTDescs(self, d):
        s = d.soa()
        self._check(self._L.sgtd_add(self._h, C.byref(s), d.n))

    def add_frames(self, xyz, label, kp_off=None, keep_keypoints=False):
        """BuildSingleScanSTD + AddSTDescs for a whole run of frames on the device
        (the caller's map loop, semantic_graph_localization.cpp:419-458).
        xyz (F,N,3)/(total,3) numpy or torch.cuda tensor; kp_off None => uniform N.
        keep_keypoints: also store the frames' keypoints under the ids they are added with (set_frame_keypoints), for
        overlap()."""
        xp, lp, off, nf, dev = self._frames_args(xyz, label, kp_off)
        c0 = self.current_frame_id_ if keep_keypoints else 0
        self._check(self._L.sgtd_add_frames(self._h, xp, lp, _p(off), nf, dev))
        if keep_keypoints and nf:
            if dev:
                xyz, label = xyz.cpu().numpy(), label.cpu().numpy()
            self.set_frame_keypoints(np.arange(c0, c0 + nf, dtype=np.int64), xyz, label, off)

    def set_frame_keypoints(self, frame_ids, xyz, label=None, kp_off=None):
        """map keypoints kept on the handle (sgtd_set_frame_keypoints), keyed by global frame id: frame frame_ids[i] gets
        the keypoints kp_off[i] .. kp_off[i+1] of xyz (.., 3) / label — what add_frames takes for that frame; kp_off None:
        xyz (n, N, 3), N keypoints a frame.  xyz=None forgets the keypoints of those ids; frame_ids=None with xyz=None
        forgets all."""
        if frame_ids is None:
            if xyz is not None:
                raise ValueError("keypoints need their frame ids")
            self._check(self._L.sgtd_set_frame_keypoints(self._h, None, None, None, None, 0))
            return
        ids = np.asarray(frame_ids)
        if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
            raise ValueError("frame_ids: a 1-D array of integer frame ids")
        if ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF):
            raise ValueError("frame ids must lie in [0, 2^32)")
        ids = np.ascontiguousarray(ids, np.uint32)
        if xyz is None:
            if ids.size:
                self._check(self._L.sgtd_set_frame_keypoints(self._h, _p(ids), None, None, None, ids.size))
            return
        if label is None:
            raise ValueError("keypoints need their labels")
        x, l, off = self._keypoint_args(xyz, label, kp_off, ids.size, "frame id")
        if ids.size:
            self._check(self._L.sgtd_set_frame_keypoints(self._h, _p(ids), _p(off), _p(x), _p(l), ids.size))

    @staticmethod
    def _keypoint_args(xyz, label, kp_off, n, what):
        """host keypoint arrays for n frames: xyz (total, 3) f32, label (total,) u32, n + 1 offsets (checked)"""
        x = np.asarray(xyz)
        if kp_off is None:
            if x.ndim != 3 or x.shape[2] != 3 or x.shape[0] != n:
                raise ValueError("xyz: (n, N, 3), one row of keypoints per %s, or kp_off" % what)
            off = np.arange(n + 1, dtype=np.int64) * x.shape[1]
        else:
            off = np.ascontiguousarray(np.asarray(kp_off).reshape(-1), np.int64)
            if off.size != n + 1:
                raise ValueError("kp_off: one offset per %s and a closing one" % what)
        cnt = off[1:] - off[:-1]
        if (cnt < 0).any() or (cnt > 65535).any():
            raise ValueError("a frame has 0 .. 65535 keypoints")
        x = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
        l = np.ascontiguousarray(label, np.uint32).reshape(-1)
        if x.shape[0] != l.size or off[0] < 0 or off[-1] > l.size:
            raise ValueError("xyz, label and kp_off do not fit each other")
        if x.shape[0] == 0:           # (never a NULL pointer for an existing, empty set)
            x, l = np.zeros((1, 3), np.float32), np.zeros(1, np.uint32)
        return x, l, off

    def finalize(self):
        self._check(self._L.sgtd_finalize(self._h))

    def remove_frames(self, frame_ids):
        """take the entries of the given frames out of the table (sgtd_remove_frames): afterwards every query and
        inspection call answers as if those frames had never been added; entry ids are renumbered densely and
        current_frame_id_ does not change.  Duplicates and ids without entries are ignored.  -> entries removed"""
        ids = np.ascontiguousarray(np.asarray(frame_ids, dtype=np.int64).reshape(-1))
        if ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF):
            raise ValueError("frame ids must lie in [0, 2^32)")
        ids = ids.astype(np.uint32)
        n = C.c_int64(0)
        self._check(self._L.sgtd_remove_frames(self._h, _p(ids) if ids.size else None, ids.size, C.byref(n)))
        return n.value

    def set_frame_filter(self, allowed, frame_lo=None, n_frames=None):
        """restrict the following queries to a set of map frames (sgtd_set_frame_filter): each query is answered as by a
        handle that holds only its allowed frames (only the visit counters still count the whole map).  `allowed`: None
        clears the filter; otherwise as pack_frame_rows takes it — frame ids shared by the batch, one id array per query,
        or a boolean matrix [n_queries, n_frames].  A batch of per-query rows must match the next batch's size."""
        if allowed is None:
            self._check(self._L.sgtd_set_frame_filter(self._h, 0, 0, None, 0))
            self._filter = None
            return
        lo, n, rows = pack_frame_rows(allowed, frame_lo, n_frames)
        self._check(self._L.sgtd_set_frame_filter(self._h, lo, n, _p(rows), rows.shape[0]))
        self._filter = (allowed, frame_lo, n_frames)

    def _with_filter(self, allowed, call):
        """call() under the filter `allowed`, then the filter set before it again"""
        if allowed is None:
            return call()
        before = getattr(self, "_filter", None)
        self.set_frame_filter(allowed)
        try:
            return call()
        finally:
            self.set_frame_filter(*before) if before is not None else self.set_frame_filter(None)

    def set_frame_poses(self, frame_ids, poses):
        """map poses kept on the handle (sgtd_set_frame_poses), keyed by global frame id: `poses` (n, 12) rows of the
        row-major 3x4 [R | t] (a graph file's "poses") or (n, 4, 4) matrices, stored as f32.  poses=None forgets the
        poses of those ids; frame_ids=None with poses=None forgets all."""
        if frame_ids is None:
            if poses is not None:
                raise ValueError("poses need their frame ids")
            self._check(self._L.sgtd_set_frame_poses(self._h, None, None, 0))
            return
        ids = np.asarray(frame_ids)
        if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
            raise ValueError("frame_ids: a 1-D array of integer frame ids")
        if ids.size and (ids.min() < 0 or ids.max() > 0xFFFFFFFF):
            raise ValueError("frame ids must lie in [0, 2^32)")
        ids = np.ascontiguousarray(ids, np.uint32)
        if poses is None:
            if ids.size:
                self._check(self._L.sgtd_set_frame_poses(self._h, _p(ids), None, ids.size))
            return
        p = np.asarray(poses)
        if p.ndim == 3 and p.shape[1:] == (4, 4):
            p = p[:, :3, :].reshape(-1, 12)
        if p.ndim != 2 or p.shape[1] != 12 or p.shape[0] != ids.size:
            raise ValueError("poses: (n, 12) rows or (n, 4, 4) matrices, one per frame id")
        p = np.ascontiguousarray(p, np.float32)
        if ids.size:
            self._check(self._L.sgtd_set_frame_poses(self._h, _p(ids), _p(p), ids.size))

    def set_position_prior(self, center, radius=None):
        """restrict the following queries to the map frames whose pose lies within `radius` of `center`
        (sgtd_set_position_prior; the poses come from set_frame_poses).  center: (dims,) for one prior shared by the
        batch or (n_queries, dims), dims 2 (x, y) or 3 (x, y, z); radius: a scalar or one per row (+inf allowed).
        None clears the prior."""
        if center is None:
            self._check(self._L.sgtd_set_position_prior(self._h, None, None, 0, 2))
            self._prior = None
            return
        c = np.asarray(center, np.float64)
        if c.ndim == 1:
            c = c[None, :]
        if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] not in (2, 3):
            raise ValueError("center: (dims,) or (n_rows, dims) with dims 2 or 3")
        if not np.isfinite(c).all():
            raise ValueError("center: finite coordinates")
        if radius is None:
            raise ValueError("a prior needs a radius")
        r = np.asarray(radius, np.float64)
        r = np.full(c.shape[0], float(r)) if r.ndim == 0 else r.reshape(-1)
        if r.size != c.shape[0]:
            raise ValueError("radius: a scalar or one per prior row")
        if np.isnan(r).any() or (r < 0).any():
            raise ValueError("radius: not NaN, not negative")
        c, r = np.ascontiguousarray(c), np.ascontiguousarray(r)
        self._check(self._L.sgtd_set_position_prior(self._h, _p(c), _p(r), c.shape[0], c.shape[1]))
        self._prior = (center, radius)

    def _with_prior(self, prior, call):
        """call() under the prior `prior` = (center, radius), then the prior set before it again"""
        if prior is None:
            return call()
        before = getattr(self, "_prior", None)
        self.set_position_prior(*prior)
        try:
            return call()
        finally:
            self.set_position_prior(*before) if before is not None else self.set_position_prior(None)

    def attach_table(self, owner):
        """borrow the finalized table of `owner` (another manager on the same device): this manager then queries the
        same map with its own work buffers and stream — two batches in flight (include/sgtd_accel.h)"""
        self._check(self._L.sgtd_attach_table(self._h, owner._h))
        self._owner = owner         # (the owner must outlive its views)

    def _frames_args(self, xyz, label, kp_off):
        is_torch = hasattr(xyz, "data_ptr")
        if is_torch:
            assert xyz.is_cuda and label.is_cuda and xyz.is_contiguous() and label.is_contiguous()
            shape = tuple(xyz.shape)
            xp, lp, dev = C.c_void_p(xyz.data_ptr()), C.c_void_p(label.data_ptr()), 1
            self._keep = (xyz, label)
        else:
            xyz = np.ascontiguousarray(xyz, dtype=np.float32)
            label = np.ascontiguousarray(label, dtype=np.uint32)
            shape = xyz.shape
            xp, lp, dev = _p(xyz), _p(label), 0
            self._keep = (xyz, label)
        if kp_off is None:
            assert len(shape) == 3
            nf, n = shape[0], shape[1]
            off = np.arange(nf + 1, dtype=np.int64) * n
        else:
            off = np.ascontiguousarray(kp_off, dtype=np.int64)
            nf = len(off) - 1
        return xp, lp, off, nf, dev

    # ---- candidate_selector -------------------------------------------------
    def query_frames(self, xyz, label, kp_off=None, fetch=True, allowed=None, prior=None):
        """fused BuildSingleScanSTD + candidate_selector for a batch of query frames
        (semantic_graph_localization.cpp:592,601 -> STDesc.cpp:98).  Asynchronous when
        fetch=False (results via .results()).  allowed: a frame filter for this batch only (set_frame_filter);
        prior: (center, radius), a position prior for this batch only (set_position_prior)."""
        xp, lp, off, nq, dev = self._frames_args(xyz, label, kp_off)
        self._nq = nq
        self._with_prior(prior, lambda: self._with_filter(
            allowed, lambda: self._check(self._L.sgtd_query_frames(self._h, xp, lp, _p(off), nq, dev))))
        return self.results() if fetch else None

    def loop_frames(self, xyz, label, kp_off=None, skip_near=0, batch=None, fetch=True):
        """sequence loop detection (sgtd_loop_frames): every frame is added to the table and searched against the
        frames added before it, minus the skip_near frames just before it — the reference's per-frame
        build -> SearchLoop -> AddSTDescs loop (skip_near = 0).  Runs in chunks of at most `batch` frames (None:
        sgtd_max_batch); chunking does not change any frame's result.  fetch=True returns the candidates of every frame
        as one BatchResult (query_frame_id: the frames' ids).  verify(), search_loop() and the result_* calls then
        refer to the last chunk — a caller that wants them for every frame passes `batch` and one chunk per call."""
        xp, lp, off, nf, dev = self._frames_args(xyz, label, kp_off)
        if nf == 0:
            return None
        if batch is None:
            batch = self.max_batch(int(np.max(off[1:] - off[:-1])))
        batch = max(1, int(batch))
        c0 = self.current_frame_id_
        parts = []
        for f0 in range(0, nf, batch):
            n = min(batch, nf - f0)
            st = self._L.sgtd_loop_frames(self._h, xp, lp, _p(np.ascontiguousarray(off[f0:f0 + n + 1])), n, int(skip_near), dev)
            if st == -6 and self.device_count > 1:
                raise SgtdError(st, "loop_frames is not available on a multi-device handle (devices=[...]): "
                                    "use one STDescManager per device")
            self._check(st)
            self._nq = n
            if fetch:
                parts.append(self.results())
        if not fetch:
            return None
        res = BatchResult(*(np.concatenate([getattr(r, k) for r in parts]) for k in ("n_cand", "cand_frame", "cand_votes", "pair_off")),
                          c0 + np.arange(nf, dtype=np.int64))
        return res

    # ---- labelled scans to keypoints (sgtd_scan_keypoints) --------------------------------------------------
    def default_scan_config(self):
        c = ScanConfig()
        self._L.sgtd_default_scan_config(C.byref(c))
        return c

    def _scan_config(self, config):
        """None, a ScanConfig, or a dict of the fields to change from the defaults (arrays: whole, or {class: value})"""
        if config is None or isinstance(config, ScanConfig):
            return config
        c = self.default_scan_config()
        for k, v in dict(config).items():
            if k in ("node_label", "min_seg"):
                arr = getattr(c, k)
                items = v.items() if isinstance(v, dict) else enumerate(v)
                for s, x in items:
                    arr[int(s)] = int(x)
            else:
                setattr(c, k, v)
        return c

    def scan_keypoints(self, points, labels, pt_off=None, config=None, fetch=True):
        """labelled scans to keypoints on the device (sgtd_scan_keypoints): points (total, 3 or 4) f32 — or (S, N, 3 or 4)
        with pt_off None — numpy or torch.cuda tensor, labels u32 (sem | inst << 16), pt_off the S + 1 offsets.  Returns
        xyz (K, 3) f32, label (K,) u32, kp_off (S + 1,) i64 and n_points (K,) i32; fetch=False leaves them on the device
        (scan_results, add_scans, query_scans)."""
        is_torch = hasattr(points, "data_ptr")
        if is_torch:
            assert points.is_cuda and labels.is_cuda and points.is_contiguous() and labels.is_contiguous()
            shape = tuple(points.shape)
            pp, lp, dev = C.c_void_p(points.data_ptr()), C.c_void_p(labels.data_ptr()), 1
        else:
            points = np.ascontiguousarray(points, dtype=np.float32)
            labels = np.ascontiguousarray(labels, dtype=np.uint32)
            shape = points.shape
            pp, lp, dev = _p(points), _p(labels), 0
        if len(shape) < 2 or shape[-1] not in (3, 4):
            raise ValueError("points: (total, 3 or 4) or (S, N, 3 or 4)")
        if pt_off is None:
            if len(shape) != 3:
                raise ValueError("points: (S, N, 3 or 4), or pt_off")
            off = np.arange(shape[0] + 1, dtype=np.int64) * shape[1]
        else:
            off = np.ascontiguousarray(np.asarray(pt_off).reshape(-1), np.int64)
            if off.size < 1:
                raise ValueError("pt_off: n_scans + 1 offsets")
            if off[-1] > int(np.prod(shape[:-1])):
                raise ValueError("pt_off names more points than were given")
        cfg = self._scan_config(config)
        self._check(self._L.sgtd_scan_keypoints(self._h, C.byref(cfg) if cfg is not None else None, pp, int(shape[-1]), lp, _p(off),
                                                off.size - 1, dev))
        self._scan_n = off.size - 1      # (after the call: one that is refused leaves the earlier results, and their count)
        return self.scan_results() if fetch else None

    def scan_results(self):
        n = C.c_int64(0)
        off = np.zeros(self._scan_n + 1, np.int64)
        st = self._L.sgtd_result_scan_keypoints(self._h, _p(off), None, None, None, 0, C.byref(n))
        self._check(st)
        k = n.value
        xyz, label, n_points = np.zeros((k, 3), np.float32), np.zeros(k, np.uint32), np.zeros(k, np.int32)
        self._check(self._L.sgtd_result_scan_keypoints(self._h, _p(off), _p(xyz), _p(label), _p(n_points), k, C.byref(n)))
        return xyz, label, off, n_points

    def scan_point_clusters(self, scan):
        n = C.c_int64(0)
        self._check(self._L.sgtd_result_scan_point_clusters(self._h, int(scan), None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        self._check(self._L.sgtd_result_scan_point_clusters(self._h, int(scan), _p(out), n.value, C.byref(n)))
        return out

    def scan_grids(self, scan):
        """(32, 4) i32 mode, polarNum, width, height and (32, 4) f64 minPitch, maxPitch, minPolar, maxPolar of one scan"""
        grid, rng = np.zeros((32, 4), np.int32), np.zeros((32, 4), np.float64)
        self._check(self._L.sgtd_result_scan_grids(self._h, int(scan), _p(grid), _p(rng)))
        return grid, rng

    def _scan_view(self):
        """the scan keypoints as add_frames / query_frames arguments: xyz, label, offsets, device_ptrs — borrowed device
        pointers, except on a multi-device handle, whose tables take host arrays"""
        if self.device_count > 1:
            xyz, label, off, _ = self.scan_results()
            self._keep = (xyz, label)
            return _p(xyz), _p(label), off, 0
        x, l = C.c_void_p(), C.c_void_p()
        self._check(self._L.sgtd_scan_device_view(self._h, C.byref(x), C.byref(l)))
        off = np.zeros(self._scan_n + 1, np.int64)
        self._check(self._L.sgtd_result_scan_keypoints(self._h, _p(off), None, None, None, 0, None))
        return x, l, off, 1

    def add_scans(self, points, labels, pt_off=None, config=None):
        """scan_keypoints, then add_frames on the keypoints where they lie on the device; returns their offsets"""
        self.scan_keypoints(points, labels, pt_off, config, fetch=False)
        x, l, off, dev = self._scan_view()
        self._check(self._L.sgtd_add_frames(self._h, x, l, _p(off), off.size - 1, dev))
        return off

    def query_scans(self, points, labels, pt_off=None, config=None, fetch=True):
        """scan_keypoints, then query_frames on the keypoints where they lie on the device"""
        self.scan_keypoints(points, labels, pt_off, config, fetch=False)
        x, l, off, dev = self._scan_view()
        self._nq = off.size - 1
        self._check(self._L.sgtd_query_frames(self._h, x, l, _p(off), self._nq, dev))
        return self.results() if fetch else None

    # ---- posed scans to local-map keypoints (sgtd_local_map_keypoints) ----------------------------------------
    @staticmethod
    def _pose_rows(poses, n):
        p = np.asarray(poses)
        if p.ndim == 3 and p.shape[1:] == (4, 4):
            p = p[:, :3, :].reshape(-1, 12)
        if p.ndim != 2 or p.shape[1] != 12 or p.shape[0] != n:
            raise ValueError("poses: (n_scans, 12) rows or (n_scans, 4, 4) matrices")
        return np.ascontiguousarray(p, np.float32)

    def local_map_keypoints(self, points, labels, pt_off, poses, anchors=None, radius=15.0, max_members=0, max_pass_points=0, config=None,
                            fetch=True):
        """posed, labelled scans to the keypoints of local maps on the device (sgtd_local_map_keypoints): the scans as
        scan_keypoints takes them, poses (S, 12) rows or (S, 4, 4) of the frames the points are given in (sensor poses:
        ingest.sensor_poses), anchors the scan indices to build a local map around (None: every scan).  Returns xyz (K, 3)
        f32 in the anchors' frames, label (K,) u32, kp_off (A + 1,) i64, n_points (K,) i32; fetch=False leaves them on
        the device (local_map_results, add_local_maps, query_local_maps)."""
        is_torch = hasattr(points, "data_ptr")
        if is_torch:
            assert points.is_cuda and labels.is_cuda and points.is_contiguous() and labels.is_contiguous()
            shape = tuple(points.shape)
            pp, lp, dev = C.c_void_p(points.data_ptr()), C.c_void_p(labels.data_ptr()), 1
        else:
            points = np.ascontiguousarray(points, dtype=np.float32)
            labels = np.ascontiguousarray(labels, dtype=np.uint32)
            shape = points.shape
            pp, lp, dev = _p(points), _p(labels), 0
        if len(shape) < 2 or shape[-1] not in (3, 4):
            raise ValueError("points: (total, 3 or 4) or (S, N, 3 or 4)")
        if pt_off is None:
            if len(shape) != 3:
                raise ValueError("points: (S, N, 3 or 4), or pt_off")
            off = np.arange(shape[0] + 1, dtype=np.int64) * shape[1]
        else:
            off = np.ascontiguousarray(np.asarray(pt_off).reshape(-1), np.int64)
            if off.size < 1:
                raise ValueError("pt_off: n_scans + 1 offsets")
            if off[-1] > int(np.prod(shape[:-1])):
                raise ValueError("pt_off names more points than were given")
        n_scans = off.size - 1
        pose = self._pose_rows(poses, n_scans)
        if anchors is None:
            ap, na = None, n_scans
        else:
            anch = np.ascontiguousarray(np.asarray(anchors).reshape(-1), np.int32)
            na = anch.size
            ap = _p(anch if na else np.zeros(1, np.int32))
        opt = LocalMapOptions()
        self._L.sgtd_default_local_map_options(C.byref(opt))
        opt.radius, opt.max_members, opt.max_pass_points = float(radius), int(max_members), int(max_pass_points)
        cfg = self._scan_config(config)
        self._check(self._L.sgtd_local_map_keypoints(self._h, C.byref(cfg) if cfg is not None else None, C.byref(opt), pp, int(shape[-1]), lp,
                                                     _p(off), _p(pose if n_scans else np.zeros((1, 12), np.float32)), n_scans, ap, na, dev))
        self._lm_n = na      # (after the call, as scan_keypoints)
        return self.local_map_results() if fetch else None

    def local_map_results(self):
        n = C.c_int64(0)
        off = np.zeros(self._lm_n + 1, np.int64)
        self._check(self._L.sgtd_result_local_map_keypoints(self._h, _p(off), None, None, None, 0, C.byref(n)))
        k = n.value
        xyz, label, n_points = np.zeros((k, 3), np.float32), np.zeros(k, np.uint32), np.zeros(k, np.int32)
        self._check(self._L.sgtd_result_local_map_keypoints(self._h, _p(off), _p(xyz), _p(label), _p(n_points), k, C.byref(n)))
        return xyz, label, off, n_points

    def local_map_members(self):
        """mem_off (A + 1,) i64, member (M,) i32 scan indices (each anchor first, then ascending), merged_points (A,) i64,
        and the number of passes of the last local_map_keypoints call"""
        n, passes = C.c_int64(0), C.c_int32(0)
        off, merged = np.zeros(self._lm_n + 1, np.int64), np.zeros(max(self._lm_n, 1), np.int64)
        self._check(self._L.sgtd_result_local_map_members(self._h, _p(off), None, 0, C.byref(n), _p(merged), C.byref(passes)))
        member = np.zeros(max(n.value, 1), np.int32)
        self._check(self._L.sgtd_result_local_map_members(self._h, None, _p(member), n.value, None, None, None))
        return off, member[:n.value], merged[:self._lm_n], passes.value

    def local_map_stage_ms(self):
        """(members, gather, scan passes) milliseconds of the last call between events (zeros unless set_timing is on)"""
        ms = [C.c_float(0) for _ in range(3)]
        self._check(self._L.sgtd_local_map_stage_ms(self._h, *[C.byref(m) for m in ms]))
        return tuple(m.value for m in ms)

    def _local_map_view(self):
        """the local-map keypoints as add_frames / query_frames arguments (as _scan_view)"""
        if self.device_count > 1:
            xyz, label, off, _ = self.local_map_results()
            self._keep = (xyz, label)
            return _p(xyz), _p(label), off, 0
        x, l = C.c_void_p(), C.c_void_p()
        self._check(self._L.sgtd_local_map_device_view(self._h, C.byref(x), C.byref(l)))
        off = np.zeros(self._lm_n + 1, np.int64)
        self._check(self._L.sgtd_result_local_map_keypoints(self._h, _p(off), None, None, None, 0, None))
        return x, l, off, 1

    def add_local_maps(self, points, labels, pt_off, poses, anchors=None, **kw):
        """local_map_keypoints, then add_frames on the keypoints where they lie on the device and set_frame_poses with
        the anchors' poses under the ids the frames were added with; returns the keypoint offsets"""
        self.local_map_keypoints(points, labels, pt_off, poses, anchors, fetch=False, **kw)
        x, l, off, dev = self._local_map_view()
        nf = off.size - 1
        c0 = self.current_frame_id_
        self._check(self._L.sgtd_add_frames(self._h, x, l, _p(off), nf, dev))
        if nf:
            rows = self._pose_rows(poses, np.asarray(poses).shape[0])
            idx = np.arange(nf) if anchors is None else np.asarray(anchors, np.int64).reshape(-1)
            self.set_frame_poses(np.arange(c0, c0 + nf, dtype=np.int64), rows[idx])
        return off

    def query_local_maps(self, points, labels, pt_off, poses, anchors=None, fetch=True, **kw):
        """local_map_keypoints, then query_frames on the keypoints where they lie on the device"""
        self.local_map_keypoints(points, labels, pt_off, poses, anchors, fetch=False, **kw)
        x, l, off, dev = self._local_map_view()
        self._nq = off.size - 1
        self._check(self._L.sgtd_query_frames(self._h, x, l, _p(off), self._nq, dev))
        return self.results() if fetch else None

    def results(self):
        nq, cn = self._nq, self.config_setting_["candidate_num"]
        n_cand = np.zeros(nq, np.int32)
        cf = np.zeros((nq, cn), np.int32)
        cv = np.zeros((nq, cn), np.int32)
        po = np.zeros((nq, cn + 1), np.int64)
        self._check(self._L.sgtd_result_candidates(self._h, _p(n_cand), _p(cf), _p(cv), _p(po)))
        return BatchResult(n_cand, cf, cv, po, self.current_frame_id_)

    def export_candidates(self, d_frame, d_votes):
        """async D2D copy of the (n_queries, candidate_num) int32 candidate tables into
        torch.cuda tensors (no host synchronisation)"""
        self._check(self._L.sgtd_export_candidates_dev(self._h, C.c_void_p(d_frame.data_ptr()),
                                                       C.c_void_p(d_votes.data_ptr())))

    # ---- the multi-GPU step (include/sgtd_accel.h, sgtd_amd/dist.py) -----------------------------------------
    @staticmethod
    def frames_in(xyz, kp_off=None):
        """query frames a batch call carries"""
        return int(xyz.shape[0]) if kp_off is None else len(kp_off) - 1

    def set_candidate_export(self, d_packed):
        """every batch writes its packed local candidate tables into this torch.cuda int32 tensor as soon as they are
        final (None: off)"""
        if d_packed is None:
            self._check(self._L.sgtd_set_candidate_export(self._h, None, 0))
        else:
            self._check(self._L.sgtd_set_candidate_export(self._h, C.c_void_p(d_packed.data_ptr()), d_packed.numel()))
        self._export_keep = d_packed

    def export_wait(self, side_stream_ptr):
        self._check(self._L.sgtd_export_wait(self._h, C.c_void_p(side_stream_ptr)))

    def export_release(self, side_stream_ptr):
        self._check(self._L.sgtd_export_release(self._h, C.c_void_p(side_stream_ptr)))

    def merge_candidates_dev(self, stream_ptr, gathered, n_tables, my_table, nq, frame, votes, n_cand, src, keep, flags):
        """the merge of STDesc.cpp:423-433 over n_tables packed tables as one kernel on `stream_ptr` (torch.cuda tensors)"""
        self._check(self._L.sgtd_merge_candidates_dev(self._h, C.c_void_p(stream_ptr), C.c_void_p(gathered.data_ptr()), n_tables, my_table, nq,
                                                      C.c_void_p(frame.data_ptr()), C.c_void_p(votes.data_ptr()), C.c_void_p(n_cand.data_ptr()),
                                                      C.c_void_p(src.data_ptr()), C.c_void_p(keep.data_ptr()), C.c_void_p(flags.data_ptr())))

    def gather_verified_dev(self, stream_ptr, gathered, n_tables, src, nq, score, pose):
        self._check(self._L.sgtd_gather_verified_dev(self._h, C.c_void_p(stream_ptr), C.c_void_p(gathered.data_ptr()), n_tables,
                                                     C.c_void_p(src.data_ptr()), nq, C.c_void_p(score.data_ptr()), C.c_void_p(pose.data_ptr())))

    def set_deferred_lists(self, on):
        self._check(self._L.sgtd_set_deferred_lists(self._h, int(bool(on))))

    def finish_lists(self, keep=None):
        """write the match lists of the last batch — of the candidates in the u64-per-query device mask only (None: all)"""
        self._check(self._L.sgtd_finish_lists(self._h, None if keep is None else C.c_void_p(keep.data_ptr())))

    def verify_masked(self, keep):
        self._check(self._L.sgtd_verify_masked(self._h, None if keep is None else C.c_void_p(keep.data_ptr())))

    def result_pairs(self, q, res):
        cn = self.config_setting_["candidate_num"]
        n = int(res.pair_off[q, cn])
        qi = np.zeros(n, np.int32)
        de = np.zeros(n, np.int64)
        got = C.c_int64(0)
        self._check(self._L.sgtd_result_pairs(self._h, q, _p(qi), _p(de), n, C.byref(got)))
        return qi, de

    def result_query_descs(self, q):
        n = C.c_int64(0)
        self._check(self._L.sgtd_result_query_desc_count(self._h, q, C.byref(n)))
        d = Descs(n.value)
        s = d.soa()
        got = C.c_int64(0)
        self._check(self._L.sgtd_result_query_descs(self._h, q, C.byref(s), n.value, C.byref(got)))
        return d

    def result_votes(self, q):
        lo = C.c_uint32(0)
        n = C.c_int64(0)
        self._check(self._L.sgtd_result_votes(self._h, q, None, 0, C.byref(lo), C.byref(n)))
        v = np.zeros(n.value, np.uint32)
        self._check(self._L.sgtd_result_votes(self._h, q, _p(v), n.value, C.byref(lo), C.byref(n)))
        return lo.value, v

    def result_rough(self, q, with_dis=True):
        n = C.c_int64(0)
        st = self._L.sgtd_result_rough(self._h, q, None, None, None, None, None, 0, C.byref(n))
        if st not in (0, -4):
            self._check(st)
        m = n.value
        out = dict(q_idx=np.zeros(m, np.int32), cell=np.zeros(m, np.int32),
                   db_entry=np.zeros(m, np.int64), frame=np.zeros(m, np.uint32),
                   dis=np.zeros(m, np.float64) if with_dis else None)
        self._check(self._L.sgtd_result_rough(self._h, q, _p(out["q_idx"]), _p(out["cell"]),
                                              _p(out["db_entry"]), _p(out["frame"]),
                                              _p(out["dis"]), m, C.byref(n)))
        return out

    def query_descs(self, stds_vec):
        """enqueue one query frame given as descriptors (sgtd_query_descs); results via .results() / .result_pairs() —
        with set_deferred_lists(True) the lists after finish_lists()"""
        s = stds_vec.soa()
        self._nq = 1
        self._check(self._L.sgtd_query_descs(self._h, C.byref(s), stds_vec.n))

    def candidate_selector(self, stds_vec):
        """one query frame given as descriptors -> list of STDMatchList"""
        self.query_descs(stds_vec)
        res = self.results()
        qi, de = self.result_pairs(0, res)
        out = []
        for k in range(int(res.n_cand[0])):
            lo, hi = res.pair_off[0, k], res.pair_off[0, k + 1]
            out.append(STDMatchList(self.current_frame_id_, res.cand_frame[0, k], res.cand_votes[0, k],
                                    qi[lo:hi], de[lo:hi]))
        return out

    # ---- table access -------------------------------------------------------
    # ---- geometric verification (STDesc.cpp:462-571) and SearchLoop's choice (:84-147)
    def verify(self):
        """candidate_verify for every (query, candidate) of the last batch, on the device"""
        self._check(self._L.sgtd_verify(self._h))

    def export_verify(self, d_score, d_pose):
        """async D2D copy of verify_score [n_queries, candidate_num] f64 and pose
        [n_queries, candidate_num, 12] f64 into torch.cuda tensors (no host synchronisation)"""
        self._check(self._L.sgtd_export_verify_dev(self._h, C.c_void_p(d_score.data_ptr()), C.c_void_p(d_pose.data_ptr())))

    def result_verify(self, q):
        """-> (score[candidate_num], rot[candidate_num,3,3], t[candidate_num,3])"""
        cn = self.config_setting_["candidate_num"]
        score = np.zeros(cn, np.float64)
        pose = np.zeros((cn, 12), np.float64)
        self._check(self._L.sgtd_result_verify(self._h, q, _p(score), _p(pose)))
        return score, pose[:, :9].reshape(cn, 3, 3).copy(), pose[:, 9:].copy()

    def result_world_poses(self, q):
        """sgtd_result_world_poses after verify(): (candidate_num, 12) f32, row k = the map pose of candidate k's frame
        composed with its relative pose (row-major 3x4); NaN rows past the candidates, for rejected ones and for frames
        without a pose"""
        cn = self.config_setting_["candidate_num"]
        w = np.zeros((cn, 12), np.float32)
        self._check(self._L.sgtd_result_world_poses(self._h, int(q), _p(w)))
        return w

    def refine_poses(self, iterations=1):
        """sgtd_refine_poses after verify(): the least-squares refit of every verified candidate's relative pose over all
        its inlier pairs, on the device; iterations > 1 re-select the inliers under the last pose before each further fit"""
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)):
            raise TypeError("iterations: an integer")
        if iterations < 1:
            raise ValueError("iterations: at least 1")
        self._check(self._L.sgtd_refine_poses(self._h, int(iterations)))

    def result_refined(self, q):
        """sgtd_result_refined of query q after refine_poses(): a dict of rot [candidate_num, 3, 3], t [candidate_num, 3],
        rmse and rmse_verify [candidate_num] (the residual of the final inlier set under the refined pose and under
        verify()'s), n_pairs [candidate_num] (int32) and moments [candidate_num, 15] (cp, cw, H).  Candidates without a
        verification result: zeros, NaN, 0 pairs"""
        q = self._query_index(q)
        cn = self.config_setting_["candidate_num"]
        pose = np.zeros((cn, 12), np.float64)
        rmse = np.zeros(cn, np.float64)
        rmse_v = np.zeros(cn, np.float64)
        n_pairs = np.zeros(cn, np.int32)
        mom = np.zeros((cn, 15), np.float64)
        self._check(self._L.sgtd_result_refined(self._h, q, _p(pose), _p(rmse), _p(rmse_v), _p(n_pairs), _p(mom)))
        return {"rot": pose[:, :9].reshape(cn, 3, 3).copy(), "t": pose[:, 9:].copy(), "rmse": rmse, "rmse_verify": rmse_v,
                "n_pairs": n_pairs, "moments": mom}

    def result_refined_world_poses(self, q):
        """sgtd_result_refined_world_poses after refine_poses(): result_world_poses with the refined relative poses"""
        q = self._query_index(q)
        cn = self.config_setting_["candidate_num"]
        w = np.zeros((cn, 12), np.float32)
        self._check(self._L.sgtd_result_refined_world_poses(self._h, q, _p(w)))
        return w

    @staticmethod
    def _query_index(q):
        if isinstance(q, bool) or not isinstance(q, (int, np.integer)):
            raise TypeError("q: an integer")
        if q < 0:
            raise ValueError("q: not negative")
        return int(q)

    def result_inliers(self, q, cand, n_pairs):
        """sucess_match_vec of one candidate as positions into its match_list_"""
        idx = np.zeros(max(int(n_pairs), 1), np.int32)
        n = C.c_int64(0)
        self._check(self._L.sgtd_result_inliers(self._h, q, cand, _p(idx), len(idx), C.byref(n)))
        return idx[:n.value].copy()

    def result_inlier_entries(self, q, capacity):
        """sucess_match_vec of EVERY candidate of query q with the table side already fetched: ->
        (cand_off[candidate_num + 1], q_idx[n], Descs of the n table entries); capacity = the sum of the
        candidates' list lengths (result pair_off's last entry) always suffices"""
        cn = self.config_setting_["candidate_num"]
        off = np.zeros(cn + 1, np.int64)
        qi = np.zeros(max(int(capacity), 1), np.int32)
        d = Descs(max(int(capacity), 1))
        s = d.soa()
        n = C.c_int64(0)
        self._check(self._L.sgtd_result_inlier_entries(self._h, q, _p(off), _p(qi), C.byref(s), int(capacity), C.byref(n)))
        return off, qi[:n.value].copy(), d.head(n.value)

    def search_loop(self, icp_threshold=None):
        """SearchLoop's result for every query of the last batch (after verify()):
        (best_cand, best_frame, best_score) arrays; frame -1 / score 0 = no loop (:144)"""
        if icp_threshold is None:
            icp_threshold = self.icp_threshold_
        nq = self._nq
        bc = np.zeros(nq, np.int32)
        bf = np.zeros(nq, np.int32)
        bs = np.zeros(nq, np.float64)
        self._check(self._L.sgtd_search_loop(self._h, float(icp_threshold), _p(bc), _p(bf), _p(bs)))
        return bc, bf, bs

    def loop_edges(self, icp_threshold=None, refined=False):
        """sgtd_result_loop_edges after verify(): one edge for every query whose search_loop choice is accepted, as a
        dict of query [m] (int32), frame_a, frame_b [m] (uint32), rel_pose [m, 12] (rot row-major, t: result_verify's
        pose of the chosen candidate, or result_refined's with refined=True) and score [m] -- what consistent_loops takes"""
        if icp_threshold is None:
            icp_threshold = self.icp_threshold_
        flags = 1 if refined else 0
        cap = max(int(getattr(self, "_nq", 0)), 1)
        q = np.zeros(cap, np.int32)
        fa = np.zeros(cap, np.uint32)
        fb = np.zeros(cap, np.uint32)
        rel = np.zeros((cap, 12), np.float64)
        sc = np.zeros(cap, np.float64)
        n = C.c_int64(0)
        self._check(self._L.sgtd_result_loop_edges(self._h, float(icp_threshold), flags, _p(q), _p(fa), _p(fb), _p(rel), _p(sc),
                                                   cap, C.byref(n)))
        m = n.value
        return {"query": q[:m].copy(), "frame_a": fa[:m].copy(), "frame_b": fb[:m].copy(), "rel_pose": rel[:m].copy(),
                "score": sc[:m].copy()}

    def consistent_loops(self, frame_a, frame_b, rel_pose, max_trans, max_rot, pose_a=None):
        """sgtd_consistent_loops: the pairwise-consistency graph of n loop closures and its greedy clique, on the device.
        frame_a / frame_b: (n,) frame ids whose poses set_frame_poses holds (frame_a may be None when pose_a, (n, 12) rows
        of the row-major 3x4 [R | t], gives the query side's poses); rel_pose: (n, 12) f64 as loop_edges returns them;
        max_rot in radians.  -> dict of in_set, degree, pick [n] (int32), n_set and thresholds (tt, min_trace)"""
        fb = np.ascontiguousarray(frame_b, np.uint32).reshape(-1)
        n = fb.size
        rel = np.ascontiguousarray(rel_pose, np.float64).reshape(-1, 12)
        if rel.shape[0] != n:
            raise ValueError("rel_pose: (n, 12), one row per edge")
        fa = None
        if frame_a is not None:
            fa = np.ascontiguousarray(frame_a, np.uint32).reshape(-1)
            if fa.size != n:
                raise ValueError("frame_a: one id per edge")
        pa = None
        if pose_a is not None:
            pa = np.asarray(pose_a)
            if pa.ndim == 3 and pa.shape[1:] == (4, 4):
                pa = pa[:, :3, :]
            pa = np.ascontiguousarray(pa, np.float32).reshape(-1, 12)
            if pa.shape[0] != n:
                raise ValueError("pose_a: (n, 12) rows or (n, 4, 4) matrices, one per edge")
        n_set = C.c_int32(0)
        self._check(self._L.sgtd_consistent_loops(self._h, n, None if fa is None else _p(fa), _p(fb), _p(rel),
                                                  None if pa is None else _p(pa), float(max_trans), float(max_rot),
                                                  C.byref(n_set)))
        self._cons_n = n
        in_set = np.zeros(n, np.int32)
        degree = np.zeros(n, np.int32)
        pick = np.zeros(n, np.int32)
        thr = np.zeros(2, np.float64)
        self._check(self._L.sgtd_result_consistent(self._h, _p(in_set), _p(degree), _p(pick), _p(thr)))
        return {"in_set": in_set, "degree": degree, "pick": pick, "n_set": n_set.value, "thresholds": thr}

    def relax_poses(self, pose0, node_i, node_j, meas, fixed=None, w_trans=None, w_rot=None, **options):
        """sgtd_relax_poses: pose-graph relaxation on the device.  pose0: (n, 12) rows of the row-major 3x4 [R | t] or
        (n, 4, 4); node_i, node_j: (m,) node indices; meas: (m, 12) Z ~ inv(X_i) X_j in the rel_pose layout; fixed: (n,)
        held nodes (None: node 0); w_trans, w_rot: (m,) weights (None: 1.0); options: fields of sgtd_relax_options.
        -> dict of pose [n, 12], edge_cost [m, 2] and the report's fields.  With no node or no edge nothing runs and
        sgtd_result_relaxed gives nothing: pose and edge_cost come back with 0 rows, whatever n is."""
        p0 = np.asarray(pose0)
        if p0.ndim == 3 and p0.shape[1:] == (4, 4):
            p0 = p0[:, :3, :]
        p0 = np.ascontiguousarray(p0, np.float64).reshape(-1, 12)
        ni = np.ascontiguousarray(node_i, np.int32).reshape(-1)
        nj = np.ascontiguousarray(node_j, np.int32).reshape(-1)
        z = np.ascontiguousarray(meas, np.float64).reshape(-1, 12)
        n, m = p0.shape[0], ni.size
        if nj.size != m or z.shape[0] != m:
            raise ValueError("node_i, node_j and meas: one entry per edge")
        fx = None if fixed is None else np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8).reshape(-1)
        if fx is not None and fx.size != n:
            raise ValueError("fixed: one flag per node")
        ws = []
        for w in (w_trans, w_rot):
            w = None if w is None else np.ascontiguousarray(w, np.float64).reshape(-1)
            if w is not None and w.size != m:
                raise ValueError("weights: one per edge")
            ws.append(w)
        opt = self._options(RelaxOptions, self._L.sgtd_default_relax_options, options)
        rep = RelaxReport()
        self._check(self._L.sgtd_relax_poses(self._h, n, _p(p0), _p(fx), m, _p(ni), _p(nj), _p(z), _p(ws[0]), _p(ws[1]),
                                             C.byref(opt), C.byref(rep)))
        filled = n > 0 and m > 0
        pose = np.zeros((n if filled else 0, 12), np.float64)
        cost = np.zeros((m if filled else 0, 2), np.float64)
        self._check(self._L.sgtd_result_relaxed(self._h, _p(pose), _p(cost)))
        return {"pose": pose, "edge_cost": cost, "cost_before": rep.cost_before, "cost_after": rep.cost_after,
                "lambda": rep.lambda_, "outer_iterations": rep.outer_iterations, "steps_accepted": rep.steps_accepted,
                "cg_iterations": rep.cg_iterations, "status": rep.status}

    def relax_session(self, frame_ids, poses, edges, in_set=None, held=None, w_loop=(1.0, 1.0), **options):
        """A session's trajectory relaxed over its chosen loops (relax_graph + relax_poses).  frame_ids: (F,) the session's
        frames in order; poses: their odometry, (F, 12) or (F, 4, 4); edges: loop_edges()'s dict (frame_a in the session: see
        relax_graph for a batch of query_frames; map ids may overlap the session's);
        in_set: consistent_loops()'s mask (None: every edge).  held=None: the session is closed against itself (frame_b in
        the session too), its first frame held.  held=(map_ids, map_poses): against a fixed map: the map frames the chosen
        loops name are held at those poses, the session starts from P = mul(B, T) of the first chosen loop carried along
        the odometry.  -> dict(poses: {frame id: (12,) row} of the session's frames, graph: what relax_poses was given,
        and relax_poses' result fields)"""
        g = relax_graph(frame_ids, poses, edges, in_set, held, w_loop)
        res = self.relax_poses(g["pose0"], g["node_i"], g["node_j"], g["meas"], g["fixed"], g["w_trans"], g["w_rot"], **options)
        ids = np.asarray(frame_ids).reshape(-1)
        res["poses"] = {int(f): res["pose"][k].copy() for k, f in enumerate(ids)} if res["pose"].shape[0] else {}
        res["graph"] = g
        return res

    def consistency_rows(self):
        """the bit matrix of the last consistent_loops call: (n, ceil(n / 64)) uint64, bit j of row i = bit j & 63 of word
        j >> 6 (parity and diagnostics)"""
        n = getattr(self, "_cons_n", 0)
        rows = np.zeros((n, (n + 63) // 64), np.uint64)
        self._check(self._L.sgtd_result_consistency_rows(self._h, 0, n, _p(rows)))
        return rows

    def pose_consensus(self, max_trans, max_rot, refined=False, aligned=False, fetch=True):
        """sgtd_pose_consensus after verify(): per query of the pending batch, the mutually consistent set of its verified
        candidates (by the world pose each implies: set_frame_poses) and one fused pose, in one launch.  refined / aligned:
        fuse refine_poses' / align_keypoints' poses instead of verify's; max_rot in radians.  -> result_consensus()
        (fetch=False: None, the call only enqueues)"""
        flags = (1 if refined else 0) | (2 if aligned else 0)
        self._check(self._L.sgtd_pose_consensus(self._h, float(max_trans), float(max_rot), flags))
        self._consensus = (int(self._nq), int(self.config_setting_["candidate_num"]))
        return self.result_consensus() if fetch else None

    def pose_consensus_rows(self, n_cand, cand_frame, score, rel_pose, max_trans, max_rot):
        """sgtd_pose_consensus_rows: the same over caller arrays, independent of the pending batch: n_cand (nq,),
        cand_frame (nq, cn) as results() gives them, score (nq, cn) and rel_pose (nq, cn, 12) as result_verify /
        result_refined / result_aligned give them (rot row-major (9), t (3)); cn <= 64.  -> result_consensus()"""
        nc = np.ascontiguousarray(n_cand, np.int32).reshape(-1)
        nq = nc.size
        sc = np.asarray(score, np.float64)
        if sc.ndim != 2 or sc.shape[0] != nq:
            raise ValueError("score: (nq, cn)")
        cn = sc.shape[1]
        sc = np.ascontiguousarray(sc)
        cf = np.ascontiguousarray(cand_frame, np.int32).reshape(nq, -1) if nq else np.zeros((0, cn), np.int32)
        rel = np.ascontiguousarray(rel_pose, np.float64).reshape(nq, -1) if nq else np.zeros((0, cn * 12), np.float64)
        if cf.shape[1] != cn or rel.shape[1] != cn * 12:
            raise ValueError("cand_frame (nq, cn), score (nq, cn) and rel_pose (nq, cn, 12) do not agree")
        self._check(self._L.sgtd_pose_consensus_rows(self._h, nq, cn, _p(nc), _p(cf), _p(sc), _p(rel), float(max_trans), float(max_rot)))
        self._consensus = (nq, cn)
        return self.result_consensus()

    def result_consensus(self, first=0, n=None):
        """sgtd_result_consensus for queries first .. first + n - 1 (all by default) -> dict of pose [n, 12] (row-major 3x4
        [R | t], NaN without a valid candidate), n_valid, n_set, seed [n] (int32), mask [n] (uint64: bit k = candidate k is a
        member), support_score, spread_t2, spread_trace [n] and thresholds (tt, min_trace)"""
        nq = getattr(self, "_consensus", (0, 0))[0]
        n = nq - first if n is None else int(n)
        m = max(n, 0)
        out = {"pose": np.zeros((m, 12), np.float64), "n_valid": np.zeros(m, np.int32), "n_set": np.zeros(m, np.int32),
               "seed": np.zeros(m, np.int32), "mask": np.zeros(m, np.uint64), "support_score": np.zeros(m, np.float64),
               "spread_t2": np.zeros(m, np.float64), "spread_trace": np.zeros(m, np.float64), "thresholds": np.zeros(2, np.float64)}
        self._check(self._L.sgtd_result_consensus(self._h, int(first), n, _p(out["pose"]), _p(out["n_valid"]), _p(out["n_set"]),
                                                  _p(out["seed"]), _p(out["mask"]), _p(out["support_score"]), _p(out["spread_t2"]),
                                                  _p(out["spread_trace"]), _p(out["thresholds"])))
        return out

    def consensus_rows(self, q):
        """sgtd_result_consensus_rows: query q's agreement rows (cn,) uint64 (bit l of row k: candidates k and l agree),
        degree (cn,) (-1: invalid) and pick (cn,) (the position in the greedy order, else -1)"""
        cn = getattr(self, "_consensus", (0, 0))[1]
        rows = np.zeros(max(cn, 1), np.uint64)
        degree = np.zeros(max(cn, 1), np.int32)
        pick = np.zeros(max(cn, 1), np.int32)
        self._check(self._L.sgtd_result_consensus_rows(self._h, int(q), _p(rows), _p(degree), _p(pick)))
        return rows[:cn], degree[:cn], pick[:cn]

    def search_loop_consensus(self, min_support=2):
        """sgtd_search_loop_consensus after pose_consensus(): a query is accepted when its set has at least min_support
        members; its choice is the member with the largest verify_score.  -> (best_cand, best_frame, best_score, support)
        arrays; -1, -1, 0 where nothing is accepted; support = n_set"""
        nq = getattr(self, "_consensus", (0, 0))[0]
        bc = np.zeros(nq, np.int32)
        bf = np.zeros(nq, np.int32)
        bs = np.zeros(nq, np.float64)
        sup = np.zeros(nq, np.int32)
        self._check(self._L.sgtd_search_loop_consensus(self._h, int(min_support), _p(bc), _p(bf), _p(bs), _p(sup)))
        return bc, bf, bs, sup

    def consensus_edges(self, min_support=2, capacity=None):
        """sgtd_result_consensus_edges after pose_consensus(): one edge per accepted query, loop_edges()'s dict: frame_b =
        the chosen member's frame, rel_pose = inv(its stored pose) * the fused pose, score = support_score -- what
        consistent_loops and relax_session take"""
        cap = max(int(getattr(self, "_consensus", (0, 0))[0]), 1) if capacity is None else int(capacity)
        room = max(cap, 1)
        q = np.zeros(room, np.int32)
        fa = np.zeros(room, np.uint32)
        fb = np.zeros(room, np.uint32)
        rel = np.zeros((room, 12), np.float64)
        sc = np.zeros(room, np.float64)
        n = C.c_int64(0)
        self._check(self._L.sgtd_result_consensus_edges(self._h, int(min_support), _p(q), _p(fa), _p(fb), _p(rel), _p(sc), cap, C.byref(n)))
        m = min(n.value, cap)
        return {"query": q[:m].copy(), "frame_a": fa[:m].copy(), "frame_b": fb[:m].copy(), "rel_pose": rel[:m].copy(),
                "score": sc[:m].copy()}

    def overlap(self, radius, refined=False, xyz=None, label=None, kp_off=None):
        """sgtd_overlap after verify(): under every verified candidate's relative pose (refined=True: refine_poses()'s),
        how many of the query's keypoints land within `radius` of a keypoint of the same label of the candidate's frame
        (set_frame_keypoints / add_frames(keep_keypoints=True)).  xyz=None: the batch's own keypoints (query_frames,
        loop_frames); otherwise xyz / label (and kp_off, or xyz (n_queries, N, 3)) for every query of the batch."""
        if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
            raise TypeError("radius: a number")
        radius = float(radius)
        if not (radius >= 0.0) or np.isinf(radius):
            raise ValueError("radius: finite, not negative")
        flags = 1 if refined else 0
        if xyz is None:
            if label is not None or kp_off is not None:
                raise ValueError("label and kp_off come with xyz")
            self._check(self._L.sgtd_overlap(self._h, radius, flags, None, None, None))
            return
        if label is None:
            raise ValueError("keypoints need their labels")
        x, l, off = self._keypoint_args(xyz, label, kp_off, self._nq, "query")
        self._check(self._L.sgtd_overlap(self._h, radius, flags, _p(x), _p(l), _p(off)))

    def result_overlap(self, q):
        """sgtd_result_overlap of query q after overlap(): a dict of n_query_kp, n_frame_kp, n_hit_query, n_hit_frame
        [candidate_num] (int32; -1 without a verification result, n_frame_kp -1 for a frame without stored keypoints),
        overlap (n_hit_query / n_query_kp) and rms [candidate_num] (NaN where undefined)"""
        q = self._query_index(q)
        cn = self.config_setting_["candidate_num"]
        out = {k: np.zeros(cn, np.int32) for k in ("n_query_kp", "n_frame_kp", "n_hit_query", "n_hit_frame")}
        out["overlap"] = np.zeros(cn, np.float64)
        out["rms"] = np.zeros(cn, np.float64)
        self._check(self._L.sgtd_result_overlap(self._h, q, _p(out["n_query_kp"]), _p(out["n_frame_kp"]), _p(out["n_hit_query"]),
                                                _p(out["n_hit_frame"]), _p(out["overlap"]), _p(out["rms"])))
        return out

    def search_loop_overlap(self, min_overlap, icp_threshold=None):
        """sgtd_search_loop_overlap: search_loop()'s rule over the candidates whose overlap reaches min_overlap (after
        overlap(); min_overlap <= 0: search_loop()'s choice) -> (best_cand, best_frame, best_score, best_overlap)"""
        if isinstance(min_overlap, bool) or not isinstance(min_overlap, (int, float, np.integer, np.floating)):
            raise TypeError("min_overlap: a number")
        if np.isnan(min_overlap):
            raise ValueError("min_overlap: not NaN")
        if icp_threshold is None:
            icp_threshold = self.icp_threshold_
        nq = self._nq
        bc = np.zeros(nq, np.int32)
        bf = np.zeros(nq, np.int32)
        bs = np.zeros(nq, np.float64)
        bo = np.zeros(nq, np.float64)
        self._check(self._L.sgtd_search_loop_overlap(self._h, float(icp_threshold), float(min_overlap), _p(bc), _p(bf), _p(bs), _p(bo)))
        return bc, bf, bs, bo

    def align_keypoints(self, radius, iterations=10, refined=False, xyz=None, label=None, kp_off=None):
        """sgtd_align_keypoints after verify(): for every verified candidate, assign each query keypoint to the nearest
        keypoint of its label of the candidate's frame within `radius` (set_frame_keypoints /
        add_frames(keep_keypoints=True)), refit the pose over the assigned pairs, and repeat up to `iterations` times or
        until the assignment stays.  refined=True starts from refine_poses()'s pose.  xyz=None: the batch's own keypoints
        (query_frames, loop_frames); otherwise xyz / label (and kp_off, or xyz (n_queries, N, 3)) for every query."""
        if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
            raise TypeError("radius: a number")
        radius = float(radius)
        if not (radius >= 0.0) or np.isinf(radius):
            raise ValueError("radius: finite, not negative")
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)):
            raise TypeError("iterations: an integer")
        if iterations < 1:
            raise ValueError("iterations: at least 1")
        flags = 1 if refined else 0
        if xyz is None:
            if label is not None or kp_off is not None:
                raise ValueError("label and kp_off come with xyz")
            self._check(self._L.sgtd_align_keypoints(self._h, radius, int(iterations), flags, None, None, None))
            return
        if label is None:
            raise ValueError("keypoints need their labels")
        x, l, off = self._keypoint_args(xyz, label, kp_off, self._nq, "query")
        self._check(self._L.sgtd_align_keypoints(self._h, radius, int(iterations), flags, _p(x), _p(l), _p(off)))

    def result_aligned(self, q):
        """sgtd_result_aligned of query q after align_keypoints(): a dict of rot [candidate_num, 3, 3], t [candidate_num, 3]
        (the aligned pose), n_fits, n_corr, stop [candidate_num] (int32; stop 0 = out of iterations, 1 = fewer than 3
        assigned, 2 = converged, -1 = no verification result), counts_before / counts_after [candidate_num, 4] (int32:
        n_query_kp, n_frame_kp, n_hit_query, n_hit_frame of result_overlap's rule under the start / the aligned pose),
        overlap_before, rms_before, overlap_after, rms_after [candidate_num] and moments [candidate_num, 15] (cp, cw, H
        of the last fit)"""
        q = self._query_index(q)
        cn = self.config_setting_["candidate_num"]
        pose = np.zeros((cn, 12), np.float64)
        out = {k: np.zeros(cn, np.int32) for k in ("n_fits", "n_corr", "stop")}
        out["counts_before"] = np.zeros((cn, 4), np.int32)
        out["counts_after"] = np.zeros((cn, 4), np.int32)
        for k in ("overlap_before", "rms_before", "overlap_after", "rms_after"):
            out[k] = np.zeros(cn, np.float64)
        out["moments"] = np.zeros((cn, 15), np.float64)
        self._check(self._L.sgtd_result_aligned(self._h, q, _p(pose), _p(out["n_fits"]), _p(out["n_corr"]), _p(out["stop"]),
                                                _p(out["counts_before"]), _p(out["counts_after"]), _p(out["overlap_before"]),
                                                _p(out["rms_before"]), _p(out["overlap_after"]), _p(out["rms_after"]),
                                                _p(out["moments"])))
        out["rot"] = pose[:, :9].reshape(cn, 3, 3).copy()
        out["t"] = pose[:, 9:].copy()
        return out

    def result_aligned_pairs(self, q, cand):
        """sgtd_result_aligned_pairs: the frame keypoint every keypoint of query q is assigned to under candidate cand's
        aligned pose, -1 where none (int32, one entry per query keypoint)"""
        q = self._query_index(q)
        if isinstance(cand, bool) or not isinstance(cand, (int, np.integer)):
            raise TypeError("cand: an integer")
        if cand < 0:
            raise ValueError("cand: not negative")
        n = C.c_int64(0)
        self._check(self._L.sgtd_result_aligned_pairs(self._h, q, int(cand), None, 0, C.byref(n)))
        a = np.zeros(max(int(n.value), 1), np.int32)
        self._check(self._L.sgtd_result_aligned_pairs(self._h, q, int(cand), _p(a), len(a), C.byref(n)))
        return a[:n.value].copy()

    def result_aligned_world_poses(self, q):
        """sgtd_result_aligned_world_poses after align_keypoints(): result_world_poses with the aligned relative poses"""
        q = self._query_index(q)
        cn = self.config_setting_["candidate_num"]
        w = np.zeros((cn, 12), np.float32)
        self._check(self._L.sgtd_result_aligned_world_poses(self._h, q, _p(w)))
        return w

    def search_loop_aligned(self, min_overlap=0.0, max_rms=0.0):
        """sgtd_search_loop_aligned after align_keypoints(): per query the candidate with the smallest rms_after among
        those with overlap_after >= min_overlap (<= 0: no bound) and rms_after <= max_rms (<= 0 or inf: no bound) ->
        (best_cand, best_frame, best_rms, best_overlap); -1, -1, NaN, NaN where nothing qualifies"""
        for name, v in (("min_overlap", min_overlap), ("max_rms", max_rms)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise TypeError(name + ": a number")
            if np.isnan(v):
                raise ValueError(name + ": not NaN")
        nq = self._nq
        bc = np.zeros(nq, np.int32)
        bf = np.zeros(nq, np.int32)
        br = np.zeros(nq, np.float64)
        bo = np.zeros(nq, np.float64)
        self._check(self._L.sgtd_search_loop_aligned(self._h, float(min_overlap), float(max_rms), _p(bc), _p(bf), _p(br), _p(bo)))
        return bc, bf, br, bo

    # ---- what the registration calls share: their arguments as the library takes them, checked, and their getters' bodies
    def _points_arg(self, points, what="points"):
        """(total, 3 or 4) f32, numpy or a torch.cuda tensor -> (shape, pointer, device_ptrs); the array is kept alive"""
        if hasattr(points, "data_ptr"):
            if not (points.is_cuda and points.is_contiguous()):
                raise ValueError(what + ": a contiguous torch.cuda tensor")
            shape, pp, dev = tuple(points.shape), C.c_void_p(points.data_ptr()), 1
        else:
            points = np.ascontiguousarray(points, dtype=np.float32)
            shape, pp, dev = points.shape, _p(points), 0
        self._keep = points
        if len(shape) != 2 or shape[1] not in (3, 4):
            raise ValueError(what + ": (total, 3 or 4)")
        return shape, pp, dev

    def _offsets(self, pt_off, shape, what="pt_off", per_query=False):
        """the clouds' offsets within points of `shape` (int64): n_clouds + 1 of them, or one cloud per query of the batch"""
        off = np.ascontiguousarray(np.asarray(pt_off).reshape(-1), np.int64)
        if per_query and off.size != self._nq + 1:
            raise ValueError(what + ": n_queries + 1 offsets")
        if off.size < 1:
            raise ValueError(what + ": n_clouds + 1 offsets")
        if off[-1] > shape[0]:
            raise ValueError(what + " names more points than were given")
        return off

    def _pairs_arg(self, src, tgt, init, what, tgt_ids=False):
        """the pairs' sources, targets (cloud or map indices; tgt_ids: frame ids) and start poses -> (src, tgt, init, n)"""
        s = np.ascontiguousarray(src, np.int32).reshape(-1)
        t = self._frame_ids(tgt) if tgt_ids else np.ascontiguousarray(tgt, np.int32).reshape(-1)
        if t.size != s.size:
            raise ValueError(what)
        p0 = None
        if init is not None:
            p0 = np.ascontiguousarray(init, np.float64).reshape(-1, 12)
            if p0.shape[0] != s.size:
                raise ValueError("init: (n, 12), one start pose per pair")
        return s, t, p0, s.size

    def _maps_arg(self, map_off, members, map_pose, frame_ids=False):
        """the maps' member offsets, members (cloud indices; frame_ids: frame ids) and member poses -> (map_off, members, map_pose)"""
        moff = np.ascontiguousarray(np.asarray(map_off).reshape(-1), np.int32)
        if moff.size < 1:
            raise ValueError("map_off: n_maps + 1 offsets")
        mem = self._frame_ids(members) if frame_ids else np.ascontiguousarray(members, np.int32).reshape(-1)
        if moff[-1] > mem.size:
            raise ValueError("map_off names more members than were given")
        mp = None
        if map_pose is not None:
            mp = np.ascontiguousarray(map_pose, np.float64).reshape(-1, 12)
            if mp.shape[0] != mem.size:
                raise ValueError("map_pose: (members, 12), one pose per member")
        return moff, mem, mp

    @staticmethod
    def _options(struct, default, options):
        """an options struct of the library: `default` fills it, then the caller's fields"""
        opt = struct()
        default(C.byref(opt))
        for k, v in options.items():
            if k not in dict(struct._fields_):
                raise TypeError("unknown option " + k)
            setattr(opt, k, v)
        return opt

    @staticmethod
    def _loops_args(start, max_per_query, max_members=0, radius=0.0):
        """what the loops calls check of their choices -> the library's code of `start`"""
        starts = {"verify": 0, "refined": 1, "aligned": 2}
        if start not in starts:
            raise ValueError('start: "verify", "refined" or "aligned"')
        if isinstance(max_per_query, bool) or not isinstance(max_per_query, (int, np.integer)) or max_per_query < 0:
            raise ValueError("max_per_query: an integer, not negative")
        if isinstance(max_members, bool) or not isinstance(max_members, (int, np.integer)) or max_members < 0:
            raise ValueError("max_members: an integer, not negative (0 = no cap)")
        if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or not (np.isfinite(radius) and radius >= 0):
            raise ValueError("radius: finite and not negative")
        return starts[start]

    def _sized(self, fn, lead, kinds):
        """a getter that is asked for its size first: fn(handle, *lead, arrays..., capacity, &n) -> the arrays, one per
        (row shape, dtype) of `kinds`, n rows each"""
        n = C.c_int64(0)
        self._check(fn(self._h, *lead, *[None] * len(kinds), 0, C.byref(n)))
        out = [np.zeros((n.value,) + row, dtype) for row, dtype in kinds]
        self._check(fn(self._h, *lead, *[_p(a) for a in out], n.value, C.byref(n)))
        return out

    def _rows_dict(self, fn, n, with_corr):
        """the result rows of a registration call of n pairs (n_corr: the voxel calls')"""
        out = {"pose": np.zeros((n, 12), np.float64), "fitness": np.zeros(n, np.float64), "cost": np.zeros((n, 2), np.float64)}
        for k in ("n_matched", "n_corr", "iterations", "status") if with_corr else ("n_matched", "iterations", "status"):
            out[k] = np.zeros(n, np.int32)
        self._check(fn(self._h, *[_p(a) for a in out.values()]))
        return out

    def _stage_ms(self, fn, k):
        v = [C.c_float(0) for _ in range(k)]
        self._check(fn(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    _VOXEL_KINDS = (((3,), np.int32), ((), np.int32), ((3,), np.float64), ((3, 3), np.float64))      # a voxel map's coord, n_points, mean, cov

    # ---- dense registration of raw clouds (sgtd_register_clouds) ---------------------------------------------
    def register_tiles(self):
        """source tile, target tile and slice length (points) of the register kernels"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._L.sgtd_register_tiles(C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def register_clouds(self, points, pt_off, src, tgt, init=None, **options):
        """sgtd_register_clouds: plane-regularised GICP of raw clouds on the device.  points: (total, 3 or 4) f32, numpy or
        a torch.cuda tensor, the clouds back to back; pt_off: the n_clouds + 1 offsets; src, tgt: (n,) cloud indices of
        the pairs; init: (n, 12) start poses in the rel_pose layout (rot row-major, t; x = R p + t takes a source point
        into the target's frame), None = the identity; options: fields of sgtd_register_options.  -> dict of pose [n, 12],
        fitness [n], cost [n, 2] (first and last linearisation), n_matched, iterations, status [n] (int32)"""
        shape, pp, dev = self._points_arg(points)
        off = self._offsets(pt_off, shape)
        s, t, p0, n = self._pairs_arg(src, tgt, init, "src and tgt: one cloud index per pair")
        opt = self._options(RegisterOptions, self._L.sgtd_default_register_options, options)
        self._check(self._L.sgtd_register_clouds(self._h, C.byref(opt), pp, int(shape[1]), _p(off), off.size - 1, _p(s), _p(t), _p(p0), n, dev))
        self._reg_n = n
        return self.result_registered()

    def result_registered(self):
        return self._rows_dict(self._L.sgtd_result_registered, self._reg_n, False)

    def register_covariances(self, cloud):
        """the regularised covariances of one cloud of the last register_clouds call: (n, 3, 3) f64; 0 rows for a cloud no
        pair named"""
        return self._sized(self._L.sgtd_result_register_covariances, (int(cloud),), (((3, 3), np.float64),))[0]

    def register_matches(self, pair):
        """the correspondences of one pair under its final pose: (tgt_index (n,) int32, -1 where none; d2 (n,) f64)"""
        return tuple(self._sized(self._L.sgtd_result_register_matches, (int(pair),), (((), np.int32), ((), np.float64))))

    def register_stage_ms(self):
        """device milliseconds of the last register_clouds call: covariances, searches, the rest, the whole call (zeros
        unless set_timing(True))"""
        return self._stage_ms(self._L.sgtd_register_stage_ms, 4)

    def register_pairs(self, max_per_query=5, start="verify"):
        """the (query, candidate) pairs register_loops forms, after verify(): per query its candidates with a verification
        result (score >= 0) in descending verify score, ties in candidate order (the node's :603), the first max_per_query
        of them -> (query [m], cand [m], frame [m] (int32), init [m, 12]) with the pose of the named stage: "verify",
        "refined" (refine_poses) or "aligned" (align_keypoints); a stage that has not run on this batch raises its state
        error"""
        self._loops_args(start, max_per_query)
        res = self.results()
        qs, cs, fs, init = [], [], [], []
        for q in range(self._nq):
            score, rot, t = self.result_verify(q)
            if start == "refined":
                r = self.result_refined(q)
                rot, t = r["rot"], r["t"]
            elif start == "aligned":
                r = self.result_aligned(q)
                rot, t = r["rot"], r["t"]
            nc = int(res.n_cand[q])
            ok = [c for c in range(nc) if score[c] >= 0]
            ok.sort(key=lambda c: -score[c])      # (stable: ties stay in candidate order)
            for c in ok[:int(max_per_query)]:
                qs.append(q)
                cs.append(c)
                fs.append(int(res.cand_frame[q, c]))
                init.append(np.concatenate([rot[c].reshape(9), t[c]]))
        return (np.array(qs, np.int32), np.array(cs, np.int32), np.array(fs, np.int32),
                np.array(init, np.float64).reshape(-1, 12))

    def register_loops(self, query_points, query_pt_off, map_clouds, max_per_query=5, start="verify", **options):
        """Dense registration of the batch's best candidates, after verify(): register_pairs' (query, candidate) pairs,
        each the query's raw cloud (query_points (total, 3 or 4) f32 with the n_queries + 1 offsets query_pt_off) against
        map_clouds[frame] (a dict or sequence of (n, 3 or 4) f32 arrays by frame id; a frame without a cloud is skipped),
        started from the named stage's pose, in ONE register_clouds call.  -> dict of query, cand, frame [m] (int32),
        init [m, 12] and register_clouds' fields per pair.  Thin raw scans first (ingest.voxel_downsample): the search is
        brute force.  The world pose of a pair is result_world_poses' composition (the frame's stored pose times the
        relative pose) with the registered pose in place of verify()'s; the node's :747 multiplies the GICP transform on
        the other side of the loop transform, which is not reproduced here."""
        pack = self._loop_clouds(query_points, query_pt_off, map_clouds)
        q, c, f, init = self.register_pairs(max_per_query, start)
        has = np.array([self._by_frame(map_clouds, int(x)) is not None for x in f], bool)
        q, c, f, init = q[has], c[has], f[has], init[has]
        pts, off, slot = pack(sorted(set(int(x) for x in f)))
        tgt = np.array([slot[int(x)] for x in f], np.int32)
        out = self.register_clouds(pts, off, q, tgt, init if len(q) else None, **options)
        out.update(query=q, cand=c, frame=f, init=init, src_cloud=q.copy(), tgt_cloud=tgt, points=pts, pt_off=off)
        return out

    @staticmethod
    def _by_frame(table, frame):
        """the entry of `frame` in a dict or sequence by frame id, None where it has none"""
        if isinstance(table, dict):
            return table.get(int(frame))
        return table[frame] if 0 <= frame < len(table) else None

    def _loop_clouds(self, query_points, query_pt_off, map_clouds):
        """the queries' clouds of register_loops / register_loops_local, checked -> pack(frames): the query clouds followed
        by the clouds of those map frames -> (points, pt_off, slot: frame id -> cloud index)"""
        qp = np.ascontiguousarray(query_points, dtype=np.float32)
        if qp.ndim != 2 or qp.shape[1] not in (3, 4):
            raise ValueError("query_points: (total, 3 or 4)")
        qoff = np.asarray(query_pt_off, np.int64).reshape(-1)
        if qoff.size != self._nq + 1:
            raise ValueError("query_pt_off: n_queries + 1 offsets")

        def pack(frames):
            clouds = []
            for x in frames:
                a = np.ascontiguousarray(self._by_frame(map_clouds, x), dtype=np.float32)
                if a.ndim != 2 or a.shape[1] != qp.shape[1]:
                    raise ValueError("map_clouds: (n, %d) arrays, as the query points" % qp.shape[1])
                clouds.append(a)
            pts = np.concatenate([qp[:qoff[-1]]] + clouds) if clouds else qp[:qoff[-1]]
            off = np.concatenate([qoff, qoff[-1] + np.cumsum([a.shape[0] for a in clouds], dtype=np.int64)]).astype(np.int64)
            return pts, off, {x: self._nq + k for k, x in enumerate(frames)}

        return pack

    # ---- map clouds kept on the device (sgtd_set_frame_clouds) and registration against them --------------------
    @staticmethod
    def _frame_ids(frames):
        f = np.asarray(frames).reshape(-1)
        if f.size and (not np.issubdtype(f.dtype, np.integer) or f.min() < 0 or f.max() > 0xFFFFFFFF):
            raise ValueError("frames: frame ids (integers, not negative)")
        return np.ascontiguousarray(f, np.uint32)

    def set_frame_clouds(self, frames, clouds, k_neighbors=20, plane_eps=1e-3):
        """sgtd_set_frame_clouds: the dense clouds of map frames, kept on the device with their covariances (84 bytes a
        point), the targets of register_stored / register_loops_stored.  frames: the frame ids; clouds: a list of (n, 3 or
        4) f32 arrays, one per id, or (points, pt_off) with the clouds back to back (points numpy or a torch.cuda tensor)
        and the len(frames) + 1 offsets; clouds=None forgets the clouds of those ids, and frames=None with clouds=None
        forgets all (and the settings).  The first call fixes k_neighbors and plane_eps until all are forgotten."""
        if frames is None:
            if clouds is not None:
                raise ValueError("frames=None forgets all clouds: clouds must be None")
            self._check(self._L.sgtd_set_frame_clouds(self._h, None, None, None, 3, 0, 0, 0.0, 0))
            return
        ids = self._frame_ids(frames)
        if clouds is None:
            if ids.size:
                self._check(self._L.sgtd_set_frame_clouds(self._h, _p(ids), None, None, 3, ids.size, 0, 0.0, 0))
            return
        if isinstance(k_neighbors, bool) or not isinstance(k_neighbors, (int, np.integer)) or not 3 <= k_neighbors <= 32:
            raise ValueError("k_neighbors: an integer in 3..32")
        if not (np.isfinite(plane_eps) and plane_eps > 0):
            raise ValueError("plane_eps: finite and > 0")
        if isinstance(clouds, tuple) and len(clouds) == 2 and not isinstance(clouds[0], (list, tuple)) and np.ndim(clouds[1]) == 1 \
                and getattr(clouds[0], "ndim", 0) == 2:
            points, off = clouds
            off = np.ascontiguousarray(np.asarray(off).reshape(-1), np.int64)
        else:
            arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in clouds]
            strides = {a.shape[1] for a in arrs if a.ndim == 2}
            if any(a.ndim != 2 for a in arrs) or len(strides) > 1 or not strides <= {3, 4}:
                raise ValueError("clouds: (n, 3) or (n, 4) arrays of one width")
            stride = strides.pop() if strides else 3
            off = np.concatenate([[0], np.cumsum([a.shape[0] for a in arrs])]).astype(np.int64)
            points = np.concatenate(arrs) if arrs else np.zeros((0, stride), np.float32)
        if off.size != ids.size + 1:
            raise ValueError("clouds: one cloud (len(frames) + 1 offsets) per frame id")
        if ids.size == 0:
            return
        if not hasattr(points, "data_ptr") and len(points) == 0:
            points = np.zeros((1, np.shape(points)[1] if np.ndim(points) == 2 else 3), np.float32)     # (a non-NULL array: NULL forgets)
        shape, pp, dev = self._points_arg(points, "clouds")
        if off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] > shape[0]:
            raise ValueError("pt_off: from 0, not decreasing, within the points given")
        self._check(self._L.sgtd_set_frame_clouds(self._h, _p(ids), _p(off), pp, int(shape[1]), ids.size, int(k_neighbors), float(plane_eps), dev))

    # ---- voxel-grid thinning of raw clouds on the device (sgtd_thin_clouds) -------------------------------------
    def _thin_args(self, points, pt_off, leaf, what="points", per_query=False):
        """thin_clouds' arguments, checked before the library is called -> (pointer, stride, offsets, device_ptrs)"""
        if isinstance(leaf, bool) or not isinstance(leaf, (int, float, np.integer, np.floating)) or not (np.isfinite(leaf) and leaf > 0):
            raise ValueError("leaf: finite and > 0")
        if hasattr(points, "data_ptr"):
            if not (points.is_cuda and points.is_contiguous()):
                raise ValueError(what + ": a contiguous torch.cuda tensor")
            shape, pp, dev = tuple(points.shape), C.c_void_p(points.data_ptr()), 1
        else:
            points = np.ascontiguousarray(points, dtype=np.float32)
            shape, pp, dev = points.shape, _p(points), 0
        self._keep = points
        if len(shape) not in (2, 3) or shape[-1] not in (3, 4) or (len(shape) == 3 and pt_off is not None):
            raise ValueError(what + ": (total, 3 or 4), or (S, N, 3 or 4) without offsets")
        total = int(np.prod(shape[:-1]))
        if pt_off is None:
            off = np.arange(shape[0] + 1, dtype=np.int64) * shape[1] if len(shape) == 3 else np.array([0, total], np.int64)
        else:
            off = np.ascontiguousarray(np.asarray(pt_off).reshape(-1), np.int64)
        if per_query and off.size != self._nq + 1:
            raise ValueError("pt_off: n_queries + 1 offsets")
        if off.size < 1 or off[0] != 0 or np.any(np.diff(off) < 0) or off[-1] > total:
            raise ValueError("pt_off: n_clouds + 1 offsets from 0, not decreasing, within the points given")
        return pp, int(shape[-1]), off, dev

    def thin_clouds(self, points, pt_off=None, leaf=0.25, fetch=True):
        """sgtd_thin_clouds: ingest.voxel_downsample of a batch of clouds on the device, bit for bit (but points whose cell
        lies outside +-2^20 cells are dropped and counted).  points: (total, 3 or 4) f32 with the n_clouds + 1 offsets
        pt_off (None: one cloud), or (S, N, 3 or 4) without offsets; numpy or a torch.cuda tensor.  -> dict of points
        (n, 3 or 4) f32, pt_off (n_clouds + 1,) i64 and n_dropped (n_clouds, 2) i32: non-finite, out of range.  fetch=False
        leaves the points on the device: the dict holds pt_off and points as a DevicePoints (pointer, stride, count), which
        set_frame_clouds((points, pt_off)) and the register calls take like a torch.cuda tensor."""
        pp, stride, off, dev = self._thin_args(points, pt_off, leaf)
        self._check(self._L.sgtd_thin_clouds(self._h, pp, stride, _p(off), off.size - 1, float(leaf), dev))
        self._thin_n = off.size - 1      # (after the call: one that is refused leaves the earlier results, and their count)
        return self.thin_results(fetch)

    def thin_results(self, fetch=True):
        """the results of the last thin_clouds call, as it returns them"""
        out_off, n = np.zeros(self._thin_n + 1, np.int64), C.c_int64(0)
        if not fetch:
            ptr, stride = C.c_void_p(), C.c_int(0)
            self._check(self._L.sgtd_thinned_device_view(self._h, C.byref(ptr), C.byref(stride), C.byref(n)))
            self._check(self._L.sgtd_result_thinned(self._h, _p(out_off), None, None, 0, None))
            return {"points": DevicePoints(ptr.value, stride.value, n.value), "pt_off": out_off}
        stride = C.c_int(0)
        self._check(self._L.sgtd_thinned_device_view(self._h, None, C.byref(stride), C.byref(n)))
        pts, dropped = np.zeros((n.value, stride.value), np.float32), np.zeros((self._thin_n, 2), np.int32)
        self._check(self._L.sgtd_result_thinned(self._h, _p(out_off), _p(pts), _p(dropped), n.value, C.byref(n)))
        return {"points": pts, "pt_off": out_off, "n_dropped": dropped}

    def thin_stage_ms(self):
        """device milliseconds of the last thin_clouds call: the sorts, the rest, the whole call (zeros unless
        set_timing(True))"""
        return self._stage_ms(self._L.sgtd_thin_stage_ms, 3)

    def _thin_first(self, points, pt_off, leaf, what, per_query=False):
        """the leaf= forms: the call's clouds thinned on the device -> (points, pt_off) as the register calls take them"""
        pp, stride, off, dev = self._thin_args(points, pt_off, leaf, what, per_query)
        self._check(self._L.sgtd_thin_clouds(self._h, pp, stride, _p(off), off.size - 1, float(leaf), dev))
        self._thin_n = off.size - 1
        view = self.thin_results(fetch=False)
        return view["points"], view["pt_off"]

    def set_frame_scans(self, frames, scans, leaf, k_neighbors=20, plane_eps=1e-3):
        """thin_clouds, then set_frame_clouds on the thinned clouds where they lie on the device: no point crosses back.
        frames: the frame ids; scans: the raw scans as set_frame_clouds takes clouds (a list of (n, 3 or 4) f32 arrays, or
        (points, pt_off)); leaf: the voxel size.  Returns the thinned clouds' offsets."""
        ids = self._frame_ids(frames)
        if isinstance(scans, tuple) and len(scans) == 2 and not isinstance(scans[0], (list, tuple)) and np.ndim(scans[1]) == 1 \
                and getattr(scans[0], "ndim", 0) == 2:
            points, off = scans
        else:
            arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in scans]
            strides = {a.shape[1] for a in arrs if a.ndim == 2}
            if any(a.ndim != 2 for a in arrs) or len(strides) != 1 or not strides <= {3, 4}:
                raise ValueError("scans: (n, 3) or (n, 4) arrays of one width")
            off = np.concatenate([[0], np.cumsum([a.shape[0] for a in arrs])]).astype(np.int64)
            points = np.concatenate(arrs)
        if np.size(off) != ids.size + 1:
            raise ValueError("scans: one scan (len(frames) + 1 offsets) per frame id")
        d_points, out_off = self._thin_first(points, off, leaf, "scans")
        self.set_frame_clouds(ids, (d_points, out_off), k_neighbors, plane_eps)
        return out_off

    def frame_clouds_info(self):
        """-> dict of n_frames, n_points (live), device_bytes (the arena's arrays), k_neighbors and plane_eps (0 while the
        store has no settings)"""
        a, b, c, k, e = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_double(0)
        self._check(self._L.sgtd_frame_clouds_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(k), C.byref(e)))
        return {"n_frames": a.value, "n_points": b.value, "device_bytes": c.value, "k_neighbors": k.value, "plane_eps": e.value}

    def frame_cloud(self, frame):
        """the stored cloud of one frame: (xyz (n, 3) f32, cov (n, 3, 3) f64), or None where the frame has none"""
        n = C.c_int64(0)
        self._check(self._L.sgtd_result_frame_cloud(self._h, int(frame), None, None, 0, C.byref(n)))
        if n.value < 0:
            return None
        xyz, cov = np.zeros((n.value, 3), np.float32), np.zeros((n.value, 3, 3), np.float64)
        self._check(self._L.sgtd_result_frame_cloud(self._h, int(frame), _p(xyz), _p(cov), n.value, C.byref(n)))
        return xyz, cov

    def register_stored(self, points, pt_off, src, tgt_frame, init=None, leaf=None, **options):
        """sgtd_register_stored: register_clouds with the targets read from the cloud store.  points, pt_off: the call's
        clouds as register_clouds takes them; src: (n,) cloud indices; tgt_frame: (n,) frame ids that have a stored cloud;
        init, options and the returned dict as register_clouds'.  The results are register_clouds' on the call's clouds
        followed by the frames' stored clouds, bit for bit.  leaf: a number thins the call's clouds on the device first
        (thin_clouds) and registers them from there; None takes them as they are."""
        if leaf is not None:
            points, pt_off = self._thin_first(points, pt_off, leaf, "points")
        shape, pp, dev = self._points_arg(points)
        off = self._offsets(pt_off, shape)
        s, t, p0, n = self._pairs_arg(src, tgt_frame, init, "src and tgt_frame: one cloud index and one frame id per pair", tgt_ids=True)
        opt = self._options(RegisterOptions, self._L.sgtd_default_register_options, options)
        self._check(self._L.sgtd_register_stored(self._h, C.byref(opt), pp, int(shape[1]), _p(off), off.size - 1, _p(s), _p(t), _p(p0), n, dev))
        self._stored_n = n
        return self.result_stored_registered()

    def result_stored_registered(self):
        return self._rows_dict(self._L.sgtd_result_stored_registered, self._stored_n, False)

    def register_loops_stored(self, query_points, query_pt_off, max_per_query=5, start="verify", leaf=None, **options):
        """sgtd_register_stored_loops, after verify(): register_loops with the map clouds read from the cloud store and the
        pairs formed on the device (register_pairs' rule; a candidate whose frame has no stored cloud is dropped).
        query_points: (total, 3 or 4) f32, numpy or a torch.cuda tensor, with the n_queries + 1 offsets query_pt_off.
        leaf: a number thins the query clouds on the device first (thin_clouds); None takes them as they are.
        -> register_loops' dict: query, cand, frame [m] (int32), init [m, 12] and register_clouds' fields per pair"""
        code = self._loops_args(start, max_per_query)
        if leaf is not None:
            query_points, query_pt_off = self._thin_first(query_points, query_pt_off, leaf, "query_points", per_query=True)
        shape, pp, dev = self._points_arg(query_points, "query_points")
        qoff = self._offsets(query_pt_off, shape, "query_pt_off", per_query=True)
        opt = self._options(RegisterOptions, self._L.sgtd_default_register_options, options)
        self._check(self._L.sgtd_register_stored_loops(self._h, C.byref(opt), pp, int(shape[1]), _p(qoff), int(max_per_query), code, dev))
        q, c, f, init = self._sized(self._L.sgtd_result_stored_pairs, (), (((), np.int32),) * 3 + (((12,), np.float64),))
        self._stored_n = len(q)
        out = self.result_stored_registered()
        out.update(query=q, cand=c, frame=f, init=init)
        return out

    def stored_covariances(self, cloud):
        """the regularised covariances of one of the call's clouds of the last register_stored / register_loops_stored
        call: (n, 3, 3) f64; 0 rows for a cloud no pair named"""
        return self._sized(self._L.sgtd_result_stored_covariances, (int(cloud),), (((3, 3), np.float64),))[0]

    def stored_matches(self, pair):
        """the correspondences of one pair under its final pose: (tgt_index (n,) int32 within the frame's stored cloud, -1
        where none; d2 (n,) f64)"""
        return tuple(self._sized(self._L.sgtd_result_stored_matches, (int(pair),), (((), np.int32), ((), np.float64))))

    def stored_register_stage_ms(self):
        """device milliseconds of the last register_stored / register_loops_stored call: covariances, searches, the rest,
        the whole run (zeros unless set_timing(True))"""
        return self._stage_ms(self._L.sgtd_stored_register_stage_ms, 4)

    # ---- voxelised registration against voxel maps (sgtd_register_voxels) -------------------------------------
    def register_voxels(self, points, pt_off, map_off, map_cloud, map_pose, src, tgt_map, init=None, **options):
        """sgtd_register_voxels: voxelised GICP of clouds against maps of Gaussian voxels on the device.  points, pt_off:
        as register_clouds; map m has the members map_cloud[map_off[m]:map_off[m + 1]] (cloud indices), posed by map_pose
        (members, 12) in the rel_pose layout (x = R p + t takes a member's point into the map's frame), None = the
        identity; src, tgt_map: (n,) the pairs' source clouds and target maps; init: (n, 12) start poses, None = the
        identity; options: fields of sgtd_voxel_register_options.  -> result_voxel_registered()"""
        shape, pp, dev = self._points_arg(points)
        off = self._offsets(pt_off, shape)
        moff, mcl, mp = self._maps_arg(map_off, map_cloud, map_pose)
        s, t, p0, n = self._pairs_arg(src, tgt_map, init, "src and tgt_map: one cloud and one map index per pair")
        opt = self._options(VoxelRegisterOptions, self._L.sgtd_default_voxel_register_options, options)
        self._check(self._L.sgtd_register_voxels(self._h, C.byref(opt), pp, int(shape[1]), _p(off), off.size - 1, _p(moff), _p(mcl), _p(mp),
                                                 moff.size - 1, _p(s), _p(t), _p(p0), n, dev))
        self._vreg_n = n
        return self.result_voxel_registered()

    def result_voxel_registered(self):
        """-> dict of pose [n, 12], fitness [n], cost [n, 2] (first and last linearisation), n_matched, n_corr, iterations,
        status [n] (int32) of the last register_voxels call"""
        return self._rows_dict(self._L.sgtd_result_voxel_registered, self._vreg_n, True)

    def voxel_map(self, m):
        """the voxels of map m of the last register_voxels call, in their numbering -> dict of coord (v, 3) int32,
        n_points (v,) int32, mean (v, 3), cov (v, 3, 3) f64"""
        return dict(zip(("coord", "n_points", "mean", "cov"), self._sized(self._L.sgtd_result_voxel_map, (int(m),), self._VOXEL_KINDS)))

    def voxel_matches(self, pair):
        """the correspondences of one pair under its final pose: (n_src, mode) int32, the voxel's index within the map per
        offset, -1 where there is none"""
        return self._sized(self._L.sgtd_result_voxel_matches, (int(pair),), (((), np.int32),))[0]

    def voxel_register_stage_ms(self):
        """device milliseconds of the last register_voxels call: covariances, map build, correspondence passes, the rest,
        the whole call (zeros unless set_timing(True))"""
        return self._stage_ms(self._L.sgtd_voxel_register_stage_ms, 5)

    # ---- voxel maps whose members are stored clouds (sgtd_register_stored_voxels) -------------------------------
    def register_stored_voxels(self, points, pt_off, map_off, map_frame, map_pose, src, tgt_map, init=None, leaf=None, **options):
        """sgtd_register_stored_voxels: register_voxels with the maps' members read from the cloud store.  points,
        pt_off: the call's clouds (the sources), numpy or a torch.cuda tensor; map m has the members
        map_frame[map_off[m]:map_off[m + 1]], frame ids that have a stored cloud (set_frame_clouds); map_pose, src,
        tgt_map, init, options and the returned dict as register_voxels'.  The results are register_voxels' on the call's
        clouds followed by the members' stored clouds, bit for bit; k_neighbors and plane_eps must be the store's.
        leaf: a number thins the call's clouds on the device first (thin_clouds); None takes them as they are."""
        if leaf is not None:
            points, pt_off = self._thin_first(points, pt_off, leaf, "points")
        shape, pp, dev = self._points_arg(points)
        off = self._offsets(pt_off, shape)
        moff, mfr, mp = self._maps_arg(map_off, map_frame, map_pose, frame_ids=True)
        s, t, p0, n = self._pairs_arg(src, tgt_map, init, "src and tgt_map: one cloud and one map index per pair")
        opt = self._options(VoxelRegisterOptions, self._L.sgtd_default_voxel_register_options, options)
        self._check(self._L.sgtd_register_stored_voxels(self._h, C.byref(opt), pp, int(shape[1]), _p(off), off.size - 1, _p(moff), _p(mfr), _p(mp),
                                                        moff.size - 1, _p(s), _p(t), _p(p0), n, dev))
        self._svreg_n = n
        return self.result_stored_voxel_registered()

    def result_stored_voxel_registered(self):
        """-> result_voxel_registered()'s dict of the last register_stored_voxels call"""
        return self._rows_dict(self._L.sgtd_result_stored_voxel_registered, self._svreg_n, True)

    def stored_voxel_map(self, m):
        """the voxels of map m of the last register_stored_voxels call -> voxel_map()'s dict"""
        return dict(zip(("coord", "n_points", "mean", "cov"), self._sized(self._L.sgtd_result_stored_voxel_map, (int(m),), self._VOXEL_KINDS)))

    def stored_voxel_matches(self, pair):
        """the correspondences of one pair of the last register_stored_voxels call, as voxel_matches()"""
        return self._sized(self._L.sgtd_result_stored_voxel_matches, (int(pair),), (((), np.int32),))[0]

    def register_loops_local_stored(self, query_points, query_pt_off, radius=15.0, max_members=0, max_per_query=5, start="verify", leaf=None,
                                    **options):
        """sgtd_register_stored_local_loops, after verify(): register_loops_local with the map clouds read from the cloud
        store (set_frame_clouds), the frames' poses from set_frame_poses, and the pairs, the local maps and the members'
        relative poses formed on the device.  A candidate whose frame has no stored cloud, no stored pose or a pose that
        is not finite is dropped.  With max_members = m > 0 a map keeps its frame and the m - 1 nearest others (ties to
        the smaller id), not voxel_map_members' first m in id order.  query_points: (total, 3 or 4) f32, numpy or a
        torch.cuda tensor, with the n_queries + 1 offsets query_pt_off.  -> register_loops_local's dict: query, cand, frame,
        tgt_map [m] (int32), init [m, 12], register_voxels' fields per pair, map_frames, members (per map, the member frame
        ids), map_off, map_frame, map_pose as register_stored_voxels takes them.  leaf: a number thins the query clouds on
        the device first (thin_clouds); None takes them as they are."""
        code = self._loops_args(start, max_per_query, max_members, radius)
        if leaf is not None:
            query_points, query_pt_off = self._thin_first(query_points, query_pt_off, leaf, "query_points", per_query=True)
        shape, pp, dev = self._points_arg(query_points, "query_points")
        qoff = self._offsets(query_pt_off, shape, "query_pt_off", per_query=True)
        opt = self._options(VoxelRegisterOptions, self._L.sgtd_default_voxel_register_options, options)
        self._check(self._L.sgtd_register_stored_local_loops(self._h, C.byref(opt), pp, int(shape[1]), _p(qoff), int(max_per_query), code,
                                                             float(radius), int(max_members), dev))
        q, c, f, tgt, init = self.stored_local_pairs()
        self._svreg_n = len(q)
        out = self.result_stored_voxel_registered()
        maps = self.stored_local_maps()
        out.update(query=q, cand=c, frame=f, tgt_map=tgt, init=init, src_cloud=q.copy(), map_frames=maps["map_frame"].tolist(),
                   members=[maps["member"][a:b].astype(np.int32) for a, b in zip(maps["mem_off"][:-1], maps["mem_off"][1:])],
                   map_off=maps["mem_off"].astype(np.int32), map_frame=maps["member"], map_pose=maps["member_pose"])
        return out

    def stored_local_pairs(self):
        """the rows of the last register_loops_local_stored call -> (query, cand, frame, tgt_map [m] int32, init [m, 12])"""
        return tuple(self._sized(self._L.sgtd_result_stored_local_pairs, (), (((), np.int32),) * 4 + (((12,), np.float64),)))

    def stored_local_maps(self):
        """the maps of the last register_loops_local_stored call -> dict of map_frame [maps] (uint32, ascending), mem_off
        [maps + 1] (int64), member [members] (uint32: a map's own frame first, the others in ascending id) and member_pose
        [members, 12] (T_frame^-1 T_member; the identity for the frame itself)"""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self._L.sgtd_result_stored_local_maps(self._h, None, None, None, None, 0, 0, C.byref(a), C.byref(b)))
        out = {"map_frame": np.zeros(a.value, np.uint32), "mem_off": np.zeros(a.value + 1, np.int64), "member": np.zeros(b.value, np.uint32),
               "member_pose": np.zeros((b.value, 12), np.float64)}
        self._check(self._L.sgtd_result_stored_local_maps(self._h, _p(out["map_frame"]), _p(out["mem_off"]), _p(out["member"]), _p(out["member_pose"]),
                                                          a.value, b.value, C.byref(a), C.byref(b)))
        return out

    def stored_voxel_register_stage_ms(self):
        """device milliseconds of the last register_stored_voxels call: covariances (of the call's clouds alone), map
        build, correspondence passes, the rest, the whole call (zeros unless set_timing(True))"""
        return self._stage_ms(self._L.sgtd_stored_voxel_register_stage_ms, 5)

    @staticmethod
    def voxel_map_members(frame, frame_poses, has_cloud, radius=15.0, max_members=0):
        """the members of the local map around `frame`: the frames that have a cloud and a pose whose position lies within
        `radius` of the frame's, the frame itself first, then in ascending frame id, the first max_members of them (0 = no
        cap).  frame_poses: a dict or sequence by frame id of 12 doubles (rot row-major, t: the frame in the world);
        has_cloud(id) -> bool.  -> (members [k] int32, rel [k, 12] f64: T_frame^-1 T_member, composed in f64)"""
        ids = sorted(frame_poses.keys()) if isinstance(frame_poses, dict) else range(len(frame_poses))
        pose = lambda f: np.asarray(frame_poses[f], np.float64).reshape(12)
        Rf, tf = pose(frame)[:9].reshape(3, 3), pose(frame)[9:]
        members = [int(frame)]
        for f in ids:
            if int(f) == int(frame) or frame_poses[f] is None or not has_cloud(int(f)):
                continue
            d = pose(f)[9:] - tf
            if float(d @ d) <= float(radius) * float(radius):
                members.append(int(f))
        if max_members:
            members = members[:int(max_members)]
        rel = np.zeros((len(members), 12), np.float64)
        for k, f in enumerate(members):
            Rm, tm = pose(f)[:9].reshape(3, 3), pose(f)[9:]
            rel[k, :9] = (Rf.T @ Rm).reshape(9)
            rel[k, 9:] = Rf.T @ (tm - tf)
        return np.array(members, np.int32), rel

    def register_loops_local(self, query_points, query_pt_off, map_clouds, frame_poses, radius=15.0, max_members=0, max_per_query=5,
                             start="verify", **options):
        """register_loops against local maps: for register_pairs' (query, frame) pairs the target is the voxel map of the
        candidate frame's local map (voxel_map_members: the frames with a cloud within `radius` of the candidate's
        position, the candidate first, each posed by T_frame^-1 T_member), one map per distinct candidate frame shared
        among the queries, in ONE register_voxels call.  frame_poses: by frame id, 12 doubles (rot row-major, t); a
        candidate without a cloud or a pose is skipped.  -> what register_loops returns (register_voxels' fields per
        pair) plus tgt_map [m], map_frames (the maps' candidate frames) and members (per map, the member frame ids),
        map_off, map_cloud, map_pose as given to the call.  evaluate.choose_registered works on its fitness."""
        pack = self._loop_clouds(query_points, query_pt_off, map_clouds)
        q, c, f, init = self.register_pairs(max_per_query, start)
        has_cloud = lambda i: self._by_frame(map_clouds, i) is not None
        has = np.array([has_cloud(int(x)) and self._by_frame(frame_poses, int(x)) is not None for x in f], bool)
        q, c, f, init = q[has], c[has], f[has], init[has]
        map_frames = sorted(set(int(x) for x in f))
        members, rels = [], []
        for x in map_frames:
            m, rel = self.voxel_map_members(x, frame_poses, has_cloud, radius, max_members)
            members.append(m)
            rels.append(rel)
        pts, off, slot = pack(sorted(set(int(i) for m in members for i in m)))
        map_off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
        map_cloud = np.array([slot[int(i)] for m in members for i in m], np.int32)
        map_pose = np.concatenate(rels).reshape(-1, 12) if rels else np.zeros((0, 12))
        map_slot = {x: k for k, x in enumerate(map_frames)}
        tgt = np.array([map_slot[int(x)] for x in f], np.int32)
        out = self.register_voxels(pts, off, map_off, map_cloud, map_pose, q, tgt, init if len(q) else None, **options)
        out.update(query=q, cand=c, frame=f, init=init, src_cloud=q.copy(), tgt_map=tgt, points=pts, pt_off=off, map_frames=map_frames,
                   members=members, map_off=map_off, map_cloud=map_cloud, map_pose=map_pose)
        return out

    def search_frame(self, stds_vec, capacity=16384, page_locked=False, lists_only=False, allowed=None, prior=None):
        """sgtd_search_frame: candidate_selector + candidate_verify + the inlier pairs of every candidate with their table
        entries for ONE query frame given as descriptors, in one call -> dict(n_cand, cand_frame, cand_votes, pair_off,
        score, rot, t, inlier_off, inlier_q_idx, entries (Descs), n_inliers, status).  page_locked: the arrays the inlier
        pairs arrive in come from sgtd_host_alloc, as adapter/STDesc_shim.hpp keeps them — the device then writes them in
        place and the call has one wait (ordinary arrays are filled from the handle's own page-locked block).
        lists_only (SGTD_FRAME_LISTS_ONLY): candidate_selector alone — no verification, inlier_off = pair_off and the pairs
        handed back are all pairs of every candidate's match list.  allowed: a frame filter for this call only
        (set_frame_filter); prior: (center, radius), a position prior for this call only (set_position_prior)"""
        if prior is not None:
            return self._with_prior(prior, lambda: self.search_frame(stds_vec, capacity, page_locked, lists_only, allowed))
        if allowed is not None:
            return self._with_filter(allowed, lambda: self.search_frame(stds_vec, capacity, page_locked, lists_only))
        from ._lib import FrameSearch
        cn = self.config_setting_["candidate_num"]
        cap = max(int(capacity), 1)
        out = dict(cand_frame=np.zeros(cn, np.int32), cand_votes=np.zeros(cn, np.int32), pair_off=np.zeros(cn + 1, np.int64),
                   score=np.zeros(cn, np.float64), pose=np.zeros((cn, 12), np.float64), inlier_off=np.zeros(cn + 1, np.int64))
        blocks = []
        if page_locked:
            def room(dt, w):
                p = C.c_void_p()
                self._check(self._L.sgtd_host_alloc(cap * w * np.dtype(dt).itemsize, C.byref(p)))
                blocks.append(p)
                a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_ubyte)), shape=(cap * w * np.dtype(dt).itemsize,)).view(dt)
                return a.reshape((cap, w)) if w > 1 else a
            ent = Descs(0)
            ent.n = cap
            for name, dt, w in Descs.FIELDS:
                setattr(ent, name, room(dt, w))
            out["inlier_q_idx"] = room(np.int32, 1)
        else:
            ent = Descs(cap)
            out["inlier_q_idx"] = np.zeros(cap, np.int32)
        try:
            fs = FrameSearch()
            for k in ("cand_frame", "cand_votes", "pair_off", "score", "pose", "inlier_off", "inlier_q_idx"):
                setattr(fs, k, out[k].ctypes.data)
            fs.entries = ent.soa()
            fs.capacity = int(capacity)
            fs.flags = 1 if lists_only else 0
            s = stds_vec.soa()
            self._nq = 1
            st = self._L.sgtd_search_frame(self._h, C.byref(s), stds_vec.n, C.byref(fs))
            if st not in (0, -4):
                self._check(st)
            n = int(fs.n_inliers)
            out.update(status=st, n_cand=int(fs.n_cand), n_inliers=n, rot=out["pose"][:, :9].reshape(cn, 3, 3).copy(), t=out["pose"][:, 9:].copy(),
                       inlier_q_idx=out["inlier_q_idx"][:min(n, capacity)].copy(), entries=ent.head(min(n, capacity)))
            if page_locked:     # (head() of a contiguous slice is a view: the results leave the block before it is given back)
                for name, _, _ in Descs.FIELDS:
                    setattr(out["entries"], name, getattr(out["entries"], name).copy())
        finally:
            ent = None
            for p in blocks:
                self._L.sgtd_host_free(p)
        return out

    def SearchLoop(self, stds_vec, icp_threshold=None):
        """mirror of STDescManager::SearchLoop (STDesc.cpp:84-147) for one query given as
        descriptors -> (loop_result (frame, score), (t, rot), success pair positions,
        match_result_list [(frame, score, (t, rot), positions)])"""
        if stds_vec.n == 0:                       # "No STDescs!" (:89-93)
            return (-1, 0.0), None, np.zeros(0, np.int32), []
        cands = self.candidate_selector(stds_vec)
        self.verify()
        score, rot, t = self.result_verify(0)
        mrl = []
        for k, c in enumerate(cands):
            inl = self.result_inliers(0, k, len(c.q_idx)) if score[k] >= 0 else np.zeros(0, np.int32)
            mrl.append((int(c.match_id_[1]), float(score[k]), (t[k], rot[k]), inl))
        bc, bf, bs = self.search_loop(icp_threshold)
        if bf[0] < 0:
            return (-1, 0.0), None, np.zeros(0, np.int32), mrl
        k = int(bc[0])
        return (int(bf[0]), float(bs[0])), (t[k], rot[k]), mrl[k][3], mrl

    # ---- persistent table
    def save_table(self, path):
        self._check(self._L.sgtd_save_table(self._h, os.fspath(path).encode()))

    def load_table(self, path):
        """replace this manager's table with a saved one; AddSTDescs / add_frames keep appending"""
        self._check(self._L.sgtd_load_table(self._h, os.fspath(path).encode()))

    def fetch_entries(self, db_entry):
        db_entry = np.ascontiguousarray(db_entry, dtype=np.int64)
        d = Descs(len(db_entry))
        s = d.soa()
        self._check(self._L.sgtd_fetch_entries(self._h, _p(db_entry), len(db_entry), C.byref(s)))
        return d

    def table_dump(self):
        self.finalize()
        # the dump shows whole buckets: a table with a tail segment is merged first (the sizing
        # call below does it and reports the capacity it needs)
        self._L.sgtd_table_dump(self._h, None, None, None, 0, 0)
        st = self.stats()
        u, e = st["n_buckets"], st["n_entries"]
        keys = np.zeros((u, 4), np.int64)
        off = np.zeros(u + 1, np.int64)
        ids = np.zeros(e, np.int64)
        self._check(self._L.sgtd_table_dump(self._h, _p(keys), _p(off), _p(ids), u, e))
        return keys, off, ids
