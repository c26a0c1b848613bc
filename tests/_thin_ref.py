"""sgtd_thin_clouds restated from its rule (include/sgtd_accel.h) in plain numpy and Python: no call of
ingest.voxel_downsample, no sort, no unique.  A dict keyed by the cell keeps the cells in the order their first points
arrive, and Python's float is the f64 whose additions the rule spells out one by one."""
import numpy as np

MAX_CELL = 1 << 20      # SGTD_THIN_MAX_CELL


def thin_cloud(points, leaf):
    """one cloud -> (thinned (m, stride) f32, (non-finite, out of range) drop counts)"""
    p = np.asarray(points, np.float32)
    assert p.ndim == 2 and p.shape[1] in (3, 4)
    stride = p.shape[1]
    wide = p.astype(np.float64)                                   # exact
    with np.errstate(over="ignore", invalid="ignore"):
        cell = np.floor(wide[:, :3] / np.float64(leaf))           # one division, rounded once, then floor
    finite = np.isfinite(wide[:, :3]).all(axis=1)
    with np.errstate(invalid="ignore"):
        inside = ((cell >= -float(MAX_CELL)) & (cell < float(MAX_CELL))).all(axis=1)
    sums, n_bad, n_out = {}, 0, 0
    for i in range(p.shape[0]):
        if not finite[i]:
            n_bad += 1
            continue
        if not inside[i]:
            n_out += 1
            continue
        key = (int(cell[i, 0]), int(cell[i, 1]), int(cell[i, 2]))
        acc = sums.get(key)
        if acc is None:
            acc = sums[key] = [0.0] * stride + [0]
        for a in range(stride):
            acc[a] = acc[a] + float(wide[i, a])                    # sequential, in ascending point index
        acc[stride] += 1
    out = np.zeros((len(sums), stride), np.float32)
    for r, acc in enumerate(sums.values()):                        # (a dict keeps insertion order: smallest point index)
        for a in range(stride):
            out[r, a] = np.float32(np.float64(acc[a]) / np.float64(acc[stride]))
    return out, (n_bad, n_out)


def thin(points, pt_off, leaf):
    """a batch -> dict of points (n, stride) f32, pt_off (n_clouds + 1,) i64, n_dropped (n_clouds, 2) i32"""
    p = np.asarray(points, np.float32)
    off = np.asarray(pt_off, np.int64).reshape(-1)
    outs, drops = [], []
    for s in range(off.size - 1):
        o, d = thin_cloud(p[off[s]:off[s + 1]], leaf)
        outs.append(o)
        drops.append(d)
    out_off = np.concatenate([[0], np.cumsum([len(o) for o in outs])]).astype(np.int64)
    pts = np.concatenate(outs) if outs else np.zeros((0, p.shape[1] if p.ndim == 2 else 3), np.float32)
    return {"points": pts, "pt_off": out_off, "n_dropped": np.array(drops, np.int32).reshape(-1, 2)}


def pairwise_mean(col, count):
    """(float)(tree sum / count) of one f64 column: what a tree reduction would give — the sums test shows its input tells
    this from the sequential sum"""
    v = [float(x) for x in col]
    while len(v) > 1:
        v = [v[k] + v[k + 1] if k + 1 < len(v) else v[k] for k in range(0, len(v), 2)]
    return np.float32(np.float64(v[0]) / np.float64(count))
