"""The contract of gloc_scan_store_add_submap(s) restated in numpy, bit for bit (include/gloc3d.h, "local submaps").

Every fp32 operation of the device kernels is an individually rounded one (no fused multiply-add), so numpy float32
arithmetic reproduces it; the per-cell sums are fp64 additions in a fixed order, reproduced one addend at a time.
Test infrastructure: the product never imports this file.
"""
import numpy as np

KEY_BIAS = 1 << 20


def _keys(xyz, T, leaf, max_range):
    """q [n, 3] float32, k [n, 3] int64 and the mask of the points that are used, of one member."""
    p = np.ascontiguousarray(xyz, np.float32)[:, :3]
    T = np.asarray(T, np.float32).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        if max_range > 0:
            mr = np.float32(max_range)
            r2 = (x * x + y * y) + z * z
            ok &= ~(r2 > mr * mr)
        inv = np.float32(1.0) / np.float32(leaf)
        q = np.empty((p.shape[0], 3), np.float32)
        k = np.zeros((p.shape[0], 3), np.int64)
        for a in range(3):
            q[:, a] = ((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]
            f = np.floor(q[:, a] * inv)
            assert f.dtype == np.float32
            ok &= np.abs(f) < np.float32(KEY_BIAS)          # False for NaN; an infinite q gives an infinite or NaN f
            k[:, a] = np.where(ok, f, 0).astype(np.int64)
    return q, k, ok


def ordered_sums(v, start, length):
    """Per run r the sum of v[start[r] : start[r] + length[r]] (float64 rows), accumulated one addend after the other in
    index order -- vectorised over the runs, never over the addends of one run."""
    order = np.argsort(-length, kind="stable")              # longest first: the runs still active at step t are a prefix
    st, ln = start[order], length[order]
    acc = np.zeros((len(start),) + v.shape[1:], np.float64)
    for t in range(int(ln[0]) if len(ln) else 0):
        na = int(np.searchsorted(-ln, -t, side="left"))     # runs with length > t
        acc[:na] += v[st[:na] + t]
    out = np.empty_like(acc)
    out[order] = acc
    return out


def submap(members, leaf=0.2, min_points=1, min_scans=1, max_range=0.0):
    """members: [(xyz [n, 3|4] float32, T [4, 4])], in list order.  Returns (points [kept, 3] float32 in cell order, info
    dict(points_in, points_used, cells, kept, cell_keys [kept, 3] int64)); kept = 0 is the library's GLOC_ERR_INVALID."""
    qs, ks, oks, mem = [], [], [], []
    for m, (xyz, T) in enumerate(members):
        q, k, ok = _keys(xyz, T, leaf, max_range)
        qs.append(q), ks.append(k), oks.append(ok), mem.append(np.full(q.shape[0], m, np.int64))
    q, k, ok, mem = np.concatenate(qs), np.concatenate(ks), np.concatenate(oks), np.concatenate(mem)
    info = dict(points_in=int(q.shape[0]), points_used=int(ok.sum()), cells=0, kept=0, cell_keys=np.zeros((0, 3), np.int64))
    q, k, mem = q[ok], k[ok], mem[ok]                        # (the concatenation's order is kept)
    if q.shape[0] == 0:
        return np.zeros((0, 3), np.float32), info
    order = np.lexsort((k[:, 2], k[:, 1], k[:, 0]))          # stable: ascending (kx, ky, kz), then the concatenation's order
    q, k, mem = q[order], k[order], mem[order]
    new = np.ones(q.shape[0], bool)
    new[1:] = (k[1:] != k[:-1]).any(axis=1)
    start = np.nonzero(new)[0]
    length = np.diff(np.append(start, q.shape[0]))
    sums = ordered_sums(q.astype(np.float64), start, length)
    cent = (sums / length[:, None].astype(np.float64)).astype(np.float32)
    newm = new.copy()
    newm[1:] |= mem[1:] != mem[:-1]                          # (member positions ascend inside a run)
    scans = np.add.reduceat(newm.astype(np.int64), start)
    keep = (length >= max(int(min_points), 1)) & (scans >= max(int(min_scans), 1))
    info.update(cells=int(len(start)), kept=int(keep.sum()), cell_keys=k[start][keep])
    return np.ascontiguousarray(cent[keep]), info
