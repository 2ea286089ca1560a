"""Restatement of the radius-support FPFH (include/gloc3d.h: gloc_fpfh_radius_params, R1 - R3) -- the contract of
gloc_scan_store_radius_neighbors / _build_normals_radius / _build_fpfh_radius / _spfh_radius and of the _radius batch entries.
numpy only; everything downstream of the lists is tests/fpfh_ref.py's (F1 - F4) and the CPU checker's normals, handed in.

A support is the tuple (normal_radius, feature_radius, normal_max_nn, feature_max_nn, normal_min_nn)."""
import numpy as np

import fpfh_ref as F

NONE = F.NONE
FLT_MAX = np.finfo(np.float32).max


def radius_lists(xyz, r, max_nn, chunk=512):
    """R1 by brute force in float32: (idx [n, max_nn] uint32, d2 [n, max_nn] float32, count [n] uint32).  d2 is
    ((dx dx + dy dy) + dz dz), every operation rounded to float32; inside iff d2 <= r * r (float32; a NaN is never inside);
    the max_nn smallest in ascending (d2, index) by np.lexsort; 0xFFFFFFFF / FLT_MAX where a list is short."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    r2 = np.float32(r) * np.float32(r)
    idx, d2 = np.full((n, max_nn), NONE, np.uint32), np.full((n, max_nn), FLT_MAX, np.float32)
    count = np.zeros(n, np.uint32)
    for s in range(0, n, chunk):
        p = xyz[s:s + chunk]
        with np.errstate(all="ignore"):
            dx, dy, dz = (p[:, None, a] - xyz[None, :, a] for a in range(3))
            d = (dx * dx + dy * dy) + dz * dz
            rows, cols = np.nonzero(d <= r2)
        dd = d[rows, cols]
        order = np.lexsort((cols, dd, rows))                     # by row, then d2, then index
        rows, cols, dd = rows[order], cols[order], dd[order]
        cnt = np.bincount(rows, minlength=len(p))
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        rank = np.arange(len(rows)) - start[rows]
        keep = rank < max_nn
        idx[s + rows[keep], rank[keep]] = cols[keep]
        d2[s + rows[keep], rank[keep]] = dd[keep]
        count[s:s + len(p)] = cnt
    return idx, d2, count


def normals(xyz, idx, count, max_nn, min_nn, oracle):
    """R2: the checker's normals from the padded lists, none where a list holds fewer than min_nn entries."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if len(xyz) == 0:
        return np.zeros((0, 3), np.float32)
    nrm = oracle.ground_normals(xyz, idx)[0].copy()
    nrm[np.minimum(count, max_nn) < min_nn] = 0.0
    return nrm


def features(xyz, support, oracle, order="forward"):
    """fpfh_ref.features over the support: dict(feat, feat64, counts, used, edge_own, flagged, nrm, idx, d2, count) -- idx, d2,
    count the FEATURE lists -- plus nidx, nd2, ncount, the normals' lists."""
    nr, fr, nmax, fmax, nmin = support
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    nidx, nd2, ncount = radius_lists(xyz, nr, nmax)
    nrm = normals(xyz, nidx, ncount, nmax, nmin, oracle)
    idx, d2, count = radius_lists(xyz, fr, fmax)
    counts, used, edge_own = F.spfh(xyz, nrm, idx, d2)
    f64 = F.fpfh(counts, used, idx, d2, order)
    return dict(feat=f64.astype(np.float32), feat64=f64, counts=counts, used=used, edge_own=edge_own, flagged=F.edge_flags(edge_own, idx),
                nrm=nrm, idx=idx, d2=d2, count=count, nidx=nidx, nd2=nd2, ncount=ncount)


def register(src, tgt, support, oracle, stream_id=0, src_feat=None, tgt_feat=None, **params):
    """F3, F4 on the features of the support (fpfh_ref.register with the features handed in)."""
    fs = features(src, support, oracle)["feat"] if src_feat is None else src_feat
    ft = features(tgt, support, oracle)["feat"] if tgt_feat is None else tgt_feat
    return F.register(src, tgt, oracle, stream_id=stream_id, src_feat=fs, tgt_feat=ft, **params)
