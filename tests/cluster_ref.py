"""Restatement of the Euclidean clusters and outlier filters of resident scans (include/gloc3d.h, E1 - E7) -- the contract of
gloc_scan_store_cluster / _add_filtered / _add_subset.  numpy only.  Every integer output is exact; every float output has a
stated summation order (run_sum below; np.cumsum adds one by one, in order).

fp32 distances are ((dx dx + dy dy) + dz dz) with numpy's un-fused float32 operations, as tests/fpfh_radius_ref.py forms
them; E5's counts are that module's R1 counts."""
import numpy as np

import fpfh_radius_ref as R

NONE = np.uint32(0xFFFFFFFF)
FLT_MAX = np.finfo(np.float32).max


def _xyz(xyz):
    return np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)


def finite_rows(xyz):
    return np.isfinite(_xyz(xyz)).all(axis=1)


def d2_rows(xyz, rows):
    """E1's d2 of the points `rows` (a slice) against every point: [len(rows), n] float32."""
    p = xyz[rows]
    with np.errstate(all="ignore"):
        dx, dy, dz = (p[:, None, a] - xyz[None, :, a] for a in range(3))
        return (dx * dx + dy * dy) + dz * dz


def adjacency(xyz, tolerance, chunk=512):
    """E1 as a dense boolean matrix [n, n]: i ~ j iff both are finite and d2(i, j) <= r2 (the diagonal of a finite point set)."""
    xyz = _xyz(xyz)
    n = len(xyz)
    r2 = np.float32(tolerance) * np.float32(tolerance)
    fin = finite_rows(xyz)
    A = np.zeros((n, n), bool)
    for s in range(0, n, chunk):
        with np.errstate(all="ignore"):
            A[s:s + chunk] = d2_rows(xyz, slice(s, s + chunk)) <= r2
    A &= fin[:, None] & fin[None, :]
    return A


def components(xyz, tolerance, chunk=512):
    """E2: root [n] uint32, the smallest upload index of each point's component; NONE for a non-finite point.  Min-label
    sweeps over the adjacency with pointer jumping in between, to the fixed point."""
    xyz = _xyz(xyz)
    n = len(xyz)
    fin = finite_rows(xyz)
    A = adjacency(xyz, tolerance, chunk)
    lab = np.arange(n, dtype=np.int64)
    while True:
        new = lab.copy()
        for s in range(0, n, chunk):
            new[s:s + chunk] = np.minimum(new[s:s + chunk], np.where(A[s:s + chunk], lab[None, :], n).min(axis=1, initial=n))
        while True:                                        # a label is a point of the same component: follow it
            nn = new[new]
            if (nn == new).all():
                break
            new = nn
        if (new == lab).all():
            break
        lab = new
    root = lab.astype(np.uint32)
    root[~fin] = NONE
    return root


def clusters(root, min_size=1, max_size=0):
    """E3: dict(cluster [n] uint32, size [K] uint32, cluster_root [K] uint32, n_components, n_kept)."""
    root = np.asarray(root, np.uint32)
    roots, counts = np.unique(root[root != NONE], return_counts=True)
    keep = counts >= max(int(min_size), 1)
    if max_size:
        keep &= counts <= int(max_size)
    kr, kc = roots[keep], counts[keep]
    order = np.lexsort((kr, -kc.astype(np.int64)))         # size descending, root ascending
    kr, kc = kr[order], kc[order]
    rank_of = np.full(len(root) + 1, NONE, np.uint32)
    rank_of[kr] = np.arange(len(kr), dtype=np.uint32)
    label = np.where(root == NONE, NONE, rank_of[np.minimum(root, len(root))]).astype(np.uint32)
    return dict(cluster=label, size=kc.astype(np.uint32), cluster_root=kr.astype(np.uint32), n_components=len(roots), n_kept=len(kr))


def _ord(f):
    """float32 -> uint32, order preserving with -0 below +0 (csrc/scan_index.hpp f2ord)."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


RUN = 64


def run_sum(v):
    """The two-level ordered sum of E4 and E6 over the terms v ([m] or [m, c] float64, in order): runs of 64 terms, each added
    one by one from +0.0, then the runs' sums added one by one from +0.0.  (np.cumsum adds in order; the +0.0 terms that
    fill the last run change nothing.)"""
    v = np.asarray(v, np.float64)
    pad = (-len(v)) % RUN
    v = np.concatenate([v, np.zeros((pad,) + v.shape[1:])])
    part = np.cumsum(v.reshape((-1, RUN) + v.shape[1:]), axis=1)[:, -1]
    return np.cumsum(part, axis=0)[-1]


def figures(xyz, label, n_kept):
    """E4: centroid [K, 3] float64, lo / hi [K, 3] float32."""
    xyz = _xyz(xyz)
    cent, lo, hi = np.zeros((n_kept, 3), np.float64), np.zeros((n_kept, 3), np.float32), np.zeros((n_kept, 3), np.float32)
    for c in range(n_kept):
        p = xyz[label == c]                                # ascending upload index
        cent[c] = run_sum(p.astype(np.float64)) / np.float64(len(p))
        o = _ord(p)
        for a in range(3):
            lo[c, a], hi[c, a] = p[np.argmin(o[:, a]), a], p[np.argmax(o[:, a]), a]
    return cent, lo, hi


def cluster(xyz, tolerance, min_size=1, max_size=0, with_figures=True):
    """E1 - E4: dict(root, cluster, size, cluster_root, n_components, n_kept, centroid, lo, hi)."""
    xyz = _xyz(xyz)
    out = dict(root=components(xyz, tolerance))
    out.update(clusters(out["root"], min_size, max_size))
    if with_figures:
        out["centroid"], out["lo"], out["hi"] = figures(xyz, out["cluster"], out["n_kept"])
    return out


# ---- E5 - E7 ---------------------------------------------------------------------------------------------------------------
def range_keep(xyz, min_range=0.0, max_range=0.0):
    xyz = _xyz(xyz)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        r2 = (x * x + y * y) + z * z
        keep = finite_rows(xyz)
        if max_range > 0:
            keep &= ~(r2 > np.float32(max_range) * np.float32(max_range))
        if min_range > 0:
            keep &= ~(r2 < np.float32(min_range) * np.float32(min_range))
    return keep


def ror_keep(xyz, radius, min_neighbors):
    """E5."""
    xyz = _xyz(xyz)
    count = R.radius_lists(xyz, radius, 1)[2].astype(np.int64)
    return finite_rows(xyz) & (count - 1 >= int(min_neighbors))


def knn_lists(xyz, k, chunk=512):
    """The k-NN lists E6 reads: idx [n, k] uint32, d2 [n, k] float32, self included, ascending (d2, index); only finite
    distances enter, the rest of a row is NONE / FLT_MAX (a non-finite point's whole row)."""
    xyz = _xyz(xyz)
    n = len(xyz)
    idx, d2 = np.full((n, k), NONE, np.uint32), np.full((n, k), FLT_MAX, np.float32)
    for s in range(0, n, chunk):
        d = d2_rows(xyz, slice(s, s + chunk))
        for r in range(len(d)):
            cols = np.flatnonzero(np.isfinite(d[r]))
            cols = cols[np.lexsort((cols, d[r, cols]))][:k]
            idx[s + r, :len(cols)], d2[s + r, :len(cols)] = cols, d[r, cols]
    return idx, d2


def sor_stats(xyz, mean_k):
    """E6: (m [n] float64 with 0 for a non-finite point, mu, sigma, finite [n] bool).  ValueError below mean_k + 1 finite points."""
    xyz = _xyz(xyz)
    n, fin = len(xyz), finite_rows(xyz)
    if not 1 <= mean_k <= 15:
        raise ValueError("mean_k outside [1, 15]")
    if int(fin.sum()) < mean_k + 1:
        raise ValueError("fewer than mean_k + 1 finite points")
    idx, d2 = knn_lists(xyz, mean_k + 1)
    m = np.zeros(n, np.float64)
    for i in np.flatnonzero(fin):
        e = np.flatnonzero(idx[i] != i)[:mean_k]           # the list without i itself, its first mean_k entries
        m[i] = np.cumsum(np.sqrt(d2[i, e].astype(np.float64)))[-1] / np.float64(mean_k)
    N = np.float64(fin.sum())
    mu = run_sum(m) / N                                    # the runs are cut over ALL upload indices: a non-finite point is a +0.0
    dev = np.where(fin, m - mu, 0.0)
    sigma = np.sqrt(run_sum(dev * dev) / N)
    return m, mu, sigma, fin


def sor_keep(xyz, mean_k, std_mul):
    m, mu, sigma, fin = sor_stats(xyz, mean_k)
    return fin & (m <= mu + np.float64(np.float32(std_mul)) * sigma)


def cluster_keep(xyz, tolerance, min_size=1, max_size=0):
    return cluster(xyz, tolerance, min_size, max_size, with_figures=False)["cluster"] != NONE


STAGES = ("range", "ror", "sor", "cluster")


def stage_keep(xyz, stage, p):
    """The survivors (bool [n]) of one stage of the parameter dict p (keys as gloc_scan_filter_params, cluster_* for the
    cluster block), or None where its switch is zero."""
    if stage == "range":
        return range_keep(xyz, p.get("min_range", 0.0), p.get("max_range", 0.0)) if p.get("min_range", 0) > 0 or p.get("max_range", 0) > 0 else None
    if stage == "ror":
        return ror_keep(xyz, p["ror_radius"], p.get("ror_min_neighbors", 0)) if p.get("ror_radius", 0) > 0 else None
    if stage == "sor":
        return sor_keep(xyz, p["sor_mean_k"], p.get("sor_std_mul", 1.0)) if p.get("sor_mean_k", 0) > 0 else None
    return (cluster_keep(xyz, p["cluster_tolerance"], p.get("cluster_min_size", 1), p.get("cluster_max_size", 0))
            if p.get("cluster_tolerance", 0) > 0 else None)


def filtered(xyz, p):
    """E7: (index [m] int64 into xyz of the survivors of the whole chain, in upload order; info dict).  ValueError where a
    stage leaves nothing (the info so far in its args[1])."""
    xyz = _xyz(xyz)
    index = np.arange(len(xyz))
    info = dict(points_in=len(xyz), after_range=len(xyz), after_ror=len(xyz), after_sor=len(xyz), after_cluster=len(xyz))
    for s, stage in enumerate(STAGES):
        keep = stage_keep(xyz[index], stage, p) if len(index) else np.zeros(0, bool)
        if keep is not None:
            index = index[keep]
        for later in STAGES[s:]:
            info["after_" + later] = len(index)
        if len(index) == 0:
            raise ValueError("nothing survives the " + stage + " stage", info)
    return index, info
