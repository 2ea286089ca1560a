"""float64 restatement of the FPFH feature-based global registration (include/gloc3d.h: gloc_fpfh_params, F1 - F4) --
the contract of gloc_scan_store_build_fpfh / gloc_reg_fpfh_match / gloc_reg_fpfh_batch_ids, as tests/gicp_ref.py is
generalized ICP's.  numpy only; the RANSAC rules it does not restate again are the CPU checker's (oracle/), handed in.

Inputs are what the device starts from: the cloud (float32), its normals (float32, zero row = none) and its exact k-NN
lists (self included, ascending (d2, index); 0xFFFFFFFF / FLT_MAX where a list is short), both as the checker builds them.

Every sum can be taken in list order ("forward") or reversed: the difference is the restatement's own rounding floor, which
the device tests scale their tolerance by.  A pair is flagged EDGE when one of its three scaled features lies within EDGE_EPS
of a bin boundary (the integers 1 .. 10: at 0 and 11 both sides clamp into the same end bin), or when the two angles that
decide the roles differ by less than EDGE_EPS without being equal: 1e-9 is nine orders above fp64 rounding, so for a pair
that is not flagged no correct evaluation can land in another bin."""
import ctypes as C

import numpy as np

NONE = 0xFFFFFFFF
DIM, NB = 33, 11
EDGE_EPS = 1e-9
DEFAULTS = dict(normal_k=10, feature_k=16, mutual=1, ransac_iters=3000, inlier_thresh=0.6, min_inlier_ratio=0.0,
                ransac_confidence=0.99, seed=1234)


def lists(xyz, k, oracle):
    """(idx [n, k] uint32, d2 [n, k] float32) of the cloud: the checker's exact k-NN, the lists the normals are built from."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if len(xyz) == 0:
        return np.zeros((0, k), np.uint32), np.zeros((0, k), np.float32)
    return oracle.ground_knn(xyz, k)


def normals(xyz, k, oracle):
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if len(xyz) == 0:
        return np.zeros((0, 3), np.float32)
    return oracle.ground_normals(xyz, oracle.ground_knn(xyz, k)[0])[0]


def _usable(xyz, nrm, idx, d2):
    n = len(xyz)
    i = np.arange(n)[:, None]
    inside = idx < n
    j = np.where(inside, idx, 0).astype(np.int64)
    fin = np.isfinite(xyz).all(1)
    has = (nrm != 0).any(1)
    with np.errstate(invalid="ignore"):
        ok = inside & (j != i) & (d2 > 0) & np.isfinite(d2) & fin[:, None] & fin[j] & has[:, None] & has[j]
    return ok, j


def pair_features(xyz, nrm, idx, d2):
    """Per list entry: counted [n, k] bool, bins [n, k, 3] (0 .. 10), edge [n, k] bool."""
    xyz, nrm = np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(nrm, np.float32).reshape(-1, 3)
    ok, j = _usable(xyz, nrm, idx, d2)
    P, N = xyz.astype(np.float64), nrm.astype(np.float64)
    with np.errstate(all="ignore"):
        dp = np.where(ok[..., None], P[j] - P[:, None, :], 0.0)
        ni, nj = np.broadcast_to(N[:, None, :], dp.shape), N[j]
        f4 = np.sqrt((dp[..., 0] * dp[..., 0] + dp[..., 1] * dp[..., 1]) + dp[..., 2] * dp[..., 2])
        ok = ok & (f4 > 0)
        dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]  # noqa: E731
        a1, a2 = dot(ni, dp) / f4, dot(nj, dp) / f4
        A1, A2 = np.arccos(np.minimum(np.abs(a1), 1.0)), np.arccos(np.minimum(np.abs(a2), 1.0))
        swap = A1 > A2
        n1, n2 = np.where(swap[..., None], nj, ni), np.where(swap[..., None], ni, nj)
        f3 = np.where(swap, -a2, a1)
        dp = np.where(swap[..., None], -dp, dp)
        cross = lambda a, b: np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],  # noqa: E731
                                       a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
        v = cross(dp, n1)
        vl = np.sqrt(dot(v, v))
        ok = ok & (vl > 0)
        v = v / vl[..., None]
        w = cross(n1, v)
        f2 = dot(v, n2)
        f1 = np.arctan2(dot(w, n2), dot(n1, n2))
        s = np.stack([11.0 * (f1 + np.pi) / (2.0 * np.pi), 11.0 * (f2 + 1.0) / 2.0, 11.0 * (f3 + 1.0) / 2.0], -1)
        fl = np.floor(s)
        bins = np.where(fl < 0, 0, np.where(fl > 10, 10, fl))
        bins = np.where(np.isnan(bins), 0, bins).astype(np.int64)
        r = np.rint(s)
        near = (np.abs(s - r) < EDGE_EPS) & (r >= 1) & (r <= 10)
        edge = near.any(-1) | ((np.abs(A1 - A2) < EDGE_EPS) & (A1 != A2))
    return ok, np.where(ok[..., None], bins, 0), edge & ok


def spfh(xyz, nrm, idx, d2):
    """counts [n, 33] int64, used [n] int64, edge [n] bool: the point has an edge pair of its own."""
    ok, bins, edge = pair_features(xyz, nrm, idx, d2)
    n = len(ok)
    counts = np.zeros((n, DIM), np.int64)
    rows = np.repeat(np.arange(n), ok.shape[1]).reshape(ok.shape)
    for f in range(3):
        np.add.at(counts, (rows[ok], f * NB + bins[..., f][ok]), 1)
    return counts, ok.sum(1).astype(np.int64), edge.any(1)


def edge_flags(edge_own, idx):
    """A point is edge-flagged if it or any entry of its list has an edge pair."""
    n = len(edge_own)
    inside = idx < n
    j = np.where(inside, idx, 0).astype(np.int64)
    return edge_own | (edge_own[j] & inside).any(1) if n else edge_own


def fpfh(counts, used, idx, d2, order="forward"):
    """The features [n, 33] float64 (before the store's rounding to float32); order: the direction of every sum."""
    n, k = idx.shape
    i = np.arange(n)[:, None]
    inside = idx < n
    j = np.where(inside, idx, 0).astype(np.int64)
    with np.errstate(all="ignore"):
        ok = inside & (j != i) & (d2 > 0) & np.isfinite(d2) & (used[j] > 0) & (used[:, None] > 0)
        wgt = np.where(ok, 1.0 / d2.astype(np.float64), 0.0)
        acc = np.zeros((n, DIM), np.float64)
        for s in (range(k) if order == "forward" else range(k - 1, -1, -1)):
            term = ((counts[j[:, s]].astype(np.float64) * 100.0) / np.maximum(used[j[:, s]], 1)[:, None].astype(np.float64)) * wgt[:, s, None]
            acc = acc + np.where(ok[:, s, None], term, 0.0)
        out = np.zeros((n, DIM), np.float64)
        for h in range(3):
            tot = np.zeros(n, np.float64)
            for b in (range(NB) if order == "forward" else range(NB - 1, -1, -1)):
                tot = tot + acc[:, h * NB + b]
            sc = np.where(ok.any(1) & (tot > 0), 100.0 / np.where(tot > 0, tot, 1.0), 0.0)
            out[:, h * NB:(h + 1) * NB] = acc[:, h * NB:(h + 1) * NB] * sc[:, None]
    return out


def features(xyz, normal_k, feature_k, oracle, order="forward", nrm=None):
    """dict(feat [n, 33] float32 as stored, feat64, counts, used, flagged [n] bool, nrm, idx, d2) of a cloud."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    nrm = normals(xyz, normal_k, oracle) if nrm is None else np.asarray(nrm, np.float32)
    idx, d2 = lists(xyz, feature_k, oracle)
    counts, used, edge_own = spfh(xyz, nrm, idx, d2)
    f64 = fpfh(counts, used, idx, d2, order)
    return dict(feat=f64.astype(np.float32), feat64=f64, counts=counts, used=used, edge_own=edge_own, flagged=edge_flags(edge_own, idx),
                nrm=nrm, idx=idx, d2=d2)


def distances(a, b):
    """[na, nb] float32: the defined sum, every operation rounded to float32 on its own."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((len(a), len(b)), np.float32)
    for c in range(DIM):
        t = a[:, c, None] - b[None, :, c]
        acc = acc + t * t
    return acc


def nearest(a, b, chunk=512):
    """For every row of a with a feature the row of b with a feature at the smallest distance, smaller index among equals:
    (idx uint32, NONE where there is none; d2 float32, +inf there)."""
    a, b = np.asarray(a, np.float32).reshape(-1, DIM), np.asarray(b, np.float32).reshape(-1, DIM)
    idx, d2 = np.full(len(a), NONE, np.uint32), np.full(len(a), np.inf, np.float32)
    va, vb = (a != 0).any(1), np.flatnonzero((b != 0).any(1))
    if not va.any() or len(vb) == 0:
        return idx, d2
    rows = np.flatnonzero(va)
    for s in range(0, len(rows), chunk):
        r = rows[s:s + chunk]
        d = distances(a[r], b[vb])
        m = np.argmin(d, axis=1)                          # (first minimum: the smallest index among equals)
        idx[r], d2[r] = vb[m].astype(np.uint32), d[np.arange(len(r)), m]
    return idx, d2


def match(a, b, mutual=True):
    """The kept matches, as gloc_reg_fpfh_match reports them."""
    idx, d2 = nearest(a, b)
    if mutual:
        back, _ = nearest(b, a)
        has = idx != NONE
        keep = has.copy()
        keep[has] = back[idx[has]] == np.flatnonzero(has)      # (no target rows: nothing has a match, nothing is looked up)
        idx, d2 = np.where(keep, idx, NONE).astype(np.uint32), np.where(keep, d2, np.inf).astype(np.float32)
    return idx, d2


def _needed_iters(oracle, inl, n, conf, cap):
    f = oracle.lib().oracle_ransac_needed_iters
    f.restype, f.argtypes = C.c_uint32, [C.c_uint32, C.c_uint32, C.c_float, C.c_uint32]
    return f(int(inl), int(n), float(conf), int(cap))


def ransac(P, Q, oracle, stream_id=0, ransac_iters=3000, inlier_thresh=0.6, min_inlier_ratio=0.0, ransac_confidence=0.99, seed=1234,
           **_):
    """F4 on the pair list (P[m], Q[m]): dict(T [4, 4] float64, inliers, ok, best_hyp, iters).  Hypotheses, inlier counts and
    the adaptive stop are the checker's statements of the existing stage; the sequential rule and the refit are here."""
    P, Q = np.ascontiguousarray(P, np.float32).reshape(-1, 3), np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    M = len(P)
    out = dict(T=np.eye(4), inliers=0, ok=False, best_hyp=NONE, iters=0, n_pairs=M)
    if M < 3:
        return out
    L = oracle.lib()
    corr = np.arange(M, dtype=np.uint32)
    adaptive = 0.0 < ransac_confidence < 1.0
    niters, best, best_h, best_Rt = int(ransac_iters), 0, NONE, None
    R, t = np.empty(9, np.float32), np.empty(3, np.float32)
    h = 0
    while h < niters:
        if L.oracle_ransac_hypothesis(P, Q, corr, M, int(seed), int(stream_id), h, R, t):
            inl = L.oracle_count_inliers(P, Q, corr, M, R, t, np.float32(inlier_thresh))
            if inl > best:
                best, best_h, best_Rt = inl, h, (R.copy(), t.copy())
                if adaptive:
                    niters = min(niters, _needed_iters(oracle, best, M, ransac_confidence, niters))
        h += 1
    out["iters"] = niters
    if best_h == NONE:
        return out
    # the refit: Kabsch on the winner's inliers (residuals in float32, un-fused, as the stage scores them)
    Rf, tf = best_Rt
    x = ((Rf[0] * P[:, 0] + Rf[1] * P[:, 1]) + Rf[2] * P[:, 2]) + tf[0]
    y = ((Rf[3] * P[:, 0] + Rf[4] * P[:, 1]) + Rf[5] * P[:, 2]) + tf[1]
    z = ((Rf[6] * P[:, 0] + Rf[7] * P[:, 1]) + Rf[8] * P[:, 2]) + tf[2]
    dx, dy, dz = x - Q[:, 0], y - Q[:, 1], z - Q[:, 2]
    thr = np.float32(inlier_thresh)
    inl = ((dx * dx + dy * dy) + dz * dz) < thr * thr
    Rd, td = Rf.astype(np.float64).copy(), tf.astype(np.float64).copy()
    if inl.sum() >= 3:
        p, q = P[inl].astype(np.float64), Q[inl].astype(np.float64)
        cnt = float(len(p))
        pbar, qbar = p.sum(0) / cnt, q.sum(0) / cnt
        Mc = np.ascontiguousarray(p.T @ q - cnt * np.outer(pbar, qbar))
        Rd, td = np.empty(9), np.empty(3)
        L.oracle_kabsch_from_cov(Mc.reshape(9), np.ascontiguousarray(pbar), np.ascontiguousarray(qbar), Rd, td)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rd.reshape(3, 3), td
    need = max(3.0, np.ceil(float(np.float32(min_inlier_ratio)) * M))
    out.update(T=T, inliers=int(best), ok=bool(best >= need), best_hyp=int(best_h))
    return out


def register(src, tgt, oracle, stream_id=0, src_feat=None, tgt_feat=None, **params):
    """The whole stage on two clouds (float32 [n, 3]): features (unless handed in), matches, pairs, RANSAC."""
    p = dict(DEFAULTS, **params)
    src, tgt = np.ascontiguousarray(src, np.float32).reshape(-1, 3), np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
    fs = features(src, p["normal_k"], p["feature_k"], oracle)["feat"] if src_feat is None else src_feat
    ft = features(tgt, p["normal_k"], p["feature_k"], oracle)["feat"] if tgt_feat is None else tgt_feat
    idx, _ = match(fs, ft, bool(p["mutual"]))
    keep = np.flatnonzero(idx != NONE)
    res = ransac(src[keep], tgt[idx[keep]], oracle, stream_id=stream_id, **p)
    res["pairs"] = np.stack([keep.astype(np.uint32), idx[keep]], 1) if len(keep) else np.zeros((0, 2), np.uint32)
    return res
