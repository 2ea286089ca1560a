"""numpy restatement of the Fast Global Registration on a match list (include/gloc3d.h: gloc_fgr_params, R1 - R4) -- the
contract of gloc_reg_fgr_pairs / gloc_reg_fpfh_fgr_batch_ids, as tests/pairgraph_ref.py is G1 - G4's.  The match list is
fpfh_ref's (features, match); the keyed 3-point sample is the CPU checker's (oracle_ransac_sample), handed in; everything
else is float64 numpy written out here.

The tuple test decides on strict inequalities between fp64 lengths.  An edge with finite, non-zero lengths is flagged EDGE
when |s lp - lq| <= 1e-9 lq or |s lq - lp| <= 1e-9 lp: the differences, products, sums and square roots behind a length are
each correctly rounded, a few units of 1e-16 relative in all, and 1e-9 is six orders above that: for a list without flagged
edges no correct evaluation decides a tuple the other way."""
import numpy as np

import pairgraph_ref as G

EDGE_EPS = 1e-9
DEFAULTS = dict(normal_k=10, feature_k=16, mutual=1, tuple_tries=10000, max_tuples=1000, tuple_scale=0.9, max_iters=64, anneal_every=4,
                anneal_div=1.4, max_corr_dist=0.6, inlier_thresh=0.6, min_inlier_ratio=0.0, seed=1234)
NSYS = 27                 # H's upper triangle (21, row-major) and g (6)
_IU = np.triu_indices(6)


def samples(M, oracle, seed, stream_id, tries):
    """F4's samples h = 0 .. tries - 1 over [0, M): uint32 [tries, 3]."""
    out = np.zeros((tries, 3), np.uint32)
    s = np.zeros(3, np.uint32)
    fn = oracle.lib().oracle_ransac_sample
    for h in range(tries):
        fn(int(seed), int(stream_id), h, int(M), s)
        out[h] = s
    return out


def _len(X, a, b):
    d = X[a] - X[b]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def tuple_test(P, Q, oracle, seed=1234, stream_id=0, tuple_tries=10000, max_tuples=1000, tuple_scale=0.9, **_):
    """R1: dict(mult [M] uint32, n_tuples, edge: the flagged edges among the samples looked at, kept [n_tuples, 3])."""
    P, Q = np.ascontiguousarray(P, np.float32).reshape(-1, 3), np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    M = len(P)
    if tuple_tries == 0:
        fin = np.isfinite(P).all(1) & np.isfinite(Q).all(1)
        return dict(mult=fin.astype(np.uint32), n_tuples=0, edge=0, kept=np.zeros((0, 3), np.uint32))
    mult = np.zeros(M, np.uint32)
    if M < 3:
        return dict(mult=mult, n_tuples=0, edge=0, kept=np.zeros((0, 3), np.uint32))
    S = samples(M, oracle, seed, stream_id, tuple_tries).astype(np.int64)
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    s = float(np.float32(tuple_scale))
    distinct = (S[:, 0] != S[:, 1]) & (S[:, 0] != S[:, 2]) & (S[:, 1] != S[:, 2])
    ok, edge = distinct.copy(), 0
    with np.errstate(all="ignore"):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            lp, lq = _len(P64, S[:, a], S[:, b]), _len(Q64, S[:, a], S[:, b])
            ok &= (s * lp < lq) & (s * lq < lp)
            live = distinct & np.isfinite(lp) & np.isfinite(lq) & (lp > 0) & (lq > 0)
            edge += int((live & ((np.abs(s * lp - lq) <= EDGE_EPS * lq) | (np.abs(s * lq - lp) <= EDGE_EPS * lp))).sum())
    kept = S[np.flatnonzero(ok)[:max_tuples]]
    np.add.at(mult, kept.reshape(-1), 1)
    return dict(mult=mult, n_tuples=len(kept), edge=edge, kept=kept.astype(np.uint32))


def weight(s2, mu):
    """The Geman-McClure weight of the robust block: t = s2 / mu, 1 / ((1 + t)(1 + t))."""
    t = s2 / mu
    return 1.0 / ((1.0 + t) * (1.0 + t))


def system(P64, Q64, mult, T, mu):
    """R3's normal equations at pose T (12: R row-major, t) and scale mu: [27] = H's upper triangle, g."""
    R, t = T[:9].reshape(3, 3), T[9:]
    X = P64 @ R.T + t
    r = X - Q64
    s2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    w = mult * weight(s2, mu)
    n = len(X)
    J = np.zeros((n, 3, 6))
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    J[:, 0, 1], J[:, 0, 2] = z, -y          # -[x]x
    J[:, 1, 0], J[:, 1, 2] = -z, x
    J[:, 2, 0], J[:, 2, 1] = y, -x
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    H = np.einsum("n,nka,nkb->ab", w, J, J)
    g = np.einsum("n,nka,nk->a", w, J, r)
    return np.concatenate([H[_IU], g])


def solve_update(sys27, T):
    """The Gauss-Newton refinements' solve: Cholesky row by row with the pivot rule, xi = -H^-1 g, Rodrigues, exp(xi) T.
    (None: degenerate, d / dmax of the smallest pivot looked at)."""
    L = np.zeros((6, 6))
    L[_IU] = sys27[:21]
    L = L + np.triu(L, 1).T
    g = sys27[21:]
    dmax = max(0.0, float(L.diagonal().max()))
    margin = np.inf
    for j in range(6):
        d = L[j, j] - float((L[j, :j] * L[j, :j]).sum())
        margin = min(margin, d / dmax) if dmax > 0.0 else 0.0
        if not d > 1e-12 * dmax:
            return None, margin
        dj = np.sqrt(d)
        L[j, j] = dj
        for i in range(j + 1, 6):
            L[i, j] = (L[i, j] - float((L[i, :j] * L[j, :j]).sum())) / dj
    y, xi = np.zeros(6), np.zeros(6)
    for i in range(6):
        y[i] = (-g[i] - float((L[i, :i] * y[:i]).sum())) / L[i, i]
    for i in range(5, -1, -1):
        xi[i] = (y[i] - float((L[i + 1:, i] * xi[i + 1:]).sum())) / L[i, i]
    wx, wy, wz = xi[:3]
    th2 = (wx * wx + wy * wy) + wz * wz
    th = np.sqrt(th2)
    A, B = 1.0, 0.5
    if th > 0.0:
        A = np.sin(th) / th
        sh = np.sin(0.5 * th)
        B = 2.0 * (sh * sh) / th2
    K = np.array([[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]])
    Rk = np.eye(3) + A * K + B * (K @ K)
    R, t = T[:9].reshape(3, 3), T[9:]
    return np.concatenate([(Rk @ R).reshape(9), Rk @ t + xi[3:]]), margin


def fgr(P, Q, oracle, stream_id=0, **params):
    """R1 - R4 on the pair list (P[m], Q[m]): dict(mult, n_tuples, edge, d2, system [27], T [4, 4] float64 (the fp32 pose),
    T64 [4, 4] (before rounding), inliers, status, ok, n_pairs, updates, near: the pairs whose fp64 residual length lies
    within 1e-4 + 1e-4 |x| of inlier_thresh, pivot_min: the smallest Cholesky pivot of the updates that ran, over the system's
    largest diagonal entry, pivot_fail: that of a degenerate update, else None, need: the inliers ok asks for)."""
    p = dict(DEFAULTS, **params)
    P, Q = np.ascontiguousarray(P, np.float32).reshape(-1, 3), np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    M = len(P)
    out = dict(mult=np.zeros(M, np.uint32), n_tuples=0, edge=0, d2=0.0, system=np.zeros(NSYS), T=np.eye(4), T64=np.eye(4), inliers=0,
               status=2, ok=False, n_pairs=M, updates=0, near=0, pivot_min=np.inf, pivot_fail=None,
               need=max(3.0, float(np.ceil(float(np.float32(p["min_inlier_ratio"])) * M))))
    if M < 3:                       # (nothing is looked at: the multiplicities stay 0 whatever tuple_tries is)
        return out
    tt = tuple_test(P, Q, oracle, stream_id=stream_id, **p)
    out.update(mult=tt["mult"], n_tuples=tt["n_tuples"], edge=tt["edge"])
    A = np.flatnonzero(tt["mult"] > 0)
    P64, Q64, mult = P[A].astype(np.float64), Q[A].astype(np.float64), tt["mult"][A].astype(np.float64)
    delta = float(np.float32(p["max_corr_dist"]))
    div = float(np.float32(p["anneal_div"]))
    if len(A):
        cP, cQ = (mult[:, None] * P64).sum(0) / mult.sum(), (mult[:, None] * Q64).sum(0) / mult.sum()
        a, b = P64 - cP, Q64 - cQ
        a2 = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
        b2 = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
        out["d2"] = float(max(a2.max(), b2.max()))
    mu = max(out["d2"], delta * delta)
    T = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    status = 0
    for k in range(int(p["max_iters"])):
        if k > 0 and k % int(p["anneal_every"]) == 0:
            mu = max(mu / div, delta * delta)
        out["system"] = system(P64, Q64, mult, T, mu)
        Tn, margin = solve_update(out["system"], T) if len(A) >= 3 else (None, 0.0)
        if Tn is None:
            status = 2
            out["pivot_fail"] = margin
            break
        T = Tn
        out["pivot_min"] = min(out["pivot_min"], margin)
        out["updates"] = k + 1
    out["status"] = status
    if out["updates"] == 0:
        return out
    T64 = np.eye(4)
    T64[:3, :3], T64[:3, 3] = T[:9].reshape(3, 3), T[9:]
    R32, t32 = T[:9].astype(np.float32), T[9:].astype(np.float32)
    thr = np.float32(p["inlier_thresh"])
    with np.errstate(all="ignore"):
        inl = int(G.inlier_mask(P, Q, R32, t32, thr).sum())
        X = P.astype(np.float64) @ T64[:3, :3].T + T64[:3, 3]
        res = np.sqrt(((X - Q.astype(np.float64)) ** 2).sum(1))
        near = int((np.isfinite(res) & (np.abs(res - float(thr)) <= 1e-4 + 1e-4 * np.abs(X).max(1))).sum())   # (an infinite residual is no inlier to anyone)
    T32 = np.eye(4)
    T32[:3, :3], T32[:3, 3] = R32.reshape(3, 3).astype(np.float64), t32.astype(np.float64)
    out.update(T=T32, T64=T64, inliers=inl, ok=bool(status == 0 and inl >= out["need"]), near=near)
    return out


def register(src, tgt, oracle, src_feat=None, tgt_feat=None, stream_id=0, **params):
    """The whole stage on two clouds (float32 [n, 3]): fpfh_ref's features (unless handed in) and matches, then fgr()."""
    import fpfh_ref as F
    p = dict(DEFAULTS, **params)
    src, tgt = np.ascontiguousarray(src, np.float32).reshape(-1, 3), np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
    fs = F.features(src, p["normal_k"], p["feature_k"], oracle)["feat"] if src_feat is None else src_feat
    ft = F.features(tgt, p["normal_k"], p["feature_k"], oracle)["feat"] if tgt_feat is None else tgt_feat
    idx, _ = F.match(fs, ft, bool(p["mutual"]))
    keep = np.flatnonzero(idx != F.NONE)
    res = fgr(src[keep], tgt[idx[keep]], oracle, stream_id=stream_id, **p)
    res["pairs"] = np.stack([keep.astype(np.uint32), idx[keep]], 1) if len(keep) else np.zeros((0, 2), np.uint32)
    return res
