"""numpy restatement of the correspondence-graph global registration (include/gloc3d.h: gloc_fpfh_graph_params, G1 - G4) --
the contract of gloc_reg_pair_graph / gloc_reg_fpfh_graph_batch_ids, as tests/fpfh_ref.py is F1 - F4's.  The match list is
fpfh_ref's (features, match); the Kabsch solve and the inlier count are the CPU checker's (oracle/), handed in; the refit is
fpfh_ref.ransac's statement of it, written out again here because that function does not expose it.

Everything up to the Kabsch fits is integer arithmetic on the bit matrix C, which one comparison per entry decides:
|a - b| < compat_thresh in float64.  An entry is flagged EDGE when ||a - b| - compat_thresh| < EDGE_EPS: the differences,
products, sums and square roots behind a and b are each correctly rounded, a few units of 1e-13 in all for lengths below
a kilometre, and 1e-9 is three orders above that: for a list without flagged entries no correct evaluation decides an
entry the other way."""
import numpy as np

NONE = 0xFFFFFFFF
EDGE_EPS = 1e-9
DEFAULTS = dict(normal_k=10, feature_k=16, mutual=1, n_seeds=64, compat_thresh=0.6, inlier_thresh=0.6, min_inlier_ratio=0.0,
                theta_num=1, theta_den=2)


ROW_BLOCK = 256          # G1 and G2 are evaluated this many rows at a time: the peak stays at a few [ROW_BLOCK, M] arrays
KEEP_MATRICES = 1025     # graph() hands C and S back for lists up to this long (tests/pairgraph_cases.py caches what it hands back)


def _lengths(X, rows=slice(None)):
    """The lengths |X_i - X_j| of rows i against every j: each entry is a function of its two points alone, so the row
    blocks below are the whole matrix bit for bit."""
    d = X[rows, None, :] - X[None, :, :]
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def compat(P, Q, compat_thresh=0.6):
    """G1: (C [M, M] bool, edge: the number of (i, j), i != j, both pairs finite, flagged EDGE)."""
    P, Q = np.asarray(P, np.float32).reshape(-1, 3), np.asarray(Q, np.float32).reshape(-1, 3)
    M = len(P)
    fin = np.isfinite(P).all(1) & np.isfinite(Q).all(1)
    thr = float(np.float32(compat_thresh))
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    C, edge = np.zeros((M, M), bool), 0
    with np.errstate(all="ignore"):
        for r0 in range(0, M, ROW_BLOCK):
            rows = slice(r0, min(r0 + ROW_BLOCK, M))
            both = fin[rows, None] & fin[None, :]
            both[np.arange(rows.stop - r0), np.arange(r0, rows.stop)] = False
            diff = np.abs(_lengths(P64, rows) - _lengths(Q64, rows))
            C[rows] = (diff < thr) & both
            edge += int(((np.abs(diff - thr) < EDGE_EPS) & both).sum())
    return C, edge


def second_rows(C, rows, c=None):
    """G2: rows `rows` (a slice or an index array) of S = C_ij |{k: C_ik and C_jk}|, int64 [len, M]."""
    c = C.astype(np.float64) if c is None else c      # (counts below 2^53: exact, and the product runs in BLAS)
    return np.where(C[rows], np.rint(c[rows] @ c), 0).astype(np.int64)


def second_order(C, keep=True):
    """G2: S [M, M] int64 (None unless keep), score [M] uint64 = the row sums of S, a block of rows at a time."""
    M = len(C)
    c = C.astype(np.float64)
    S, score = (np.zeros((M, M), np.int64) if keep else None), np.zeros(M, np.uint64)
    for r0 in range(0, M, ROW_BLOCK):
        rows = slice(r0, min(r0 + ROW_BLOCK, M))
        blk = second_rows(C, rows, c)
        score[rows] = blk.sum(1).astype(np.uint64)
        if keep:
            S[rows] = blk
    return S, score


def kabsch(p, q, oracle):
    """The fp64 fit of two point lists as the refit forms it: raw moments, centroids, covariance, the checker's solve."""
    cnt = float(len(p))
    pbar, qbar = p.sum(0) / cnt, q.sum(0) / cnt
    Mc = np.ascontiguousarray(p.T @ q - cnt * np.outer(pbar, qbar))
    Rd, td = np.empty(9), np.empty(3)
    oracle.lib().oracle_kabsch_from_cov(Mc.reshape(9), np.ascontiguousarray(pbar), np.ascontiguousarray(qbar), Rd, td)
    return Rd, td


def inlier_mask(P, Q, R, t, thr):
    """F4's residual: float32, un-fused, < thr^2 (a NaN residual is no inlier)."""
    x = ((R[0] * P[:, 0] + R[1] * P[:, 1]) + R[2] * P[:, 2]) + t[0]
    y = ((R[3] * P[:, 0] + R[4] * P[:, 1]) + R[5] * P[:, 2]) + t[1]
    z = ((R[6] * P[:, 0] + R[7] * P[:, 1]) + R[8] * P[:, 2]) + t[2]
    dx, dy, dz = x - Q[:, 0], y - Q[:, 1], z - Q[:, 2]
    return ((dx * dx + dy * dy) + dz * dz) < thr * thr


def graph(P, Q, oracle, n_seeds=64, compat_thresh=0.6, inlier_thresh=0.6, min_inlier_ratio=0.0, theta_num=1, theta_den=2, **_):
    """G1 - G4 on the pair list (P[m], Q[m]): dict(degree [M] uint32, score [M] uint64, seeds [n_seeds] uint32 (NONE beyond
    M), set_sizes [n_seeds], seed_inliers [n_seeds], sets (list of index arrays, None: no hypothesis), T [4, 4] float64,
    inliers, winner_rank (NONE: none), ok, n_pairs, edge, density, C, S (both None for a list longer than KEEP_MATRICES: 8 + 1
    bytes per entry are not worth keeping; compat() and second_order() make them on request), winner_mask)."""
    P, Q = np.ascontiguousarray(P, np.float32).reshape(-1, 3), np.ascontiguousarray(Q, np.float32).reshape(-1, 3)
    M = len(P)
    C, edge = compat(P, Q, compat_thresh)
    keep = M <= KEEP_MATRICES
    S, score = second_order(C, keep)
    order = np.lexsort((np.arange(M), -score.astype(np.int64)))[:n_seeds]       # score descending, position ascending
    seeds = np.full(n_seeds, NONE, np.uint32)
    seeds[:len(order)] = order
    set_sizes, seed_inl = np.zeros(n_seeds, np.uint32), np.zeros(n_seeds, np.uint32)
    sets, hyps = [None] * n_seeds, [None] * n_seeds
    corr = np.arange(M, dtype=np.uint32)
    thr = np.float32(inlier_thresh)
    seed_rows = S[order] if keep else second_rows(C, order)                     # the seeds' rows of S are all G3 reads
    with np.errstate(all="ignore"):
        for r, s in enumerate(order):
            row = seed_rows[r]
            mx = int(row.max(initial=0))
            if mx == 0:
                continue
            member = (int(theta_den) * row >= int(theta_num) * mx) & (row > 0)
            member[s] = True
            idx = np.flatnonzero(member)
            set_sizes[r] = len(idx)
            if len(idx) < 3:
                continue
            sets[r] = idx
            Rd, td = kabsch(P[idx].astype(np.float64), Q[idx].astype(np.float64), oracle)
            R32, t32 = Rd.astype(np.float32), td.astype(np.float32)
            hyps[r] = (R32, t32)
            seed_inl[r] = oracle.lib().oracle_count_inliers(P, Q, corr, M, R32, t32, thr)
    degree = C.sum(1).astype(np.uint32)
    out = dict(degree=degree, score=score, seeds=seeds, set_sizes=set_sizes, seed_inliers=seed_inl, sets=sets,
               T=np.eye(4), inliers=0, winner_rank=NONE, ok=False, n_pairs=M, edge=edge,
               density=float(degree.sum(dtype=np.int64)) / max(M * (M - 1), 1), C=C if keep else None, S=S, winner_mask=np.zeros(M, bool))
    if M < 3 or not seed_inl.any():
        return out
    w = int(np.argmax(seed_inl))                                                # the most inliers, then the smaller rank
    Rf, tf = hyps[w]
    with np.errstate(all="ignore"):
        inl = inlier_mask(P, Q, Rf, tf, thr)
    Rd, td = Rf.astype(np.float64), tf.astype(np.float64)
    if inl.sum() >= 3:
        Rd, td = kabsch(P[inl].astype(np.float64), Q[inl].astype(np.float64), oracle)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rd.reshape(3, 3), td
    best = int(seed_inl[w])
    need = max(3.0, np.ceil(float(np.float32(min_inlier_ratio)) * M))
    out.update(T=T, inliers=best, winner_rank=w, ok=bool(best >= need), winner_mask=inl)
    return out


def register(src, tgt, oracle, src_feat=None, tgt_feat=None, **params):
    """The whole stage on two clouds (float32 [n, 3]): fpfh_ref's features (unless handed in) and matches, then graph()."""
    import fpfh_ref as F
    p = dict(DEFAULTS, **params)
    src, tgt = np.ascontiguousarray(src, np.float32).reshape(-1, 3), np.ascontiguousarray(tgt, np.float32).reshape(-1, 3)
    fs = F.features(src, p["normal_k"], p["feature_k"], oracle)["feat"] if src_feat is None else src_feat
    ft = F.features(tgt, p["normal_k"], p["feature_k"], oracle)["feat"] if tgt_feat is None else tgt_feat
    idx, _ = F.match(fs, ft, bool(p["mutual"]))
    keep = np.flatnonzero(idx != F.NONE)
    res = graph(src[keep], tgt[idx[keep]], oracle, **p)
    res["pairs"] = np.stack([keep.astype(np.uint32), idx[keep]], 1) if len(keep) else np.zeros((0, 2), np.uint32)
    return res
