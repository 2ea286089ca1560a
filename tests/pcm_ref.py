"""The float64 contract of the pose graph's closure selection (include/gloc3d.h, gloc_pgo_consistency, C1 - C6): pairwise
consistency of loop closures and the greedy clique over them, in numpy.  Every floating-point function takes `dt`
(numpy.float64 by default) like pgo_ref.py: the GPU tests evaluate a case in float64 and in numpy.longdouble and take the
difference as the formula's rounding scale.  The pair statistic is evaluated for all pairs of a case at once (arrays with a
leading pair axis); pair_s2_scalar states the same thing for one pair through pgo_ref.residual, and the CPU tests hold the
two together.

Conventions are pgo_ref.py's: node k has pose (R_k, t_k), node -> map; closure a = (i, j, Z, Omega), Z ~ T_j^-1 T_i;
perturbations are left ones, xi = (w, v), rotation first.
"""
import numpy as np

import pgo_ref as R

NONE = 0xFFFFFFFF
CHI2_99_6 = 16.8119                      # the 99 % quantile of chi-squared with 6 degrees of freedom
DEFAULTS = dict(chi2=CHI2_99_6, drift_rot=0.0, drift_trans=0.0, n_seeds=64, min_clique=2)


# ---- C1: the per-closure setup ---------------------------------------------------------------------------------------------
def chol6(H, dt=np.float64):
    """pgo_kernels.hpp's chol6 on a batch [..., 6, 6] (read from the LOWER triangle, which the callers fill from the upper
    one): (the lower factors, ok [...]).  A failed pivot leaves that matrix's factor meaningless."""
    L = np.array(H, dt)
    dmax = np.maximum(dt(0), np.max(np.diagonal(L, axis1=-2, axis2=-1), axis=-1))
    ok = np.ones(L.shape[:-2], bool)
    for j in range(6):
        d = L[..., j, j].copy()
        for k in range(j):
            d = d - L[..., j, k] * L[..., j, k]
        ok &= d > dt(1e-12) * dmax
        dj = np.sqrt(np.where(ok, d, dt(1)))
        L[..., j, j] = dj
        for i in range(j + 1, 6):
            s = L[..., i, j].copy()
            for k in range(j):
                s = s - L[..., i, k] * L[..., j, k]
            L[..., i, j] = s / dj
    return L, ok


def forward(L, r):
    """y = L^-1 r on a batch."""
    y = np.zeros_like(r)
    for i in range(6):
        s = r[..., i].copy()
        for k in range(i):
            s = s - L[..., i, k] * y[..., k]
        y[..., i] = s / L[..., i, i]
    return y


def backward(L, y):
    """z = L^-T y on a batch."""
    z = np.zeros_like(y)
    for i in range(5, -1, -1):
        s = y[..., i].copy()
        for k in range(i + 1, 6):
            s = s - L[..., k, i] * z[..., k]
        z[..., i] = s / L[..., i, i]
    return z


def sym_from_upper(M):
    up = np.triu(M)
    return up + np.swapaxes(np.triu(M, 1), -1, -2)


def inv_rigid(T):
    """(R^T, -(R^T t)) on a batch [..., 4, 4]."""
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:4])[..., 0]
    out[..., 3, 3] = 1
    return out


class Setup:
    pass


def setup(poses, src, tgt, Z, info, path=None, dt=np.float64):
    """C1.  Ti, Tj [L, 4, 4] (translations relative to node 0's), Z [L, 4, 4], B = (T_j Z) T_i^-1, Sigma [L, 6, 6] (column b
    of Omega^-1 by the Cholesky solve of the unit vector e_b, its rows a <= b kept and mirrored), status [L] (1: Omega
    failed the pivot rule), pi, pj [L]."""
    P = np.array(poses, dt)
    P[:, :3, 3] -= np.asarray(poses[0][:3, 3], dt)
    src, tgt = np.asarray(src, np.int64), np.asarray(tgt, np.int64)
    S = Setup()
    S.L = len(src)
    S.Ti, S.Tj, S.Z = P[src], P[tgt], np.asarray(Z).astype(dt)
    S.B = (S.Tj @ S.Z) @ inv_rigid(S.Ti)
    Lf, ok = chol6(sym_from_upper(np.asarray(info).astype(dt)), dt)
    S.status = (~ok).astype(np.uint8)
    cols = np.zeros((S.L, 6, 6), dt)
    for b in range(6):
        e = np.zeros((S.L, 6), dt)
        e[:, b] = 1
        cols[:, :, b] = backward(Lf, forward(Lf, e))
    S.Sigma = sym_from_upper(cols)
    S.Sigma[~ok] = 0
    pth = np.zeros(len(P), dt) if path is None else np.asarray(path).astype(dt)
    S.pi, S.pj = pth[src], pth[tgt]
    return S


# ---- C2: the pair statistic ---------------------------------------------------------------------------------------------------
def log_so3(Rm, dt=np.float64):
    """pgo_ref.log_so3 on a batch [..., 3, 3]."""
    v = np.stack([Rm[..., 2, 1] - Rm[..., 1, 2], Rm[..., 0, 2] - Rm[..., 2, 0], Rm[..., 1, 0] - Rm[..., 0, 1]], -1) * dt(0.5)
    s = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    c = (((Rm[..., 0, 0] + Rm[..., 1, 1]) + Rm[..., 2, 2]) - dt(1)) * dt(0.5)
    small = s < dt(1e-8)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(small, dt(1) + s * s / dt(6), np.arctan2(s, c) / np.where(small, dt(1), s))
    return v * f[..., None]


def residual(Ti, Tj, Z, dt=np.float64):
    """pgo_ref.residual (G2) on a batch."""
    Ri, ti, Rj, tj, Rz, tz = Ti[..., :3, :3], Ti[..., :3, 3], Tj[..., :3, :3], Tj[..., :3, 3], Z[..., :3, :3], Z[..., :3, 3]
    RjT = np.swapaxes(Rj, -1, -2)
    RE = (RjT @ Ri) @ np.swapaxes(Rz, -1, -2)
    tE = (RjT @ (ti - tj)[..., None])[..., 0] - (RE @ tz[..., None])[..., 0]
    return np.concatenate([log_so3(RE, dt), tE], -1)


def skew(t, dt=np.float64):
    K = np.zeros(t.shape[:-1] + (3, 3), dt)
    K[..., 0, 1], K[..., 0, 2] = -t[..., 2], t[..., 1]
    K[..., 1, 0], K[..., 1, 2] = t[..., 2], -t[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -t[..., 1], t[..., 0]
    return K


def pair_s2(S, a, b, drift_rot=0.0, drift_trans=0.0, dt=np.float64):
    """C2 for the pairs (a[k], b[k]) in THIS order (C3 calls it with a < b only): s2 [len(a)], +inf where a closure has
    status 1, where M fails the pivot rule or where the value is not finite."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    Tja, Tjb = S.Tj[a], S.Tj[b]
    RjaT = np.swapaxes(Tja[:, :3, :3], -1, -2)
    RX = RjaT @ Tjb[:, :3, :3]
    tX = (RjaT @ (Tjb[:, :3, 3] - Tja[:, :3, 3])[..., None])[..., 0]
    r = residual(S.B[b] @ S.Ti[a], Tja, S.Z[a], dt)
    Ad = np.zeros((len(a), 6, 6), dt)
    Ad[:, :3, :3] = RX
    Ad[:, 3:, 3:] = RX
    Ad[:, 3:, :3] = skew(tX, dt) @ RX
    d = np.abs(S.pi[a] - S.pi[b]) + np.abs(S.pj[a] - S.pj[b])
    M = S.Sigma[a] + Ad @ (S.Sigma[b] @ np.swapaxes(Ad, -1, -2))
    dr, dtr = (dt(drift_rot) * dt(drift_rot)) * d, (dt(drift_trans) * dt(drift_trans)) * d
    for k in range(3):
        M[:, k, k] += dr
        M[:, 3 + k, 3 + k] += dtr
    Lf, ok = chol6(sym_from_upper(M), dt)
    with np.errstate(all="ignore"):
        y = forward(Lf, r)
        s2 = ((((y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2]) + y[:, 3] * y[:, 3]) + y[:, 4] * y[:, 4]) + y[:, 5] * y[:, 5]
    ok &= (S.status[a] == 0) & (S.status[b] == 0) & np.isfinite(s2)
    return np.where(ok, s2, dt(np.inf))


def pair_s2_scalar(poses, src, tgt, Z, info, a, b, path=None, drift_rot=0.0, drift_trans=0.0):
    """One pair as the header words C2, float64, through pgo_ref's own residual and numpy's inverse: what pair_s2 must agree
    with to rounding (tests/test_pcm_cases_cpu.py)."""
    P = np.array(poses, np.float64)
    P[:, :3, 3] -= P[0, :3, 3].copy()
    pth = np.zeros(len(P)) if path is None else np.asarray(path, np.float64)
    ia, ja, ib, jb = int(src[a]), int(tgt[a]), int(src[b]), int(tgt[b])
    Za, Zb = np.asarray(Z[a], np.float64), np.asarray(Z[b], np.float64)
    X = np.linalg.inv(P[ja]) @ P[jb]
    r = R.residual(P[jb] @ Zb @ np.linalg.inv(P[ib]) @ P[ia], P[ja], Za)
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = Ad[3:, 3:] = X[:3, :3]
    Ad[3:, :3] = R.skew(X[:3, 3]) @ X[:3, :3]
    d = abs(pth[ia] - pth[ib]) + abs(pth[ja] - pth[jb])
    M = np.linalg.inv(R.sym_from_upper(info[a])) + Ad @ np.linalg.inv(R.sym_from_upper(info[b])) @ Ad.T
    M += np.diag([drift_rot ** 2 * d] * 3 + [drift_trans ** 2 * d] * 3)
    return float(r @ np.linalg.solve(M, r))


def s2_matrix(S, drift_rot=0.0, drift_trans=0.0, dt=np.float64):
    """C3's s2 [L, L]: entries (a, b) and (b, a) both the statistic of (min, max), the diagonal +inf."""
    out = np.full((S.L, S.L), np.inf, dt)
    a, b = np.triu_indices(S.L, 1)
    if len(a):
        v = pair_s2(S, a, b, drift_rot, drift_trans, dt)
        out[a, b] = v
        out[b, a] = v
    return out


# ---- C3 - C6: integers from here ---------------------------------------------------------------------------------------------------
def consistency_matrix(s2, chi2):
    return np.asarray(s2 < chi2)           # (+inf and the diagonal are not below any chi2)


def degree_score(C):
    Ci = C.astype(np.int64)
    return Ci.sum(1).astype(np.uint32), (Ci * (Ci @ Ci)).sum(1).astype(np.uint64)


def seeds_of(key, n_seeds):
    """C4: the n_seeds positions of largest key, ties to the smaller position; ranks past L are NONE."""
    order = np.lexsort((np.arange(len(key)), -key.astype(np.int64)))
    out = np.full(n_seeds, NONE, np.uint32)
    k = min(n_seeds, len(key))
    out[:k] = order[:k]
    return out


def greedy_clique(C, s):
    """C5: the members of the seed's clique as a bool vector."""
    K = np.zeros(len(C), bool)
    K[s] = True
    cand = C[s].copy()
    Ci = C.astype(np.int64)
    while cand.any():
        cnt = np.where(cand, Ci[:, cand].sum(1), -1)
        v = int(np.argmax(cnt))            # (the first maximum: the smaller position)
        K[v] = True
        cand &= C[v]
    return K


def select(C, n_seeds=64, min_clique=2):
    """C4 - C6 on a consistency matrix: dict(degree, score, seeds, clique_sizes, winner_rank, clique_size, mask, ok)."""
    deg, score = degree_score(C)
    seeds = seeds_of(score + deg.astype(np.uint64), n_seeds)
    sizes, cliques = np.zeros(n_seeds, np.uint32), {}
    for rank, s in enumerate(seeds):
        if s != NONE:
            cliques[rank] = greedy_clique(C, int(s))
            sizes[rank] = cliques[rank].sum()
    win = int(np.argmax(sizes))            # (the first maximum: the smaller rank)
    ok = int(sizes[win] >= min_clique)
    mask = cliques[win].astype(np.uint8) if ok else np.zeros(len(C), np.uint8)
    return dict(degree=deg, score=score, seeds=seeds, clique_sizes=sizes, winner_rank=win, clique_size=int(sizes[win]), mask=mask, ok=ok)


def consistency(poses, src, tgt, Z, info, path=None, dt=np.float64, **over):
    """The whole stage.  Adds status, s2 [L, L] and C to select()'s dict."""
    prm = dict(DEFAULTS, **over)
    S = setup(poses, src, tgt, Z, info, path, dt)
    s2 = s2_matrix(S, prm["drift_rot"], prm["drift_trans"], dt)
    C = consistency_matrix(s2, dt(prm["chi2"]))
    out = select(C, prm["n_seeds"], prm["min_clique"])
    out.update(status=S.status, s2=s2, C=C)
    return out
