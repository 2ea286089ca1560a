"""The float64 contract of the pose-graph optimisation (include/gloc3d.h, gloc_pgo_*): residual, Jacobian, robust
objective, linearisation, and the Levenberg-Marquardt loop with a dense solve and with the device's block-Jacobi PCG
restated in numpy.  Every function takes `dt` (numpy.float64 by default): the GPU tests evaluate a case in float64 and in
numpy.longdouble and take the difference as the formula's rounding scale.

Conventions: node k has pose (R_k, t_k), node -> map.  Edge e = (i, j, Z, Omega): Z maps source i -> target j,
Z ~ T_j^-1 T_i.  Perturbations are left ones, (exp(w) R, exp(w) t + v), xi = (w, v), rotation first.
"""
import numpy as np

NONE, HUBER, CAUCHY, TUKEY, GEMAN_MCCLURE = range(5)
# (the stops the CPU tests of this file run at, tighter than gloc_pgo_default_params' 1e-6; a GPU test that compares the
# device with this file passes its stops to both)
DEFAULTS = dict(max_iters=50, pcg_max_iters=200, lambda_init=1e-4, pcg_tol=1e-8, rot_eps=1e-9, trans_eps=1e-9, grad_eps=1e-9)


def skew(a, dt=np.float64):
    z = dt(0)
    return np.array([[z, -a[2], a[1]], [a[2], z, -a[0]], [-a[1], a[0], z]], dt)


def exp_so3(w, dt=np.float64):
    """Rodrigues as gn6_kernels.hpp::chol_rodrigues states it."""
    w = np.asarray(w, dt)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    a, b = dt(1), dt(0.5)
    if th > 0:
        a = np.sin(th) / th
        sh = np.sin(dt(0.5) * th)
        b = dt(2) * (sh * sh) / th2
    K = skew(w, dt)
    return np.eye(3, dtype=dt) + a * K + b * (K @ K)


def log_so3(R, dt=np.float64):
    """The rotation vector of R, |w| < pi: v = vee(R - R^T) / 2 has |v| = sin th, th = atan2(|v|, (tr R - 1) / 2)."""
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dt) * dt(0.5)
    s = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    c = (((R[0, 0] + R[1, 1]) + R[2, 2]) - dt(1)) * dt(0.5)
    if s < dt(1e-8):
        return v * (dt(1) + s * s / dt(6))
    return v * (np.arctan2(s, c) / s)


def jl_inv(w, dt=np.float64):
    """The inverse of SO(3)'s left Jacobian: I - [w]x / 2 + c [w]x^2, c = 1/th^2 - (1 + cos th) / (2 th sin th)."""
    th = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    c = dt(1) / dt(12)
    if not th < dt(1e-6):
        c = dt(1) / (th * th) - (dt(1) + np.cos(th)) / (dt(2) * th * np.sin(th))
    K = skew(w, dt)
    return np.eye(3, dtype=dt) - dt(0.5) * K + c * (K @ K)


def residual(Ti, Tj, Z, dt=np.float64, jac=False):
    """r (6), and with jac the 6 x 6 A of r(delta) = r + A (delta_i - delta_j)."""
    Ri, ti, Rj, tj, Rz, tz = Ti[:3, :3], Ti[:3, 3], Tj[:3, :3], Tj[:3, 3], Z[:3, :3], Z[:3, 3]
    RE = Rj.T @ Ri @ Rz.T
    REtz = RE @ tz
    tE = Rj.T @ (ti - tj) - REtz
    w = log_so3(RE, dt)
    r = np.concatenate([w, tE])
    if not jac:
        return r
    A = np.zeros((6, 6), dt)
    A[:3, :3] = jl_inv(w, dt) @ Rj.T
    A[3:, :3] = skew(REtz, dt) @ Rj.T - Rj.T @ skew(ti, dt)
    A[3:, 3:] = Rj.T
    return r, A


def weight(kind, s2, c2, dt=np.float64):
    """robust.hpp::weight."""
    if kind == NONE:
        return dt(1)
    t = s2 / c2
    if kind == HUBER:
        return dt(1) if t <= 1 else dt(1) / np.sqrt(t)
    if kind == CAUCHY:
        return dt(1) / (dt(1) + t)
    if kind == TUKEY:
        return (dt(1) - t) * (dt(1) - t) if t <= 1 else dt(0)
    return dt(1) / ((dt(1) + t) * (dt(1) + t))


def rho(kind, s2, c2, dt=np.float64):
    """The objective whose derivative in s2 is weight()."""
    if kind == NONE:
        return s2
    t = s2 / c2
    if kind == HUBER:
        return s2 if t <= 1 else c2 * (dt(2) * np.sqrt(t) - dt(1))
    if kind == CAUCHY:
        return c2 * np.log1p(t)
    if kind == TUKEY:
        u = dt(1) - t
        return (c2 / dt(3)) * (dt(1) - u * u * u) if t <= 1 else c2 / dt(3)
    return s2 / (dt(1) + t)


def sym_from_upper(M):
    return np.triu(M) + np.triu(M, 1).T


def origin_of(poses, fixed):
    return np.array(poses[int(np.flatnonzero(fixed)[0])][:3, 3])


class Lin:
    pass


def linearize(poses, fixed, src, tgt, Z, info, mask=None, kind=NONE, scale=1.0, dt=np.float64, shift=True):
    """poses [n,4,4], Z [m,4,4] (float32 values), info [m,6,6] -> r, s2, w, rho, W [m,6,6], b [m,6], g [n,6], Hd [n,6,6],
    F.  Translations are taken relative to the first fixed node's (shift=False: as they are)."""
    n, m = len(poses), len(src)
    P = np.array(poses, dt)
    if shift:
        P[:, :3, 3] -= np.asarray(origin_of(poses, fixed), dt)
    Zd, Om = np.asarray(Z).astype(dt), np.asarray(info).astype(dt)
    c2 = dt(np.float32(scale)) * dt(np.float32(scale))
    L = Lin()
    L.r, L.s2, L.w, L.rho = np.zeros((m, 6), dt), np.zeros(m, dt), np.zeros(m, dt), np.zeros(m, dt)
    L.W, L.b = np.zeros((m, 6, 6), dt), np.zeros((m, 6), dt)
    L.g, L.Hd = np.zeros((n, 6), dt), np.zeros((n, 6, 6), dt)
    for e in range(m):
        i, j = int(src[e]), int(tgt[e])
        r, A = residual(P[i], P[j], Zd[e], dt, jac=True)
        O = sym_from_upper(Om[e])
        y = O @ r
        s2 = r @ y
        k = kind if (mask is None or mask[e]) else NONE
        w = weight(k, s2, c2, dt)
        L.r[e], L.s2[e], L.w[e], L.rho[e] = r, s2, w, rho(k, s2, c2, dt)
        L.W[e] = w * (A.T @ O @ A)
        L.b[e] = w * (A.T @ y)
    for e in range(m):                       # CSR order: ascending edge index at every node
        i, j = int(src[e]), int(tgt[e])
        L.g[i] += L.b[e]
        L.g[j] -= L.b[e]
        L.Hd[i] += L.W[e]
        L.Hd[j] += L.W[e]
    L.F = L.rho.sum(dtype=dt)
    return L


def free_nodes(fixed, src, tgt, n):
    deg = np.bincount(np.concatenate([src, tgt]).astype(np.int64), minlength=n)
    return (~np.asarray(fixed, bool)) & (deg > 0)


def chol6(H):
    """gn6_kernels.hpp's Cholesky and pivot rule: the lower factor, or None."""
    L = np.array(H, np.float64)
    dmax = max(0.0, L.diagonal().max())
    for j in range(6):
        d = L[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 1e-12 * dmax:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (L[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return np.tril(L)


def matvec(L, src, tgt, free, lam, x):
    y = np.zeros_like(x)
    d = L.W @ (x[src] - x[tgt])[:, :, None]
    np.add.at(y, src, d[:, :, 0])
    np.subtract.at(y, tgt, d[:, :, 0])
    y += lam * (L.Hd @ x[:, :, None])[:, :, 0]
    y[~free] = 0.0
    return y


def solve_dense(L, src, tgt, free, lam):
    n = len(free)
    idx = np.flatnonzero(free)
    pos = -np.ones(n, np.int64)
    pos[idx] = np.arange(len(idx))
    H = np.zeros((6 * len(idx), 6 * len(idx)))
    for k in idx:
        if chol6((1.0 + lam) * L.Hd[k]) is None:
            return None, 0
        a = 6 * pos[k]
        H[a:a + 6, a:a + 6] += (1.0 + lam) * L.Hd[k]
    for e in range(len(src)):
        a, b = pos[src[e]], pos[tgt[e]]
        if a >= 0 and b >= 0:
            H[6 * a:6 * a + 6, 6 * b:6 * b + 6] -= L.W[e]
            H[6 * b:6 * b + 6, 6 * a:6 * a + 6] -= L.W[e]
    x = np.zeros((n, 6))
    x[idx] = np.linalg.solve(H, -L.g[idx].reshape(-1)).reshape(-1, 6)
    return x, 0


def solve_pcg(L, src, tgt, free, lam, tol, max_iters, hist=None):
    """Block-Jacobi preconditioned conjugate gradients from x = 0 on (H + lam D) x = -g; M = ((1 + lam) H_kk)^-1.
    hist (a dict, optional) receives rr: |residual|^2 before iteration 0 and after every iteration, g2, and breakdown:
    whether the loop left through `not pAp > 0`."""
    n = len(free)
    if hist is not None:
        hist.update(rr=[], g2=0.0, breakdown=False)
    Minv = np.zeros((n, 6, 6))
    for k in np.flatnonzero(free):
        Lk = chol6(L.Hd[k])                    # (the pivot rule does not depend on the factor 1 + lam)
        if Lk is None:
            return None, 0
        Li = np.linalg.inv(Lk)
        Minv[k] = (Li.T @ Li) / (1.0 + lam)
    prec = lambda v: (Minv @ v[:, :, None])[:, :, 0]
    x = np.zeros((n, 6))
    r = np.where(free[:, None], -L.g, 0.0)
    g2 = (r * r).sum()
    z = prec(r)
    p, rz, rr, it = z.copy(), (r * z).sum(), g2, 0
    if hist is not None:
        hist["g2"] = float(g2)
        hist["rr"].append(float(rr))
    while it < max_iters and not rr <= tol * tol * g2:
        Ap = matvec(L, src, tgt, free, lam, p)
        pAp = (p * Ap).sum()
        if not pAp > 0:
            if hist is not None:
                hist["breakdown"] = True
            break
        a = rz / pAp
        x += a * p
        r -= a * Ap
        it += 1
        rr = (r * r).sum()
        if hist is not None:
            hist["rr"].append(float(rr))
        z = prec(r)
        rz_new = (r * z).sum()
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, it


def retract(P, x):
    Q = P.copy()
    for k in range(len(P)):
        if x[k].any():
            E = exp_so3(x[k, :3])
            Q[k, :3, :3] = E @ P[k, :3, :3]
            Q[k, :3, 3] = E @ P[k, :3, 3] + x[k, 3:]
    return Q


def optimize(poses, fixed, src, tgt, Z, info, mask=None, kind=NONE, scale=1.0, solver="dense", trace=None, **over):
    """Levenberg-Marquardt with Marquardt scaling.  Returns dict(poses, s2, weight, iters, accepted, pcg_iters, status,
    cost_initial, cost_final, lam, grad_inf).  trace (a list, optional) receives one dict per attempt: gain, accepted, lam
    (the attempt's), max_w, max_v (the step's), grad_inf (of the trial linearisation), pcg (solve_pcg's hist; PCG only)."""
    prm = dict(DEFAULTS, **over)
    poses = np.asarray(poses, np.float64)
    fixed, src, tgt = np.asarray(fixed, bool), np.asarray(src, np.int64), np.asarray(tgt, np.int64)
    n = len(poses)
    free = free_nodes(fixed, src, tgt, n)
    org = origin_of(poses, fixed)
    P = poses.copy()
    P[:, :3, 3] -= org
    lin = lambda Q: linearize(Q, fixed, src, tgt, Z, info, mask, kind, scale, shift=False)
    L = lin(P)
    ginf = lambda L_: float(np.abs(L_.g[free]).max()) if free.any() else 0.0
    out = dict(iters=0, accepted=0, pcg_iters=0, status=0, cost_initial=float(L.F), lam=prm["lambda_init"])
    lam, nu = prm["lambda_init"], 2.0
    if not free.any():
        out["status"] = 2
    elif prm["grad_eps"] > 0 and ginf(L) <= prm["grad_eps"]:
        out["status"] = 3
    else:
        for _ in range(prm["max_iters"]):
            out["iters"] += 1
            hist = {} if trace is not None else None
            if solver == "dense":
                x, it = solve_dense(L, src, tgt, free, lam)
            else:
                x, it = solve_pcg(L, src, tgt, free, lam, prm["pcg_tol"], prm["pcg_max_iters"], hist)
            out["pcg_iters"] += it
            if x is None:
                out["status"] = 2
                break
            Pn = retract(P, x)
            Ln = lin(Pn)
            den = float((x * (lam * (L.Hd @ x[:, :, None])[:, :, 0] - L.g)).sum())
            gain = (L.F - Ln.F) / den if den != 0 else -1.0
            if trace is not None:
                trace.append(dict(gain=float(gain), accepted=bool(gain > 0 and np.isfinite(Ln.F)), lam=float(lam), pcg=hist, grad_inf=ginf(Ln),
                                  max_w=float(np.linalg.norm(x[:, :3], axis=1).max()), max_v=float(np.linalg.norm(x[:, 3:], axis=1).max())))
            if gain > 0 and np.isfinite(Ln.F):
                P, L = Pn, Ln
                out["accepted"] += 1
                lam, nu = lam * max(1.0 / 3.0, 1.0 - (2.0 * gain - 1.0) ** 3), 2.0
                mw, mv = np.linalg.norm(x[:, :3], axis=1).max(), np.linalg.norm(x[:, 3:], axis=1).max()
                if prm["rot_eps"] > 0 and prm["trans_eps"] > 0 and mw <= prm["rot_eps"] and mv <= prm["trans_eps"]:
                    out["status"] = 1
                    break
                if prm["grad_eps"] > 0 and ginf(L) <= prm["grad_eps"]:
                    out["status"] = 3
                    break
            else:
                lam, nu = lam * nu, 2.0 * nu
    res = P.copy()
    res[:, :3, 3] += org
    res[~free] = poses[~free]
    out.update(poses=res, s2=L.s2, weight=L.w, cost_final=float(L.F), lam=lam, grad_inf=ginf(L))
    return out
