"""Float64 restatement of the point-to-plane ICP refinement (gloc_reg_p2l_*): the executable contract of
gloc3d_amd/csrc/p2l_kernels.hpp.  numpy plus a 1-NN search handed in (the project's oracle `nn3`: exact, fp32 un-fused
distance, smallest index among equals).  The target's normals are an input.

One pass at pose T = (R, t), source -> target (include/gloc3d.h):
  p = R s + t in fp32 with the pose rounded to fp32, ((r0 x + r1 y) + r2 z) + t un-fused -- what the device's search moves
  the source by; j = 1-NN of p; the pair is used iff d2 is finite, max_corr_dist <= 0 or d2 <= max_corr_dist^2, n_j != 0;
  r = n_j . (p - q_j), J = [p x n_j ; n_j] in fp64; H = sum J J^T, g = sum J r; fewer than 6 pairs or a Cholesky pivot
  <= 1e-12 max diag(H): degenerate (status 2); H xi = -g, xi = (w, v); T <- (Rodrigues(w), v) T.

A non-finite source point is in no pair (its p is not finite), and neither is a pair whose target normal is zero -- which
is what a non-finite or isolated target point has (oracle/ground_oracle.c: normal_of); an empty target gives no pairs.

`exact=True` keeps p in float64 (no fp32 rounding anywhere but inside the search): the form the CPU tests use to state
properties of the formulas to 1e-9.  `order` is the order the pairs are summed in ("forward", "reversed": one after the
other, which no reduction tree is further from) -- two evaluations of the same formulas whose difference is the
restatement's own noise floor.  `events`, a list, gets the branches of the loop a run takes (EVENTS).
"""
import numpy as np

# What align() records in `events`: how the run ended, and the two branches of an update that the end pose does not show.
EVENTS = ("converged", "capped", "degenerate_at_0", "degenerate_later", "zero_angle", "angle_above_0.3")


def move(T, src, exact=False):
    """The source moved by T: fp32, the device's operation order (math3.hpp xform) -- or float64 when exact."""
    if exact:
        T = np.asarray(T, np.float64)
        return np.asarray(src, np.float64) @ T[:3, :3].T + T[:3, 3]
    Tf = np.asarray(T, np.float64).astype(np.float32)
    s = np.asarray(src, np.float32)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    out = np.empty_like(s)
    for a in range(3):
        out[:, a] = ((Tf[a, 0] * x + Tf[a, 1] * y) + Tf[a, 2] * z) + Tf[a, 3]
    return out


def pairs(src, tgt, nrm, T, nn, max_corr_dist=0.0, exact=False):
    """(p, q, n) of the pairs one pass uses, float64 [m, 3] each."""
    p = move(T, src, exact)
    if len(tgt) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))
    idx, d2 = nn(p.astype(np.float32), np.asarray(tgt, np.float32))
    idx = idx.astype(np.int64)
    ok = np.isfinite(d2) & np.isfinite(p).all(1) & (idx < len(tgt))
    if max_corr_dist > 0:
        g2 = np.float32(max_corr_dist) * np.float32(max_corr_dist)
        ok &= d2 <= g2
    idx = np.where(ok, idx, 0)
    n = np.asarray(nrm)[idx]
    ok &= (n != 0).any(1)
    return p[ok].astype(np.float64), np.asarray(tgt)[idx[ok]].astype(np.float64), n[ok].astype(np.float64)


def jacobian(p, q, n):
    """r [m] and J [m, 6] = [p x n ; n]."""
    r = np.einsum("ij,ij->i", n, p - q)
    return r, np.concatenate([np.cross(p, n), n], axis=1)


def _sum(c, order):
    if len(c) == 0:
        return np.zeros(c.shape[1:])
    if order == "reversed":
        c = c[::-1]
    return np.cumsum(c, axis=0)[-1]


def system_of_pairs(p, q, n, order="forward"):
    """H [6, 6], g [6], sum r^2, pairs used -- of pairs already chosen, summed one after the other in `order`."""
    r, J = jacobian(p, q, n)
    return _sum(J[:, :, None] * J[:, None, :], order), _sum(J * r[:, None], order), float(_sum(r * r, order)), len(r)


def system(src, tgt, nrm, T, nn, max_corr_dist=0.0, exact=False, order="forward"):
    """H [6, 6], g [6], sum r^2, pairs used."""
    return system_of_pairs(*pairs(src, tgt, nrm, T, nn, max_corr_dist, exact), order=order)


def cholesky_solve(H, g):
    """xi with H xi = -g, or None when a pivot is <= 1e-12 of the largest diagonal entry (row-by-row Cholesky)."""
    L = np.zeros((6, 6))
    dmax = max(np.diag(H).max(), 0.0)
    for j in range(6):
        d = H[j, j] - L[j, :j] @ L[j, :j]
        if not d > 1e-12 * dmax:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        y[i] = (-g[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def rodrigues(w):
    th2 = float(w @ w)
    th = np.sqrt(th2)
    A, B = 1.0, 0.5
    if th > 0:
        A = np.sin(th) / th
        B = 2.0 * np.sin(0.5 * th) ** 2 / th2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)
    return np.eye(3) + A * K + B * (K @ K)


def gauss_newton(system_at, init_T, max_iters, trans_eps, rot_eps, exact, events=None):
    """The loop of passes both refinements share: system_at(T) -> H, g, squared residual, pairs.  A job converges only
    with BOTH eps set; with one of them 0 it runs to the cap."""
    T = np.eye(4) if init_T is None else np.asarray(init_T, np.float64).copy()
    if not exact:
        T = np.asarray(init_T if init_T is not None else np.eye(4), np.float32).astype(np.float64)
    ev = events if events is not None else []
    iters, status, trace, steps = 0, 0, [T.copy()], []
    for _ in range(int(max_iters)):
        H, g, _, cnt = system_at(T)
        xi = cholesky_solve(H, g) if cnt >= 6 else None
        if xi is None:
            status = 2
            break
        th, vn = float(np.sqrt(xi[:3] @ xi[:3])), float(np.linalg.norm(xi[3:]))
        if th == 0.0 and "zero_angle" not in ev:
            ev.append("zero_angle")
        if th > 0.3 and "angle_above_0.3" not in ev:
            ev.append("angle_above_0.3")
        Tk = np.eye(4)
        Tk[:3, :3] = rodrigues(xi[:3])
        Tk[:3, 3] = xi[3:]
        T = Tk @ T
        iters += 1
        trace.append(T.copy())
        steps.append((vn, th))
        if trans_eps > 0 and rot_eps > 0 and vn < trans_eps and th < rot_eps:
            status = 1
            break
    ev.append(("capped", "converged", "degenerate_at_0" if iters == 0 else "degenerate_later")[status])
    _, _, s, cnt = system_at(T)
    return dict(T=T, iters=iters, status=status, rmse=np.sqrt(s / cnt) if cnt else 0.0, trace=trace, steps=steps)


def align(src, tgt, nrm, nn, init_T=None, max_iters=30, max_corr_dist=0.0, trans_eps=0.0, rot_eps=0.0, exact=False,
          order="forward", events=None):
    """The whole refinement: dict(T float64 [4, 4], iters, status 0 cap / 1 converged / 2 degenerate, rmse, trace, steps
    [(|v|, |w|) of every update])."""
    return gauss_newton(lambda T: system(src, tgt, nrm, T, nn, max_corr_dist, exact, order), init_T, max_iters, trans_eps,
                        rot_eps, exact, events)


def p2p_align(src, tgt, nn, init_T=None, max_iters=30):
    """Point-to-point ICP (Kabsch on the 1-NN pairs) in float64 from the same start: the comparison of the sliding test."""
    T = np.eye(4) if init_T is None else np.asarray(init_T, np.float64).copy()
    trace = [T.copy()]
    for _ in range(int(max_iters)):
        p = move(T, src, True)
        idx, _ = nn(p.astype(np.float32), np.asarray(tgt, np.float32))
        q = np.asarray(tgt, np.float64)[idx.astype(np.int64)]
        pc, qc = p.mean(0), q.mean(0)
        U, _, Vt = np.linalg.svd((q - qc).T @ (p - pc))
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
        Tk = np.eye(4)
        Tk[:3, :3] = U @ D @ Vt
        Tk[:3, 3] = qc - Tk[:3, :3] @ pc
        T = Tk @ T
        trace.append(T.copy())
    return dict(T=T, trace=trace)


def pose_err(A, B):
    E = np.linalg.inv(np.asarray(A, np.float64)) @ np.asarray(B, np.float64)
    return np.linalg.norm(E[:3, 3]), np.linalg.norm(E[:3, :3] - np.eye(3)) / np.sqrt(2.0)    # (2 sin(th / 2): no arccos near 1)
