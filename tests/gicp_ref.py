"""Float64 restatement of the generalized (plane-to-plane) ICP refinement (gloc_reg_gicp_*): the executable contract of
gloc3d_amd/csrc/gicp_kernels.hpp.  numpy plus a 1-NN search handed in (the project's oracle `nn3`: exact, fp32 un-fused
distance, smallest index among equals).  Both scans' normals are inputs; a zero normal means "no normal".

One pass at pose T = (R, t), source -> target (include/gloc3d.h), a = 1 - plane_eps (plane_eps as its fp32 value):
  p = R s + t in fp32 with the pose rounded to fp32 (p2l_ref.move); j = 1-NN of p; the pair is used iff d2 and p are finite
  and max_corr_dist <= 0 or d2 <= max_corr_dist^2; C_A = I - a n_s n_s^T, C_B = I - a n_j n_j^T (zero normal: I);
  m = R n_s with R the fp32 pose widened, S = C_B + R C_A R^T = 2I - a (n_j n_j^T + m m^T), M = S^-1; e = p - q_j,
  J = [-[p]x , I] for T <- exp(xi) T, xi = (w, v); H = sum J^T M J, g = sum J^T M e, sum e^T M e; fewer than 6 pairs or a
  Cholesky pivot <= 1e-12 max diag(H): degenerate (status 2); H xi = -g; T <- (Rodrigues(w), v) T.

A zero normal on either side is KEPT (that side's covariance is I) and the pair counted; a non-finite source point is in
no pair; an empty target gives no pairs.

M is frozen at the linearisation point of each pass: Gauss-Newton as in fast_gicp, not PCL's BFGS inner loop.

`exact=True` keeps p and R in float64.  `how` picks the inverse ("inv": numpy.linalg.inv, "adj": the symmetric adjugate)
and `order` the order the pairs are summed in ("forward", "reversed": one after the other, which no reduction tree is
further from) -- two evaluations of the same formulas whose difference is the restatement's own noise floor.
"""
import numpy as np

from p2l_ref import EVENTS, _sum, cholesky_solve, gauss_newton, move, p2p_align, pose_err, rodrigues  # noqa: F401  (re-exported: the tests' R.*)


def rotation(T, exact=False):
    """R as a pass uses it on the normals: the fp32-rounded pose widened to float64, or T itself when exact."""
    T = np.asarray(T, np.float64)
    return T[:3, :3] if exact else T.astype(np.float32).astype(np.float64)[:3, :3]


def pairs(src, src_nrm, tgt, tgt_nrm, T, nn, max_corr_dist=0.0, exact=False):
    """(p, q, n_s, n_j) of the pairs one pass uses, float64 [m, 3] each.  A normals argument of None: no normals."""
    p = move(T, src, exact)
    if len(tgt) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))
    idx, d2 = nn(p.astype(np.float32), np.asarray(tgt, np.float32))
    idx = idx.astype(np.int64)
    ok = np.isfinite(d2) & np.isfinite(p).all(1) & (idx < len(tgt))
    if max_corr_dist > 0:
        g2 = np.float32(max_corr_dist) * np.float32(max_corr_dist)
        ok &= d2 <= g2
    idx = np.where(ok, idx, 0)
    ns = np.zeros((len(p), 3)) if src_nrm is None else np.asarray(src_nrm, np.float64)
    nt = np.zeros((len(tgt), 3)) if tgt_nrm is None else np.asarray(tgt_nrm, np.float64)
    return p[ok].astype(np.float64), np.asarray(tgt)[idx[ok]].astype(np.float64), ns[ok], nt[idx[ok]]


def spread(ns, nt, R, plane_eps=1e-3):
    """S [m, 3, 3] = C_B + R C_A R^T = 2I - a (n_j n_j^T + m m^T), m = R n_s."""
    a = 1.0 - float(np.float32(plane_eps))
    m = ns @ R.T
    return 2.0 * np.eye(3) - a * (nt[:, :, None] * nt[:, None, :] + m[:, :, None] * m[:, None, :])


def adjugate_inverse(S):
    """The inverse of symmetric 3 x 3 matrices [m, 3, 3] by cofactors."""
    xx, xy, xz, yy, yz, zz = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    cxx, cxy, cxz = yy * zz - yz * yz, xz * yz - xy * zz, xy * yz - xz * yy
    cyy, cyz, czz = xx * zz - xz * xz, xy * xz - xx * yz, xx * yy - xy * xy
    det = xx * cxx + xy * cxy + xz * cxz
    return np.stack([np.stack([cxx, cxy, cxz], 1), np.stack([cxy, cyy, cyz], 1), np.stack([cxz, cyz, czz], 1)], 1) / det[:, None, None]


def information(ns, nt, R, plane_eps=1e-3, how="inv"):
    S = spread(ns, nt, R, plane_eps)
    if len(S) == 0:
        return S
    return np.linalg.inv(S) if how == "inv" else adjugate_inverse(S)


def jacobian(p):
    """J [m, 3, 6] = [-[p]x , I]: the derivative of exp(xi) p at xi = 0, xi = (w, v)."""
    J = np.zeros((len(p), 3, 6))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    J[:, 0, 1], J[:, 0, 2] = z, -y
    J[:, 1, 0], J[:, 1, 2] = -z, x
    J[:, 2, 0], J[:, 2, 1] = y, -x
    J[:, :, 3:] = np.eye(3)
    return J


def system_of_pairs(p, q, ns, nt, R, plane_eps=1e-3, how="inv", order="forward"):
    """H [6, 6], g [6], sum e^T M e, pairs used -- of pairs already chosen."""
    M = information(ns, nt, R, plane_eps, how)
    e = p - q
    J = jacobian(p)
    MJ = np.einsum("mij,mjb->mib", M, J)
    Me = np.einsum("mij,mj->mi", M, e)
    H = _sum(np.einsum("mia,mib->mab", J, MJ), order)
    g = _sum(np.einsum("mia,mi->ma", J, Me), order)
    s = float(_sum(np.einsum("mi,mi->m", e, Me), order))
    return H, g, s, len(p)


def system(src, src_nrm, tgt, tgt_nrm, T, nn, max_corr_dist=0.0, plane_eps=1e-3, exact=False, how="inv", order="forward"):
    p, q, ns, nt = pairs(src, src_nrm, tgt, tgt_nrm, T, nn, max_corr_dist, exact)
    return system_of_pairs(p, q, ns, nt, rotation(T, exact), plane_eps, how, order)


def align(src, src_nrm, tgt, tgt_nrm, nn, init_T=None, max_iters=30, max_corr_dist=0.0, trans_eps=0.0, rot_eps=0.0,
          plane_eps=1e-3, exact=False, how="inv", order="forward", events=None):
    """The whole refinement: dict(T float64 [4, 4], iters, status 0 cap / 1 converged / 2 degenerate, rmse, trace, steps);
    `events` as p2l_ref.align."""
    kw = dict(max_corr_dist=max_corr_dist, plane_eps=plane_eps, exact=exact, how=how, order=order)
    return gauss_newton(lambda T: system(src, src_nrm, tgt, tgt_nrm, T, nn, **kw), init_T, max_iters, trans_eps, rot_eps,
                        exact, events)
