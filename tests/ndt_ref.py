"""float64 numpy restatement of NDT scan registration -- the executable contract of the device code in
gloc3d_amd/csrc/ndt.hip (gloc_reg_ndt_*), and of nothing else.

The reference calls PCL for this (ndt_match_3d, registration/global_registration.cpp:250-330): an ApproximateVoxelGrid
(0.2 m) on the source, a NormalDistributionsTransform (0.5 m cells, step 0.1, epsilon 0.01, 35 iterations) against the
unfiltered target.  PCL is not available to this project, so what follows restates PCL 1.8-1.10's algorithm as it is
publicly documented (Magnusson 2009; More & Thuente 1994); parity with PCL itself is NOT pinned.

Every function works on float32 points (as a scan store holds them) and computes in float64 where the text says so.
"""
import numpy as np

DEFAULTS = dict(source_leaf=0.2, resolution=0.5, step_size=0.1, trans_eps=0.01, max_iters=35, outlier_ratio=0.55,
                min_points_per_cell=6, min_covar_eigvalue_mult=0.01)
HIST = 512          # ApproximateVoxelGrid's hash slots
KEY_BIAS = 1 << 20  # packed cell key: 21 bits per axis, (kx + B) << 42 | (ky + B) << 21 | (kz + B)


# ---- source filter: ApproximateVoxelGrid ------------------------------------------------------------------------
def voxel_slots(pts, leaf):
    """Per point: cell k = floor(p * (1/leaf)) in fp32 -> int32, hash slot, and whether the point is finite."""
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    inv = np.float32(1.0) / np.float32(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(p * inv)
    ok = (np.abs(f) < np.float32(2 ** 30)).all(1)      # finite, and a cell index int32 holds
    k = np.where(ok[:, None], f, np.float32(0)).astype(np.int32)
    ku = k.astype(np.uint32)
    h = (ku[:, 0] * np.uint32(7171) + ku[:, 1] * np.uint32(3079) + ku[:, 2] * np.uint32(4231)) & np.uint32(HIST - 1)
    return k, h, ok


def approx_voxel_sequential(pts, leaf):
    """The literal 512-slot loop: a point whose slot holds another cell flushes that slot first; every non-empty slot
    is flushed at the end.  Centroids are fp32 sums in point order divided by the fp32 count."""
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    k, h, ok = voxel_slots(p, leaf)
    cnt = [0] * HIST
    cell = [None] * HIST
    acc = [None] * HIST
    out = []
    for i in range(len(p)):
        if not ok[i]:
            continue
        s = int(h[i])
        ki = (int(k[i, 0]), int(k[i, 1]), int(k[i, 2]))
        if cnt[s] and cell[s] != ki:
            out.append(acc[s] / np.float32(cnt[s]))
            cnt[s] = 0
        if cnt[s] == 0:
            acc[s] = np.zeros(3, np.float32)
        cell[s] = ki
        cnt[s] += 1
        acc[s] = acc[s] + p[i]
    for s in range(HIST):
        if cnt[s]:
            out.append(acc[s] / np.float32(cnt[s]))
    return np.array(out, np.float32).reshape(-1, 3)


def approx_voxel(pts, leaf):
    """The same filter without a sequential scan (what the device does): stable-sort the finite points by slot; inside
    a slot every run of consecutive equal cells is one output point, its centroid summed in point order.  Rows come out
    in (slot, first point) order; approx_voxel_sequential emits the same rows in another order."""
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    if leaf <= 0:
        return p[np.isfinite(p).all(1)].copy()
    k, h, ok = voxel_slots(p, leaf)
    idx = np.nonzero(ok)[0]
    order = idx[np.argsort(h[idx], kind="stable")]
    if len(order) == 0:
        return np.zeros((0, 3), np.float32)
    hs, ks = h[order], k[order]
    start = np.ones(len(order), bool)
    start[1:] = (hs[1:] != hs[:-1]) | (ks[1:] != ks[:-1]).any(1)
    first = np.nonzero(start)[0]
    length = np.diff(np.append(first, len(order)))
    acc = np.zeros((len(first), 3), np.float32)
    for j in range(int(length.max())):          # position j of every run at once: fp32 sums in point order
        m = length > j
        acc[m] = acc[m] + p[order[first[m] + j]]
    return acc / length.astype(np.float32)[:, None]


def sort_rows_by_bits(a):
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
    b = a.view(np.uint32)
    return a[np.lexsort((b[:, 2], b[:, 1], b[:, 0]))]


# ---- target cells: VoxelGridCovariance ---------------------------------------------------------------------------
def pack_keys(k):
    k = np.asarray(k, np.int64) + KEY_BIAS
    return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]


def build_cells(pts, resolution, min_points=6, eig_mult=0.01, all_occupied=False):
    """Cells of the target: k = floor(p * (1/resolution)) in fp32; n, sum p and sum p p^T in fp64 relative to the cell's
    corner k * resolution; mean = corner + sum/n; cov = (S2 - 2 sum mean^T)/n + mean mean^T (relative coordinates), times
    (n - 1)/n.  Valid: n >= min_points, eigenvalues (ascending) l0, l1 >= 0 and l2 > 0; if l0 < eig_mult * l2 the small
    ones are raised to it and cov = V diag(l) V^T; icov = cov^-1, dropped if it has an infinite entry.
    Returns dict(key3 [m,3] int32, count [m], mean [m,3], icov [m,3,3], packed [m]) sorted by key (valid cells only;
    all_occupied: also 'occupied', the number of occupied cells)."""
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    p = p[np.isfinite(p).all(1)]
    inv = np.float32(1.0) / np.float32(resolution)
    k = np.floor(p * inv).astype(np.int64)
    keep = (np.abs(k) < KEY_BIAS).all(1)
    p, k = p[keep], k[keep]
    uniq, inv_idx, n = np.unique(k, axis=0, return_inverse=True, return_counts=True)
    inv_idx = inv_idx.reshape(-1)
    corner = uniq.astype(np.float64) * float(resolution)
    rel = p.astype(np.float64) - corner[inv_idx]
    S1 = np.zeros((len(uniq), 3))
    S2 = np.zeros((len(uniq), 3, 3))
    np.add.at(S1, inv_idx, rel)
    np.add.at(S2, inv_idx, rel[:, :, None] * rel[:, None, :])
    nd = n.astype(np.float64)
    m_rel = S1 / nd[:, None]
    cov = (S2 - 2.0 * S1[:, :, None] * m_rel[:, None, :]) / nd[:, None, None] + m_rel[:, :, None] * m_rel[:, None, :]
    cov = cov * ((nd - 1.0) / nd)[:, None, None]
    mean = corner + m_rel
    sel = n >= min_points
    out_key, out_n, out_mean, out_icov = [], [], [], []
    for c in np.nonzero(sel)[0]:
        lam, V = np.linalg.eigh(cov[c])
        if lam[0] < 0 or lam[1] < 0 or lam[2] <= 0:
            continue
        C = cov[c]
        lo = eig_mult * lam[2]
        if lam[0] < lo:
            lam = lam.copy()
            lam[0] = lo
            if lam[1] < lo:
                lam[1] = lo
            C = V @ np.diag(lam) @ V.T
        ic = np.linalg.inv(C)
        if not np.isfinite(ic).all():
            continue
        out_key.append(uniq[c])
        out_n.append(n[c])
        out_mean.append(mean[c])
        out_icov.append(ic)
    key3 = np.array(out_key, np.int32).reshape(-1, 3)
    d = dict(key3=key3, count=np.array(out_n, np.uint32), mean=np.array(out_mean).reshape(-1, 3),
             icov=np.array(out_icov).reshape(-1, 3, 3), packed=pack_keys(key3))
    if all_occupied:
        d["occupied"] = len(uniq)
    return d


# ---- pose parameterisation ---------------------------------------------------------------------------------------
def _rot(axis, c, s):
    if axis == 0:
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)
    if axis == 1:
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


def _drot(axis, c, s, order):
    """d^order/dangle^order of the elementary rotation (order 1 or 2)."""
    if order == 1:
        c_, s_ = -s, c          # d cos = -sin, d sin = cos
    else:
        c_, s_ = -c, -s
    M = _rot(axis, c_, s_)
    M[axis, axis] = 0.0
    return M


def pose_matrix(p):
    """T(p) = Trans(tx, ty, tz) Rx(rx) Ry(ry) Rz(rz), fp64, real cos / sin."""
    p = np.asarray(p, np.float64)
    R = _rot(0, np.cos(p[3]), np.sin(p[3])) @ _rot(1, np.cos(p[4]), np.sin(p[4])) @ _rot(2, np.cos(p[5]), np.sin(p[5]))
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = p[:3]
    return T


def _cs_small(a):
    """PCL's small-angle rule for the derivatives: |angle| < 1e-4 -> cos = 1, sin = 0."""
    return (1.0, 0.0) if abs(a) < 1e-4 else (np.cos(a), np.sin(a))


def angle_derivatives(p):
    """M[k] = dR/dangle_k (3x3, k = rx, ry, rz) and MH[(k, l)] = d2R/dangle_k dangle_l (k <= l), with the small-angle
    rule -- the matrix form of Magnusson's eq. 6.19 / 6.21 (PCL's j_ang / h_ang vectors are their rows)."""
    cs = [_cs_small(p[3]), _cs_small(p[4]), _cs_small(p[5])]
    R = [_rot(a, *cs[a]) for a in range(3)]
    D1 = [_drot(a, *cs[a], 1) for a in range(3)]
    D2 = [_drot(a, *cs[a], 2) for a in range(3)]

    def prod(orders):
        M = np.eye(3)
        for a in range(3):
            M = M @ (R[a] if orders[a] == 0 else D1[a] if orders[a] == 1 else D2[a])
        return M

    M = [prod([1 if a == k else 0 for a in range(3)]) for k in range(3)]
    MH = {}
    for k in range(3):
        for l in range(k, 3):
            o = [0, 0, 0]
            o[k] += 1
            o[l] += 1
            MH[(k, l)] = prod(o)
    return M, MH


def euler_xyz(R):
    """Eigen's R.eulerAngles(0, 1, 2) (R = Rx(a) Ry(b) Rz(c)), fp64: the first angle comes out in [0, pi]."""
    R = np.asarray(R, np.float64)
    r0 = np.arctan2(R[1, 2], R[2, 2])
    c2 = np.hypot(R[0, 0], R[0, 1])
    if r0 > 0:
        r0 -= np.pi
        r1 = np.arctan2(-R[0, 2], -c2)
    else:
        r1 = np.arctan2(-R[0, 2], c2)
    s1, c1 = np.sin(r0), np.cos(r0)
    r2 = np.arctan2(s1 * R[2, 0] - c1 * R[1, 0], c1 * R[1, 1] - s1 * R[2, 1])
    return -np.array([r0, r1, r2])


def pose_vector(T):
    T = np.asarray(T, np.float64)
    return np.concatenate([T[:3, 3], euler_xyz(T[:3, :3])])


# ---- score, gradient, Hessian --------------------------------------------------------------------------------------
def gauss_consts(resolution, outlier_ratio):
    c1 = 10.0 * (1.0 - outlier_ratio)
    c2 = outlier_ratio / resolution ** 3
    d3 = -np.log(c2)
    d1 = -np.log(c1 + c2) - d3
    d2 = -2.0 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / d1)
    return d1, d2


def neighbour_pairs(y, cells, resolution):
    """(point, cell) pairs: the valid cells whose mean lies strictly within `resolution` of the transformed point (only
    the 27 cells around its own can).  The point's own cell is floor(y * (1/resolution)) in fp64."""
    fin = np.isfinite(y).all(1)
    home = np.floor(np.where(fin[:, None], y, 0.0) * (1.0 / resolution)).astype(np.int64)
    keys = cells["packed"]
    pi, ci = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = home + np.array([dx, dy, dz])
                ok = fin & (np.abs(k) < KEY_BIAS - 1).all(1)
                q = pack_keys(np.where(ok[:, None], k, 0))
                j = np.searchsorted(keys, q)
                j = np.minimum(j, max(len(keys) - 1, 0))
                hit = ok & (len(keys) > 0) & (keys[j] == q) if len(keys) else np.zeros(len(y), bool)
                if not hit.any():
                    continue
                ii = np.nonzero(hit)[0]
                jj = j[ii]
                d = y[ii] - cells["mean"][jj]
                near = (d * d).sum(1) < resolution * resolution
                pi.append(ii[near])
                ci.append(jj[near])
    if not pi:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(pi), np.concatenate(ci)


def derivatives(src, cells, p, resolution=0.5, outlier_ratio=0.55, hessian=True):
    """score, gradient [6] and Hessian [6,6] at p (Magnusson 2009 eq. 6.9-6.13, PCL's computeDerivatives):
    x' = T(p) x - mean, e = exp(-d2/2 x'^T icov x'); a pair adds -d1 e to the score unless d2 e is outside [0, 1]
    (then it adds nothing)."""
    x = np.ascontiguousarray(src, np.float32).reshape(-1, 3).astype(np.float64)
    T = pose_matrix(p)
    y = x @ T[:3, :3].T + T[:3, 3]
    d1, d2 = gauss_consts(resolution, outlier_ratio)
    pi, ci = neighbour_pairs(y, cells, resolution)
    g = np.zeros(6)
    H = np.zeros((6, 6))
    if len(pi) == 0:
        return 0.0, g, H
    M, MH = angle_derivatives(p)
    xs = x[pi]
    d = y[pi] - cells["mean"][ci]
    ic = cells["icov"][ci]
    u = np.einsum("nij,nj->ni", ic, d)
    q = (d * u).sum(1)
    e = np.exp(-d2 * q / 2.0)
    de = d2 * e
    use = (de >= 0) & (de <= 1)
    score = float((-d1 * e[use]).sum())
    w = (d1 * de)[use]
    xs, u, ic = xs[use], u[use], ic[use]
    J = np.zeros((len(xs), 3, 6))
    J[:, :, :3] = np.eye(3)
    for k in range(3):
        J[:, :, 3 + k] = xs @ M[k].T
    a = np.einsum("ni,nij->nj", u, J)                                   # x'^T icov J_i
    g = (w[:, None] * a).sum(0)
    if hessian:
        JiJ = np.einsum("nki,nkl,nlj->nij", J, ic, J)                   # J_i^T icov J_j
        uH = np.zeros((len(xs), 6, 6))
        for (k, l), Mkl in MH.items():
            v = ((xs @ Mkl.T) * u).sum(1)
            uH[:, 3 + k, 3 + l] = v
            uH[:, 3 + l, 3 + k] = v
        H = (w[:, None, None] * (-d2 * a[:, :, None] * a[:, None, :] + uH + JiJ)).sum(0)
    return score, g, H


# ---- Newton with the More-Thuente line search ---------------------------------------------------------------------
def solve_newton(H, g):
    """delta = pinv(H) (-g): H is symmetric, so its SVD is its eigen-decomposition with |lambda| as singular values;
    singular values below max(6 eps sigma_max, DBL_MIN) are cut (Eigen's JacobiSVD default threshold)."""
    lam, V = np.linalg.eigh(H)
    s = np.abs(lam)
    cut = max(6 * np.finfo(np.float64).eps * (s.max() if len(s) else 0.0), np.finfo(np.float64).tiny)
    inv = np.where(s >= cut, 1.0 / np.where(lam == 0, 1.0, lam), 0.0)
    return V @ (inv * (V.T @ (-g)))


def _psi(a, f_a, f_0, g_0, mu):
    return f_a - f_0 - mu * g_0 * a


def _dpsi(g_a, g_0, mu):
    return g_a - mu * g_0


def _cubic(a_l, f_l, g_l, a_t, f_t, g_t):
    z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l
    w = np.sqrt(z * z - g_t * g_l)
    return a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w)


def _note(events, name):
    """Read-only instrumentation: record that a branch was taken (align's `events` list); no arithmetic."""
    if events is not None:
        events.append(name)


def trial_value(a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t, events=None):
    """More & Thuente's trial value selection, cases 1-4, as PCL's trialValueSelectionMT.  After update_interval has moved
    a_l to the last trial (its outcomes 2 and 3) the next call has a_t == a_l, f_t == f_l, g_t == g_l: that is case 3
    with a_c = a_s = NaN (0 / 0), and std::min / std::max (Python's too, in this argument order) return the bound
    a_t + 0.66 (a_u - a_t).  With finite values case 4 cannot be reached at all (tests/test_ndt_sweep_cpu.py says why)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return _trial_value(a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t, events)


def _trial_value(a_l, f_l, g_l, a_u, f_u, g_u, a_t, f_t, g_t, events):
    if f_t > f_l:
        _note(events, "trial_case_1")
        a_c = _cubic(a_l, f_l, g_l, a_t, f_t, g_t)
        a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t))
        return a_c if abs(a_c - a_l) < abs(a_q - a_l) else 0.5 * (a_q + a_c)
    if g_t * g_l < 0:
        _note(events, "trial_case_2")
        a_c = _cubic(a_l, f_l, g_l, a_t, f_t, g_t)
        a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l
        return a_c if abs(a_c - a_t) >= abs(a_s - a_t) else a_s
    if abs(g_t) <= abs(g_l):
        _note(events, "trial_case_3")
        a_c = _cubic(a_l, f_l, g_l, a_t, f_t, g_t)
        a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l
        a_n = a_c if abs(a_c - a_t) < abs(a_s - a_t) else a_s
        return min(a_t + 0.66 * (a_u - a_t), a_n) if a_t > a_l else max(a_t + 0.66 * (a_u - a_t), a_n)
    _note(events, "trial_case_4")
    return _cubic(a_u, f_u, g_u, a_t, f_t, g_t)


def update_interval(I, a_t, f_t, g_t, events=None):
    """PCL's updateIntervalMT on I = [a_l, f_l, g_l, a_u, f_u, g_u] (in place); True: the interval has converged."""
    if f_t > I[1]:
        _note(events, "interval_case_1")
        I[3:6] = [a_t, f_t, g_t]
        return False
    if g_t * (I[0] - a_t) > 0:
        _note(events, "interval_case_2")
        I[0:3] = [a_t, f_t, g_t]
        return False
    if g_t * (I[0] - a_t) < 0:
        _note(events, "interval_case_3")
        I[3:6] = I[0:3]
        I[0:3] = [a_t, f_t, g_t]
        return False
    _note(events, "interval_converged")
    return True


EVENTS = ("trial_case_1", "trial_case_2", "trial_case_3", "trial_case_4",
          "interval_case_1", "interval_case_2", "interval_case_3", "interval_converged",
          "interval_closed", "direction_reversed", "dphi0_zero", "trial_clamped_max", "trial_clamped_min",
          "search_cap", "hessian_reevaluated", "end_trans_eps", "end_iteration_cap", "end_zero_step", "end_nan_step")


def align(src, cells, init_T=None, params=None, trace=None, events=None):
    """PCL's computeTransformation: returns dict(T [4,4] fp64, p, prob, iters, converged, evals).  `src` is the FILTERED
    source.  converged: the loop stopped on the step criterion or a zero step (stricter than PCL's hasConverged(),
    which is also true at the iteration cap).
    events: an optional list that receives, in order, the names (EVENTS) of the branches the run takes; "first_clamped_max"
    / "first_clamped_min" (the first trial step min(|delta|, step_max) of a search, as opposed to a selected trial value)
    are recorded too.  "trial_clamped_max" / "_min" say which bound a selected trial value was outside of (above
    step_max / below step_min) before max(min(a, step_max), step_min); where step_min exceeds step_max the value that
    was cut at step_max ends at step_min.  Recording changes no value."""
    prm = dict(DEFAULTS, **(params or {}))
    res, o = prm["resolution"], prm["outlier_ratio"]
    eps, step_max, max_iters = prm["trans_eps"], prm["step_size"], prm["max_iters"]
    step_min = eps / 2
    mu, nu = 1e-4, 0.9
    n_src = len(src)
    p = pose_vector(np.eye(4) if init_T is None else np.asarray(init_T, np.float32).astype(np.float64))
    evals = 1
    score, g, H = derivatives(src, cells, p, res, o, True)
    iters = 0
    converged = False
    while True:
        delta = solve_newton(H, g)
        dn = float(np.sqrt(delta @ delta))
        if dn == 0 or dn != dn:
            converged = dn == dn
            _note(events, "end_zero_step" if converged else "end_nan_step")
            break
        d = delta / dn
        # computeStepLengthMT(p, d, dn, step_max, step_min)
        phi_0 = -score
        dphi_0 = -(g @ d)
        if dphi_0 >= 0:
            if dphi_0 == 0:
                _note(events, "dphi0_zero")
                a_t = 0.0
                x_t = p.copy()
                stepped = False
            else:
                _note(events, "direction_reversed")
                dphi_0 = -dphi_0
                d = -d
        if dphi_0 != 0:
            stepped = True
            I = [0.0, _psi(0.0, phi_0, phi_0, dphi_0, mu), _dpsi(dphi_0, dphi_0, mu),
                 0.0, _psi(0.0, phi_0, phi_0, dphi_0, mu), _dpsi(dphi_0, dphi_0, mu)]
            interval_converged = False
            open_interval = True
            a_t = max(min(dn, step_max), step_min)
            if events is not None and a_t != dn:
                events.append("first_clamped_max" if dn > step_max else "first_clamped_min")
            x_t = p + d * a_t
            score, g, H = derivatives(src, cells, x_t, res, o, True)
            evals += 1
            phi_t, dphi_t = -score, -(g @ d)
            psi_t, dpsi_t = _psi(a_t, phi_t, phi_0, dphi_0, mu), _dpsi(dphi_t, dphi_0, mu)
            step_iters = 0
            while (not interval_converged and step_iters < 10
                   and not (psi_t <= 0 and dphi_t <= -nu * dphi_0)):
                if open_interval:
                    a_t = trial_value(*I, a_t, psi_t, dpsi_t, events=events)
                else:
                    a_t = trial_value(*I, a_t, phi_t, dphi_t, events=events)
                if events is not None and (a_t > step_max or a_t < step_min):
                    events.append("trial_clamped_max" if a_t > step_max else "trial_clamped_min")
                # np.float64, so that the next selection's a_t == a_l (both clamped to one bound) divides as IEEE
                # arithmetic does (PCL's C++, the device): NaN, which min / max then drop -- not Python's ZeroDivisionError
                a_t = np.float64(max(min(a_t, step_max), step_min))
                x_t = p + d * a_t
                score, g, _ = derivatives(src, cells, x_t, res, o, False)
                evals += 1
                phi_t, dphi_t = -score, -(g @ d)
                psi_t, dpsi_t = _psi(a_t, phi_t, phi_0, dphi_0, mu), _dpsi(dphi_t, dphi_0, mu)
                if open_interval and (psi_t <= 0 and dpsi_t >= 0):
                    open_interval = False
                    _note(events, "interval_closed")
                    I[1] = I[1] + phi_0 - mu * dphi_0 * I[0]
                    I[2] = I[2] + mu * dphi_0
                    I[4] = I[4] + phi_0 - mu * dphi_0 * I[3]
                    I[5] = I[5] + mu * dphi_0
                if open_interval:
                    interval_converged = update_interval(I, a_t, psi_t, dpsi_t, events=events)
                else:
                    interval_converged = update_interval(I, a_t, phi_t, dphi_t, events=events)
                step_iters += 1
            if (events is not None and step_iters >= 10 and not interval_converged
                    and not (psi_t <= 0 and dphi_t <= -nu * dphi_0)):
                events.append("search_cap")
            if step_iters:
                _note(events, "hessian_reevaluated")
                _, _, H = derivatives(src, cells, x_t, res, o, True)
                evals += 1
        if trace is not None:
            trace.append((iters, a_t, score))
        p = p + d * a_t if stepped else p
        stop = iters > max_iters or (iters and abs(a_t) < eps)
        if stop:
            converged = bool(iters and abs(a_t) < eps)
            _note(events, "end_trans_eps" if converged else "end_iteration_cap")
            iters += 1
            break
        iters += 1
    return dict(T=pose_matrix(p), p=p, prob=score / n_src if n_src else 0.0, iters=iters, converged=converged,
                evals=evals)
