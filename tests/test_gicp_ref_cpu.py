"""CPU: properties of the generalized ICP restatement tests/gicp_ref.py (the contract of gloc_reg_gicp_*) -- it is half the
point-to-point system at plane_eps = 1 and where normals are missing, H and g are the derivatives they claim to be, S is
positive definite, and on planes it reaches the pose point-to-point is still creeping towards."""
import numpy as np

import gicp_ref as R


def _rot(rx, ry, rz):
    return R.rodrigues(np.array([rx, ry, rz], np.float64))


def _se3(w, v):
    T = np.eye(4)
    T[:3, :3] = R.rodrigues(np.asarray(w, np.float64))
    T[:3, 3] = v
    return T


def _patches(rng, n_per, which=(0, 1, 2)):
    """Points on up to three mutually non-parallel planes (separate patches metres apart, so that a point's nearest
    neighbour is on its own plane) and the planes' unit normals, all turned by one rotation so that nothing is axis-aligned."""
    frames = [(np.array([0.0, 0.0, 0.0]), np.eye(3)),
              (np.array([-6.0, 0.0, 4.0]), _rot(0.0, np.pi / 2, 0.0)),
              (np.array([0.0, -7.0, 4.5]), _rot(-np.pi / 2 + 0.3, 0.0, 0.0))]
    W = _rot(0.21, -0.13, 0.4)
    pts, nrm = [], []
    for k in which:
        c, F = frames[k]
        uv = rng.uniform(-2.5, 2.5, (n_per, 2))
        local = np.concatenate([uv, np.zeros((n_per, 1))], axis=1)
        pts.append((local @ F.T + c) @ W.T)
        nrm.append(np.tile(W @ F[:, 2], (n_per, 1)))
    return np.concatenate(pts), np.concatenate(nrm)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _scene(seed=9, n_tgt=2000, n_src=500):
    rng = np.random.default_rng(seed)
    tgt, tn = _patches(rng, n_tgt)
    src, sn = _patches(rng, n_src)
    return src, sn, tgt, tn, _se3([0.02, 0.01, -0.015], [0.05, -0.03, 0.04])


def _p2p_system(p, q):
    """The point-to-point Gauss-Newton system of the same pairs: sum J^T J, sum J^T e."""
    J, e = R.jacobian(p), p - q
    return np.cumsum(np.einsum("mia,mib->mab", J, J), axis=0)[-1], np.cumsum(np.einsum("mia,mi->ma", J, e), axis=0)[-1], float(np.cumsum(np.einsum("mi,mi->m", e, e))[-1])


def test_plane_eps_one_is_half_the_point_to_point_system(oracle_mod):
    src, sn, tgt, tn, T0 = _scene()
    p, q, ns, nt = R.pairs(src, sn, tgt, tn, T0, oracle_mod.nn3, exact=True)
    assert len(p) == len(src)
    H, g, s, cnt = R.system(src, sn, tgt, tn, T0, oracle_mod.nn3, plane_eps=1.0, exact=True)
    Hp, gp, sp = _p2p_system(p, q)
    # a = 0: S = 2I, M = I / 2 whatever the normals; halving is exact in binary floating point
    assert cnt == len(p) and (H == 0.5 * Hp).all() and (g == 0.5 * gp).all() and s == 0.5 * sp
    r = R.align(src, sn, tgt, tn, oracle_mod.nn3, init_T=T0, max_iters=1, plane_eps=1.0, exact=True)
    xi = R.cholesky_solve(Hp, gp)
    step = _se3(xi[:3], xi[3:]) @ T0
    assert r["iters"] == 1 and np.abs(r["T"] - step).max() <= 1e-12


def test_g_is_half_the_gradient_of_the_weighted_residual(oracle_mod):
    src, sn, tgt, tn, T0 = _scene()
    p, q, ns, nt = R.pairs(src, sn, tgt, tn, T0, oracle_mod.nn3, exact=True)       # the pairs, then held fixed -- and so is M
    M = R.information(ns, nt, R.rotation(T0, True))
    H, g, s, cnt = R.system(src, sn, tgt, tn, T0, oracle_mod.nn3, exact=True)

    def f(xi):
        Tk = _se3(xi[:3], xi[3:])
        e = p @ Tk[:3, :3].T + Tk[:3, 3] - q
        return float(np.einsum("mi,mij,mj->", e, M, e))

    assert abs(f(np.zeros(6)) - s) <= 1e-12 * s
    h = 1e-6
    fd = np.array([(f(h * e) - f(-h * e)) / (2 * h) for e in np.eye(6)])
    assert np.abs(fd - 2 * g).max() <= 1e-7 * np.abs(2 * g).max()
    # H is symmetric, and the Gauss-Newton step is a descent step of that function
    assert np.abs(H - H.T).max() <= 1e-14 * np.abs(H).max()
    Ha, ga, _, _ = R.system(src, sn, tgt, tn, T0, oracle_mod.nn3, exact=True, how="adj")
    assert np.abs(Ha - Ha.T).max() <= 1e-14 * np.abs(Ha).max() and np.abs(Ha - H).max() <= 1e-12 * np.abs(H).max()
    xi = R.cholesky_solve(H, g)
    assert xi is not None and f(xi) < 0.05 * s
    # max_corr_dist drops pairs, by <=
    d = np.sqrt(((p - q) ** 2).sum(1))
    cut = float(np.float32(np.median(d)))
    _, _, _, c2 = R.system(src, sn, tgt, tn, T0, oracle_mod.nn3, max_corr_dist=cut, exact=True)
    assert 0 < c2 < cnt


def test_s_is_positive_definite_and_m_its_inverse():
    rng = np.random.default_rng(21)
    n = 5000
    ns, nt = _unit(rng, n), _unit(rng, n)
    nt[:500] = ns[:500] @ _rot(0.3, -0.2, 0.5).T          # the worst case: R n_s parallel to n_j
    Rm = _rot(0.3, -0.2, 0.5)
    for eps in (1e-3, 1e-2, 1.0):
        S = R.spread(ns, nt, Rm, eps)
        assert np.abs(S - S.transpose(0, 2, 1)).max() == 0
        w = np.linalg.eigvalsh(S)
        eps32 = float(np.float32(eps))
        assert w.min() >= 2 * eps32 * (1 - 1e-9) and w.max() <= 2 * (1 + 1e-12)
        assert abs(w[:500, 0] - 2 * eps32).max() <= 1e-12
        for how in ("inv", "adj"):
            M = R.information(ns, nt, Rm, eps, how)
            assert np.abs(M @ S - np.eye(3)).max() <= 1e-10      # (condition number 1 / eps)


def test_a_missing_normal_makes_that_side_isotropic(oracle_mod):
    src, sn, tgt, tn, T0 = _scene()
    nn = oracle_mod.nn3
    p, q, ns, nt = R.pairs(src, sn, tgt, tn, T0, nn, exact=True)
    Hp, gp, sp = _p2p_system(p, q)
    # none on either side: point-to-point (M = I / 2), by None or by zeros
    for a, b in ((None, None), (np.zeros_like(sn), np.zeros_like(tn))):
        H, g, s, cnt = R.system(src, a, tgt, b, T0, nn, exact=True)
        assert cnt == len(p) and (H == 0.5 * Hp).all() and (g == 0.5 * gp).all() and s == 0.5 * sp
    # one side only: S = 2I - a n n^T, whose inverse is (I + a / (2 - a) n n^T) / 2 for a unit n (Sherman-Morrison)
    a = 1.0 - float(np.float32(1e-3))
    Rm = R.rotation(T0, True)
    for ns_, nt_, n in ((None, tn, nt), (sn, None, ns @ Rm.T)):
        H, g, s, cnt = R.system(src, ns_, tgt, nt_, T0, nn, exact=True)
        M = 0.5 * (np.eye(3) + a / (2 - a) * n[:, :, None] * n[:, None, :])
        J, e = R.jacobian(p), p - q
        Hx = np.einsum("mia,mij,mjb->ab", J, M, J)
        gx = np.einsum("mia,mij,mj->a", J, M, e)
        assert cnt == len(p)
        assert np.abs(H - Hx).max() <= 1e-10 * np.abs(Hx).max() and np.abs(g - gx).max() <= 1e-10 * np.abs(Hx).max()
    # a pair keeps its place when only SOME points lack a normal
    tn2 = tn.copy()
    tn2[::3] = 0
    _, _, _, cnt = R.system(src, sn, tgt, tn2, T0, nn, exact=True)
    assert cnt == len(p)


def test_two_parallel_planes_with_lateral_offset_are_degenerate(oracle_mod):
    """Two parallel planes (a floor and a ceiling), the source the same planes moved sideways: nothing holds the lateral
    offset but the weight 1 / 2 a pair keeps ALONG its plane, against 1 / (2 plane_eps) across it.  The smallest Cholesky
    pivot (a lateral shift: N / 2) over the largest diagonal entry (a tilt: N r^2 / (2 plane_eps), r^2 = 2.1 m^2 the mean
    squared lever arm here) is therefore about plane_eps / 2 -- so the pivot rule's 1e-12 calls the scene degenerate for
    plane_eps below about 2e-12, the plane-to-plane limit, and not above.  Both sides are stated:
      plane_eps = 1e-14 (200 x inside that bound; exact unit normals in float64, so S stays positive definite): status 2,
      no update, the guess comes back;
      plane_eps = 1e-3 (the default): the pivot is 4.6e-4 of the largest diagonal entry, the job runs (status 0), moved
      by what point-to-point pairs see of the offset -- the planes' edges.  Degenerate at every plane_eps is what is degenerate for
      point-to-point (test_what_is_degenerate)."""
    rng = np.random.default_rng(5)

    def planes(n):
        uv = rng.uniform(-2.5, 2.5, (2 * n, 2))
        z = np.repeat([0.0, 3.0], n)
        return np.concatenate([uv, z[:, None]], axis=1), np.tile([0.0, 0.0, 1.0], (2 * n, 1))

    def smallest_pivot(eps):
        H, _, _, cnt = R.system(src, sn, tgt, tn, guess, oracle_mod.nn3, plane_eps=eps, exact=True)
        assert cnt == len(src)
        return np.diag(np.linalg.cholesky(H)).min() ** 2 / np.diag(H).max()

    tgt, tn = planes(3000)
    src, sn = planes(1000)
    guess = _se3([0.0, 0.0, 0.0], [0.15, -0.1, 0.0])
    limit, default = smallest_pivot(1e-14), smallest_pivot(1e-3)
    print(f"smallest Cholesky pivot over the largest diagonal entry: {limit:.2e} at plane_eps 1e-14, {default:.2e} at 1e-3")
    assert limit < 1e-12 < default
    assert 0.25e-14 < limit < 1e-14 and 0.25e-3 < default < 1e-3                       # about plane_eps / 2, within 2 x
    r = R.align(src, sn, tgt, tn, oracle_mod.nn3, init_T=guess, max_iters=10, plane_eps=1e-14, exact=True)
    assert r["status"] == 2 and r["iters"] == 0
    assert np.abs(r["T"] - guess).max() == 0
    r = R.align(src, sn, tgt, tn, oracle_mod.nn3, init_T=guess, max_iters=10, exact=True)
    assert r["status"] == 0 and r["iters"] == 10


def test_what_is_degenerate(oracle_mod):
    rng = np.random.default_rng(6)
    tgt, tn = _patches(rng, 2000)
    src, sn = _patches(rng, 500)
    guess = _se3([0.01, 0.0, -0.01], [0.02, 0.03, -0.05])
    nn = oracle_mod.nn3
    # fewer than 6 pairs, whatever their geometry
    for exact in (True, False):
        r = R.align(src[:5], sn[:5], tgt, tn, nn, init_T=guess, max_iters=3, exact=exact)
        assert r["status"] == 2 and r["iters"] == 0
        assert np.abs(r["T"] - guess.astype(np.float32 if not exact else np.float64)).max() == 0
    # a gate that rejects every pair
    far = src + 100.0
    r = R.align(far, sn, tgt, tn, nn, max_iters=3, max_corr_dist=1.0, exact=True)
    assert r["status"] == 2 and r["rmse"] == 0.0
    # points on one line through the origin, matched to themselves: the turn about the line moves nothing
    line = np.outer(np.linspace(-5, 5, 200), [1.0, 0.0, 0.0])
    r = R.align(line, None, line, None, nn, max_iters=3, exact=True)
    assert r["status"] == 2 and r["iters"] == 0


def _passes_until(trace, truth, tol):
    for k, T in enumerate(trace):
        dt, da = R.pose_err(truth, T)
        if dt < tol and da < tol:
            return k
    return len(trace) + 1


def test_on_planes_it_ends_closer_than_point_to_point(oracle_mod):
    rng = np.random.default_rng(3)
    tgt, tn = _patches(rng, 4000)
    on_planes, on_n = _patches(rng, 1500)                    # another sampling of the same planes
    truth = _se3([0.012, -0.02, 0.015], [0.06, -0.04, 0.05])
    src = (on_planes - truth[:3, 3]) @ truth[:3, :3]          # truth maps src onto the planes ...
    sn = on_n @ truth[:3, :3]                                 # ... and its normals onto theirs
    r = R.align(src, sn, tgt, tn, oracle_mod.nn3, max_iters=10, exact=True)
    assert r["status"] == 0 and r["iters"] == 10
    pp = R.p2p_align(src, tgt, oracle_mod.nn3, max_iters=30)
    eg, ep = R.pose_err(truth, r["T"]), R.pose_err(truth, pp["T"])
    print(f"error against the truth: generalized ICP after 10 passes {eg[0]:.2e} m {eg[1]:.2e} rad, point-to-point after 30 "
          f"{ep[0]:.2e} m {ep[1]:.2e} rad")
    assert eg[0] < ep[0] and eg[1] < ep[1]
    # with the stop test on it converges (status 1) and says so after the pass that made the small update
    r2 = R.align(src, sn, tgt, tn, oracle_mod.nn3, max_iters=30, trans_eps=1e-6, rot_eps=1e-6, exact=True)
    assert r2["status"] == 1 and r2["iters"] < 30
    # the fp32 form (the device's) lands within fp32 rounding of the same pose
    r3 = R.align(src.astype(np.float32), sn.astype(np.float32), tgt.astype(np.float32), tn.astype(np.float32), oracle_mod.nn3, max_iters=10)
    dt, da = R.pose_err(r["T"], r3["T"])
    assert dt < 1e-4 and da < 1e-4, (dt, da)
