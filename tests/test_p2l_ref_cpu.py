"""CPU: properties of the point-to-plane restatement tests/p2l_ref.py (the contract of gloc_reg_p2l_*) -- it slides along
planes where point-to-point creeps, a single plane is degenerate, and H, g are the derivatives they claim to be."""
import numpy as np
import pytest

import p2l_ref as R


def _rot(rx, ry, rz):
    return R.rodrigues(np.array([rx, ry, rz], np.float64))


def _patches(rng, n_per, which=(0, 1, 2)):
    """Points on up to three mutually non-parallel planes (separate patches metres apart, so that a point's nearest
    neighbour is on its own plane) and the planes' unit normals, all turned by one rotation so that nothing is axis-aligned."""
    frames = [(np.array([0.0, 0.0, 0.0]), np.eye(3)),                             # normal z
              (np.array([-6.0, 0.0, 4.0]), _rot(0.0, np.pi / 2, 0.0)),            # normal x
              (np.array([0.0, -7.0, 4.5]), _rot(-np.pi / 2 + 0.3, 0.0, 0.0))]     # normal ~y, tilted
    W = _rot(0.21, -0.13, 0.4)
    pts, nrm = [], []
    for k in which:
        c, F = frames[k]
        uv = rng.uniform(-2.5, 2.5, (n_per, 2))
        local = np.concatenate([uv, np.zeros((n_per, 1))], axis=1)
        pts.append((local @ F.T + c) @ W.T)
        nrm.append(np.tile(W @ F[:, 2], (n_per, 1)))
    return np.concatenate(pts), np.concatenate(nrm)


def _se3(w, v):
    T = np.eye(4)
    T[:3, :3] = R.rodrigues(np.asarray(w, np.float64))
    T[:3, 3] = v
    return T


def _passes_until(trace, truth, tol):
    for k, T in enumerate(trace):
        dt, da = R.pose_err(truth, T)
        if dt < tol and da < tol:
            return k
    return len(trace) + 1


def test_point_to_plane_slides_where_point_to_point_creeps(oracle_mod):
    rng = np.random.default_rng(3)
    tgt, nrm = _patches(rng, 4000)
    on_planes, _ = _patches(rng, 1500)                       # another sampling of the same planes
    truth = _se3([0.012, -0.02, 0.015], [0.06, -0.04, 0.05])
    src = (on_planes - truth[:3, 3]) @ truth[:3, :3]          # truth maps src onto the planes
    r = R.align(src, tgt, nrm, oracle_mod.nn3, max_iters=8, exact=True)
    dt, da = R.pose_err(truth, r["T"])
    assert r["status"] == 0 and r["iters"] == 8
    assert dt < 1e-9 and da < 1e-9, (dt, da)
    n_p2l = _passes_until(r["trace"], truth, 1e-6)
    assert n_p2l <= 5                                        # "a handful"
    pp = R.p2p_align(src, tgt, oracle_mod.nn3, max_iters=40)
    n_p2p = _passes_until(pp["trace"], truth, 1e-6)
    print(f"passes to 1e-6 of the truth: point-to-plane {n_p2l}, point-to-point {n_p2p} (42: not within 40)")
    assert n_p2l < n_p2p
    # with the stop test on it converges (status 1) and says so after the pass that made the small update
    r2 = R.align(src, tgt, nrm, oracle_mod.nn3, max_iters=30, trans_eps=1e-8, rot_eps=1e-8, exact=True)
    assert r2["status"] == 1 and r2["iters"] < 10
    # the fp32 form (the device's) lands within fp32 rounding of the same pose
    r3 = R.align(src.astype(np.float32), tgt.astype(np.float32), nrm.astype(np.float32), oracle_mod.nn3, max_iters=8)
    dt, da = R.pose_err(truth, r3["T"])
    assert dt < 1e-5 and da < 1e-5, (dt, da)


def test_a_single_plane_is_degenerate(oracle_mod):
    rng = np.random.default_rng(5)
    tgt, nrm = _patches(rng, 3000, which=(0,))
    on_plane, _ = _patches(rng, 1000, which=(0,))
    guess = _se3([0.01, 0.0, -0.01], [0.02, 0.03, -0.05])
    for exact in (True, False):
        r = R.align(on_plane, tgt, nrm, oracle_mod.nn3, init_T=guess, max_iters=10, exact=exact)
        assert r["status"] == 2 and r["iters"] == 0
        assert np.abs(r["T"] - guess.astype(np.float32 if not exact else np.float64)).max() == 0
    # fewer than 6 pairs: degenerate whatever their geometry
    r = R.align(on_plane[:5], tgt, nrm, oracle_mod.nn3, max_iters=3, exact=True)
    assert r["status"] == 2
    # pairs without a normal are not pairs
    H, g, s2, cnt = R.system(on_plane, tgt, np.zeros_like(nrm), np.eye(4), oracle_mod.nn3, exact=True)
    assert cnt == 0 and s2 == 0 and not H.any() and not g.any()


def test_h_and_g_are_the_derivatives_of_half_the_squared_residuals(oracle_mod):
    rng = np.random.default_rng(9)
    tgt, nrm = _patches(rng, 2000)
    src, _ = _patches(rng, 500)
    T0 = _se3([0.02, 0.01, -0.015], [0.05, -0.03, 0.04])
    p, q, n = R.pairs(src, tgt, nrm, T0, oracle_mod.nn3, exact=True)      # the correspondences, then held fixed
    assert len(p) == len(src)
    r0, J = R.jacobian(p, q, n)
    H, g, s2, cnt = R.system(src, tgt, nrm, T0, oracle_mod.nn3, exact=True)
    assert cnt == len(p) and abs(s2 - r0 @ r0) <= 1e-12 * s2
    assert np.abs(H - J.T @ J).max() <= 1e-12 * np.abs(H).max() and np.abs(g - J.T @ r0).max() <= 1e-12 * np.abs(g).max()

    def res(xi):
        Tk = _se3(xi[:3], xi[3:])
        pk = p @ Tk[:3, :3].T + Tk[:3, 3]
        return np.einsum("ij,ij->i", n, pk - q)

    h = 1e-6
    Jfd = np.stack([(res(h * e) - res(-h * e)) / (2 * h) for e in np.eye(6)], axis=1)
    assert np.abs(Jfd - J).max() <= 1e-8 * np.abs(J).max()
    gfd = np.array([(0.5 * res(h * e) @ res(h * e) - 0.5 * res(-h * e) @ res(-h * e)) / (2 * h) for e in np.eye(6)])
    assert np.abs(gfd - g).max() <= 1e-7 * np.abs(g).max()
    # the Gauss-Newton step is a descent step of that function
    xi = R.cholesky_solve(H, g)
    assert xi is not None and res(xi) @ res(xi) < 0.05 * (r0 @ r0)
    # max_corr_dist drops pairs, by <=
    d = np.sqrt(((p - q) ** 2).sum(1))
    cut = float(np.float32(np.median(d)))
    _, _, _, c2 = R.system(src, tgt, nrm, T0, oracle_mod.nn3, max_corr_dist=cut, exact=True)
    assert 0 < c2 < cnt
