"""CPU: properties of the voxelized generalized ICP restatement tests/vgicp_ref.py (the contract of gloc_reg_vgicp_*) --
with one point a voxel it IS generalized ICP on the same pairs, g is the derivative it claims to be, S is positive
definite for every mean of unit outer products, and the voxel rule's edges: faces, negative coordinates, the key range,
non-finite points, an empty target, a target without normals."""
import numpy as np

import gicp_ref as G
import vgicp_ref as V


def _se3(w, v):
    T = np.eye(4)
    T[:3, :3] = G.rodrigues(np.asarray(w, np.float64))
    T[:3, 3] = v
    return T


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _lattice(rng, n_side=9, res=1.0):
    """One point in every voxel of a block of n_side^3 voxels around the origin (negative coordinates included), well
    inside its voxel, with a random unit normal."""
    g = np.arange(n_side) - n_side // 2
    k = np.stack([m.ravel() for m in np.meshgrid(g, g, g, indexing="ij")], 1)
    tgt = ((k + rng.uniform(0.3, 0.7, k.shape)) * res).astype(np.float32)
    return tgt, _unit(rng, len(tgt)).astype(np.float32)


def _brute_nn(p, t):
    d = ((p[:, None, :].astype(np.float64) - t[None, :, :].astype(np.float64)) ** 2).sum(2)
    i = d.argmin(1)
    return i.astype(np.uint32), d[np.arange(len(p)), i].astype(np.float32)


def test_one_point_a_voxel_is_generalized_icp_on_the_same_pairs():
    rng = np.random.default_rng(5)
    tgt, tn = _lattice(rng)
    vox = V.voxels(tgt, tn, 1.0)
    assert len(vox["count"]) == len(tgt) and (vox["count"] == 1).all()
    T = _se3([0.01, -0.02, 0.015], [0.02, -0.01, 0.03])
    # every source point is a target point pulled back through T with 5 cm of noise: T moves it into its match's voxel
    pick = rng.choice(len(tgt), 300, replace=False)
    moved = tgt[pick].astype(np.float64) + rng.uniform(-0.05, 0.05, (300, 3))
    src = ((moved - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    sn = _unit(rng, 300).astype(np.float32)
    idx, _ = _brute_nn(G.move(T, src), tgt)
    assert (idx == pick).all()
    for gate in (0.0, 0.06):
        a = V.system(src, sn, vox, T, 1.0, 1, max_corr_dist=gate)
        b = G.system(src, sn, tgt, tn, T, _brute_nn, max_corr_dist=gate)
        scale = max(np.abs(b[0]).max(), np.abs(b[1]).max(), b[2])
        # (the mean of one point is corner + (x - corner): a rounding of 1e-16 of a coordinate, nothing else differs)
        assert a[3] == b[3] and (gate == 0.0 and a[3] == 300 or 0 < a[3] < 300)
        assert max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max(), abs(a[2] - b[2])) <= 1e-12 * scale
    # ... and Nbar of one point is its outer product exactly
    n64 = tn.astype(np.float64)
    order = np.lexsort((vox["key3"][:, 2], vox["key3"][:, 1], vox["key3"][:, 0]))
    assert (order == np.arange(len(order))).all()                     # listed by (kx, ky, kz)
    k, _ = V.cell_of(tgt, 1.0)
    at = np.searchsorted(vox["packed"], V._pack(k))
    assert (V.nn_full(vox["nn6"])[at] == n64[:, :, None] * n64[:, None, :]).all()


def test_g_is_half_the_gradient_of_the_weighted_residual():
    rng = np.random.default_rng(6)
    tgt = rng.uniform(-6, 6, (4000, 3)).astype(np.float32)            # ~2.3 points a voxel of 1 m: means and mixed Nbar
    tn = _unit(rng, len(tgt)).astype(np.float32)
    src = rng.uniform(-5, 5, (500, 3)).astype(np.float32)
    sn = _unit(rng, len(src)).astype(np.float32)
    T0 = _se3([0.02, 0.01, -0.015], [0.05, -0.03, 0.04])
    vox = V.voxels(tgt, tn, 1.0)
    assert vox["count"].max() > 1
    for nb in (1, 7, 27):
        p, mu, ns, Nbar, w = V.pairs(src, sn, vox, T0, 1.0, nb, exact=True)  # the pairs, then held fixed -- and so is M
        M = V.information(ns, Nbar, G.rotation(T0, True))
        H, g, s, cnt = V.system(src, sn, vox, T0, 1.0, nb, exact=True)
        assert cnt == len(p) and cnt > 300 * (1, 3, 10)[(1, 7, 27).index(nb)] // 3

        def f(xi):
            Tk = _se3(xi[:3], xi[3:])
            e = p @ Tk[:3, :3].T + Tk[:3, 3] - mu
            return float(np.einsum("m,mi,mij,mj->", w, e, M, e))

        assert abs(f(np.zeros(6)) - s) <= 1e-12 * s
        h = 1e-6
        fd = np.array([(f(h * e) - f(-h * e)) / (2 * h) for e in np.eye(6)])
        assert np.abs(fd - 2 * g).max() <= 1e-7 * np.abs(2 * g).max()
        assert np.abs(H - H.T).max() <= 1e-14 * np.abs(H).max()
        Ha, ga, sa, _ = V.system(src, sn, vox, T0, 1.0, nb, exact=True, how="adj", order="reversed")
        assert np.abs(Ha - H).max() <= 1e-12 * np.abs(H).max() and abs(sa - s) <= 1e-12 * s
        xi = G.cholesky_solve(H, g)
        assert xi is not None and f(xi) < f(np.zeros(6))
    # the neighbourhoods nest: 1 < 7 < 27 pairs, and the gate drops pairs by <=
    c = [V.system(src, sn, vox, T0, 1.0, nb)[3] for nb in (1, 7, 27)]
    assert c[0] < c[1] < c[2]
    assert 0 < V.system(src, sn, vox, T0, 1.0, 27, max_corr_dist=0.8)[3] < c[2]


def test_s_is_positive_definite_for_every_mean_of_unit_outer_products():
    rng = np.random.default_rng(21)
    n = 3000
    Rm = G.rodrigues(np.array([0.3, -0.2, 0.5]))
    ns = _unit(rng, n)
    # Nbar: means of 1 .. 8 unit outer products, some members missing (zero normals); the worst case first -- every member
    # parallel to R n_s
    Nbar = np.zeros((n, 3, 3))
    members = rng.integers(1, 9, n)
    for i in range(n):
        u = _unit(rng, members[i])
        if i < 300:
            u = np.tile(Rm @ ns[i], (members[i], 1))
        elif i % 5 == 0:
            u[rng.integers(0, members[i])] = 0.0
        Nbar[i] = (u[:, :, None] * u[:, None, :]).mean(0)
    for eps in (1e-3, 1e-2, 1.0):
        S = V.spread(ns, Nbar, Rm, eps)
        assert np.abs(S - S.transpose(0, 2, 1)).max() <= 1e-16
        w = np.linalg.eigvalsh(S)
        eps32 = float(np.float32(eps))
        assert w.min() >= 2 * eps32 * (1 - 1e-9) and w.max() <= 2 * (1 + 1e-12)
        assert abs(w[:300, 0] - 2 * eps32).max() <= 1e-12
        for how in ("inv", "adj"):
            M = V.information(ns, Nbar, Rm, eps, how)
            assert np.abs(M @ S - np.eye(3)).max() <= 1e-10


def test_voxel_edges():
    f32 = np.float32
    # a point exactly on a face belongs to the voxel that starts there; negative coordinates floor, they do not truncate
    pts = np.array([[1.0, 0.0, 0.0], [0.999, 0.0, 0.0], [-0.25, -1.0, 0.5], [-1.0, -0.001, 0.0], [2.5, 2.5, 2.5]], f32)
    k, ok = V.cell_of(pts, 1.0)
    assert ok.all() and k.tolist() == [[1, 0, 0], [0, 0, 0], [-1, -1, 0], [-1, -1, 0], [2, 2, 2]]
    k, ok = V.cell_of(pts, 0.5)
    assert k.tolist() == [[2, 0, 0], [1, 0, 0], [-1, -2, 1], [-2, -1, 0], [5, 5, 5]]
    vox = V.voxels(pts, None, 1.0)
    assert vox["key3"].tolist() == [[-1, -1, 0], [0, 0, 0], [1, 0, 0], [2, 2, 2]] and vox["count"].tolist() == [2, 1, 1, 1]
    assert np.abs(vox["mean"][0] - pts[2:4].astype(np.float64).mean(0)).max() <= 1e-15
    assert V.voxels(pts, None, 1.0, min_points=2)["key3"].tolist() == [[-1, -1, 0]]
    # the key range: |k| >= 2^20 is in no voxel, 2^20 - 1 is; NaN and inf are in none
    lim = float(1 << 20)
    # (-2^20 + 0.5 floors to -2^20, outside; truncated it would be inside)
    odd = np.array([[lim, 0, 0], [lim - 1, 0, 0], [-lim, 0, 0], [-lim + 1, 0, 0], [0, np.nan, 0], [np.inf, 0, 0], [0, 0, -np.inf],
                    [3e38, 0, 0], [-lim + 0.5, 0, 0]], f32)
    k, ok = V.cell_of(odd, 1.0)
    assert ok.tolist() == [False, True, False, True, False, False, False, False, False]
    assert k[1].tolist() == [(1 << 20) - 1, 0, 0] and k[3].tolist() == [-(1 << 20) + 1, 0, 0]
    vox = V.voxels(odd, None, 1.0)
    assert vox["count"].tolist() == [1, 1] and np.isfinite(vox["mean"]).all()
    # a source point beside the last voxel of the range: its neighbour outside the range is no pair, and nothing overflows
    for nb in (1, 7, 27):
        p = V.pairs(odd, None, vox, np.eye(4), 1.0, nb)
        assert len(p[0]) == 2 and (p[4] == 1).all()
    # an empty target, and a source of non-finite points: no pairs, a zero system
    empty = V.voxels(np.zeros((0, 3), f32), None, 1.0)
    assert len(empty["count"]) == 0 and empty["mean"].shape == (0, 3) and empty["nn6"].shape == (0, 6)
    H, g, s, cnt = V.system(pts, None, empty, np.eye(4), 1.0, 27)
    assert cnt == 0 and not H.any() and not g.any() and s == 0.0
    r = V.align(pts, None, np.zeros((0, 3), f32), None, init_T=_se3([0, 0, 0.1], [1, 2, 3]), max_iters=4)
    assert r["status"] == 2 and r["iters"] == 0 and r["rmse"] == 0.0
    assert V.system(odd[4:7], None, V.voxels(pts, None, 1.0), np.eye(4), 1.0, 27)[3] == 0


def test_a_target_without_normals_makes_that_side_isotropic():
    rng = np.random.default_rng(8)
    tgt = rng.uniform(-3, 3, (600, 3)).astype(np.float32)
    src = rng.uniform(-3, 3, (200, 3)).astype(np.float32)
    sn = _unit(rng, len(src)).astype(np.float32)
    T = _se3([0.01, 0.02, -0.01], [0.02, 0.0, -0.03])
    vox = V.voxels(tgt, np.zeros_like(tgt), 1.0)
    assert not vox["nn6"].any() and (V.voxels(tgt, None, 1.0)["nn6"] == vox["nn6"]).all()
    p, mu, ns, Nbar, w = V.pairs(src, sn, vox, T, 1.0, 7)
    assert len(p) > 200 and not Nbar.any()
    a = 1.0 - float(np.float32(1e-3))
    S = V.spread(ns, Nbar, G.rotation(T))
    m = ns @ G.rotation(T).T
    assert np.abs(S - (2.0 * np.eye(3) - a * (m[:, :, None] * m[:, None, :]))).max() == 0
    # without normals on the source either, every pair has M = I / 2: half the weighted point-to-voxel-mean system
    H, g, s, cnt = V.system(src, None, vox, T, 1.0, 7)
    J, e = G.jacobian(p), p - mu
    Hp = np.einsum("m,mia,mib->ab", w, J, J)
    assert cnt == len(p) and np.abs(H - 0.5 * Hp).max() <= 1e-12 * np.abs(Hp).max()
    assert abs(s - 0.5 * float(np.einsum("m,mi,mi->", w, e, e))) <= 1e-12 * s
