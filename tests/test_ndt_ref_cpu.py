"""CPU: the NDT restatement (tests/ndt_ref.py) checked against itself -- analytic derivatives against finite
differences, the slot-sort filter against the literal 512-slot loop, the cell statistics against numpy.cov, and the
Newton / More-Thuente loop on a small synthetic scene."""
import numpy as np
import pytest

import ndt_ref as R


@pytest.fixture(scope="module")
def scene():
    from gloc3d_amd import synth
    w = synth.make_world(1001, n_boxes=400, extent=50.0)        # a cluttered scene (NDT's basin)
    tgt = synth.lidar_scan(w, None, seed=5, n_az=400)[:, :3]
    truth = synth.se3(2.0, (0.2, 0.0, 0.0))                      # source frame -> target frame
    src = synth.lidar_scan(w, truth, seed=6, n_az=400)[:, :3]
    return src, tgt, truth


def test_derivatives_match_finite_differences(scene):
    src, tgt, _ = scene
    cells = R.build_cells(tgt, 0.5)
    x = R.approx_voxel(src, 0.2)
    x = x[np.linalg.norm(x, axis=1) < 25][::2]    # short lever arms: a rotation by h moves no point across a cell's reach
    p0 = np.array([0.3, -0.05, 0.02, 0.004, -0.006, 0.05])     # every angle > 1e-3
    s, g, H = R.derivatives(x, cells, p0)
    assert s > 0 and np.abs(g).max() > 0
    h = 1e-7
    gn, Hn = np.zeros(6), np.zeros((6, 6))
    for i in range(6):
        dp = np.zeros(6)
        dp[i] = h
        sp, gp, _ = R.derivatives(x, cells, p0 + dp, hessian=False)
        sm, gm, _ = R.derivatives(x, cells, p0 - dp, hessian=False)
        gn[i] = (sp - sm) / (2 * h)
        Hn[:, i] = (gp - gm) / (2 * h)
    # (a pair entering or leaving the neighbourhood between +h and -h would show up as a jump: none at this pose)
    assert np.abs(gn - g).max() < 1e-4 * np.abs(g).max()
    assert np.abs(Hn - H).max() < 1e-4 * np.abs(H).max()
    assert np.abs(H - H.T).max() < 1e-9 * np.abs(H).max()


def test_slot_sort_filter_equals_the_sequential_loop(scene):
    src, _, _ = scene
    rng = np.random.default_rng(3)
    cases = [src, src - 30.0, np.array([[1.0, 2.0, 3.0]], np.float32),
             np.full((50, 3), 0.05, np.float32) + rng.random((50, 3)).astype(np.float32) * 0.1,
             rng.uniform(-40, 40, (3000, 3)).astype(np.float32)]
    nanc = src[:2000].copy()
    nanc[::7, 1] = np.nan
    nanc[::11, 0] = np.inf
    cases.append(nanc)
    for c in cases:
        a = R.approx_voxel(c, 0.2)
        b = R.approx_voxel_sequential(c, 0.2)
        assert len(a) == len(b)
        assert (R.sort_rows_by_bits(a).view(np.uint32) == R.sort_rows_by_bits(b).view(np.uint32)).all()
    # more distinct cells than slots: collisions flush early, so the filter keeps more points than a plain grid
    u = rng.uniform(-40, 40, (3000, 3)).astype(np.float32)
    assert len(R.approx_voxel(u, 0.2)) >= len(np.unique(np.floor(u * np.float32(5.0)), axis=0))


def test_cell_statistics_match_numpy_cov(scene):
    _, tgt, _ = scene
    c = R.build_cells(tgt + np.float32(80.0), 0.5, all_occupied=True)
    assert c["occupied"] > len(c["count"]) > 100
    p = (tgt + np.float32(80.0)).astype(np.float32)
    k = np.floor(p * (np.float32(1) / np.float32(0.5))).astype(np.int64)
    pk = R.pack_keys(k)
    assert (np.diff(c["packed"]) > 0).all()
    for j in range(0, len(c["count"]), max(1, len(c["count"]) // 40)):
        pts = p[pk == c["packed"][j]].astype(np.float64)
        assert len(pts) == c["count"][j] >= 6
        assert np.allclose(c["mean"][j], pts.mean(0), rtol=0, atol=1e-9)
        n = len(pts)
        cov = np.cov(pts.T, bias=True) * (n - 1) / n
        lam, V = np.linalg.eigh(cov)
        if lam[0] < 0.01 * lam[2]:
            lam = np.maximum(lam, 0.01 * lam[2])
            cov = V @ np.diag(lam) @ V.T
        ic = np.linalg.inv(cov)
        assert np.abs(c["icov"][j] - ic).max() < 1e-6 * np.abs(ic).max()


def test_euler_decomposition_round_trips():
    rng = np.random.default_rng(1)
    for _ in range(50):
        p = np.concatenate([rng.normal(size=3), rng.uniform(-3, 3, 3)])
        T = R.pose_matrix(p)
        q = R.pose_vector(T)
        assert 0 <= q[3] <= np.pi
        assert np.abs(R.pose_matrix(q) - T).max() < 1e-12


def test_newton_recovers_the_pose(scene):
    src, tgt, truth = scene
    cells = R.build_cells(tgt, 0.5)
    x = R.approx_voxel(src, 0.2)
    r = R.align(x, cells, init_T=np.eye(4))
    E = np.linalg.inv(truth) @ r["T"]
    ang = np.degrees(np.arccos(np.clip((np.trace(E[:3, :3]) - 1) / 2, -1, 1)))
    assert np.linalg.norm(E[:3, 3]) < 0.02 and ang < 0.1, (E, r)
    assert r["converged"] and 1 <= r["iters"] <= 35 and r["prob"] > 0
