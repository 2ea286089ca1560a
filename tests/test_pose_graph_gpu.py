"""GPU: one end-to-end run of the pose graph on synthetic resident scans -- ray-cast scans along a short loop, generalized
ICP over the odometry pairs and the loop closures, gloc_reg_evaluate_pairs for the information matrices, PoseGraph, the
optimiser -- reduces the drift injected into the initial trajectory."""
import numpy as np
import pytest

import pgo_cases as G

pytestmark = pytest.mark.gpu

N, RADIUS, N_AZ = 6, 4.0, 200


def test_registered_pairs_to_corrected_poses(capi):
    from gloc3d_amd import synth
    from gloc3d_amd.pose_graph import PoseGraph
    world = synth.make_world(2024)
    truth = []
    for k in range(N):
        a = 2 * np.pi * k / N
        truth.append(synth.se3(np.rad2deg(a) + 90.0, (RADIUS * np.cos(a), RADIUS * np.sin(a), 0.0)))
    truth = np.array(truth)
    store = capi.ScanStore()
    reg = capi.Registrar(store=store)
    ids = [store.add(np.ascontiguousarray(synth.lidar_scan(world, truth[k], seed=2024 + k, n_az=N_AZ)[:, :3])) for k in range(N)]
    node = {sid: k for k, sid in enumerate(ids)}
    # the pairs: odometry k + 1 -> k, and the closures 5 -> 0, 4 -> 0, 3 -> 1; started a little off the true relative pose
    pairs = [(k + 1, k) for k in range(N - 1)] + [(5, 0), (4, 0), (3, 1)]
    rng = np.random.default_rng(7)
    init = np.array([G.left(np.concatenate([rng.normal(size=3) * 0.01, rng.normal(size=3) * 0.05]), np.linalg.inv(truth[j]) @ truth[i])
                     for i, j in pairs])
    src, tgt = [ids[i] for i, _ in pairs], [ids[j] for _, j in pairs]
    T, rmse, iters, status = reg.gicp_pairs(src, tgt, init)
    # the initial trajectory: the truth with a drift that grows along the chain
    pg = PoseGraph()
    drifted = [truth[0]]
    for k in range(1, N):
        step = G.left(np.array([0.0, 0.0, 0.03, 0.15, -0.1, 0.0]), np.linalg.inv(truth[k - 1]) @ truth[k])
        drifted.append(drifted[-1] @ step)
    for k in range(N):
        pg.add_node(drifted[k], fixed=(k == 0))
    kept = pg.add_registered(reg, node, src[:N - 1], tgt[:N - 1], T[:N - 1], robust=False)
    kept += pg.add_registered(reg, node, src[N - 1:], tgt[N - 1:], T[N - 1:], min_fitness=0.3)
    assert len(kept) == len(pairs) == pg.n_edges
    err = lambda P: max(np.linalg.norm(P[k][:3, 3] - truth[k][:3, 3]) for k in range(N))
    before = err(pg.poses)
    P, (s2, w), res = pg.optimize(robust=capi.default_robust_params(kind=capi.ROBUST_CAUCHY, scale=3.0))
    after = err(P)
    print(f"pose graph end to end: node error {before:.3f} m -> {after:.3f} m, status {res.status}, iters {res.iters}, cost {res.cost_initial:.3e} -> {res.cost_final:.3e}")
    assert np.isfinite(P).all() and res.accepted > 0 and res.cost_final < res.cost_initial
    assert after < before
    assert P[0].tobytes() == np.asarray(drifted[0], np.float64).tobytes()
    assert pg.prune(0.0) == 0 and pg.prune(2.0) == len(pairs) and pg.n_edges == 0           # every weight is at most 1
    pg.close()
    reg.close()
    store.close()
