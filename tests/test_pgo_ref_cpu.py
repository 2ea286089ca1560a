"""CPU: the float64 contract of the pose-graph optimisation (tests/pgo_ref.py) checked against itself -- the Jacobian
against central differences, each objective's derivative against the library's weight, Levenberg-Marquardt on consistent
graphs, the dense solve against the PCG, and gauge freedom."""
import numpy as np
import pytest

import pgo_cases as G
import pgo_ref as R


def _unit(rng):
    a = rng.normal(size=3)
    return a / np.linalg.norm(a)


# the size of the residual rotation: 0, either side of the series threshold 1e-6, and up to 3.0 rad
THETAS = [0.0, 0.9e-6, 1.1e-6, 1e-3, 0.5, 1.5, 2.5, 3.0]


@pytest.mark.parametrize("theta", THETAS)
def test_jacobian_against_central_differences(theta):
    rng = np.random.default_rng(int(theta * 1e7) + 5)
    for _ in range(4):
        Tj = G.se3(rng.normal(size=3), rng.normal(size=3) * 20.0)
        Z = G.se3(rng.normal(size=3), rng.normal(size=3) * 5.0)
        E = G.se3(_unit(rng) * theta, rng.normal(size=3) * 0.5)          # the residual we want: T_j^-1 T_i = E Z
        Ti = Tj @ E @ Z
        r, A = R.residual(Ti, Tj, Z, jac=True)
        assert abs(np.linalg.norm(r[:3]) - theta) < 1e-9
        h = 1e-6
        for node, sign in ((0, 1.0), (1, -1.0)):
            num = np.empty((6, 6))
            for a in range(6):
                d = np.zeros(6)
                d[a] = h
                P = [G.left(d, Ti), Tj] if node == 0 else [Ti, G.left(d, Tj)]
                M = [G.left(-d, Ti), Tj] if node == 0 else [Ti, G.left(-d, Tj)]
                num[:, a] = (R.residual(P[0], P[1], Z) - R.residual(M[0], M[1], Z)) / (2 * h)
            # central differences at h = 1e-6: truncation ~ h^2, rounding ~ 1e-16 |t| / h with |t| ~ 30 m
            assert np.abs(num - sign * A).max() < 2e-7 * max(1.0, np.abs(A).max()), (theta, node)


@pytest.mark.parametrize("kind", [R.HUBER, R.CAUCHY, R.TUKEY, R.GEMAN_MCCLURE])
def test_rho_derivative_is_the_library_weight(capi, kind):
    rob = capi.default_robust_params(kind=kind, scale=1.5)
    c2 = 1.5 * 1.5
    for s2 in (0.0, 0.3, 1.0, 2.2, 2.3, 5.0, 40.0):
        w_lib = capi.robust_weight(rob, 0, s2)
        assert w_lib == R.weight(kind, np.float64(s2), np.float64(c2))
        if s2 > 0 and abs(s2 / c2 - 1.0) > 1e-3:                       # (Huber's and Tukey's kink at t = 1 has no derivative)
            h = 1e-5
            num = (R.rho(kind, np.float64(s2 + h), np.float64(c2)) - R.rho(kind, np.float64(s2 - h), np.float64(c2))) / (2 * h)
            assert abs(num - w_lib) < 1e-8
    assert R.rho(kind, np.float64(0.0), np.float64(c2)) == 0.0


def test_consistent_graph_has_zero_cost_and_lm_returns_to_the_truth():
    g = G.graph(24, 6, seed=11)
    L = R.linearize(g["truth"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"])
    assert L.F < 1e-6                                                   # Z is float32: (1e-7 x 30 m)^2 x 2e3 x 30 edges
    for solver in ("dense", "pcg"):
        out = R.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], solver=solver)
        er, et = G.rel_error(out["poses"], g["truth"])
        assert out["status"] in (1, 3) and er < 1e-5 and et < 1e-4, (solver, out["status"], er, et)
        assert out["cost_final"] < 1e-6 < out["cost_initial"]


@pytest.mark.parametrize("kind,outliers", [(R.NONE, 0.0), (R.CAUCHY, 0.2)])
def test_dense_and_pcg_agree(kind, outliers):
    g = G.graph(40, 12, seed=3, noise=1.0, outliers=outliers)
    mask = (~g["odo"]).astype(np.uint8)
    a = R.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], mask, kind, 3.0, solver="dense")
    b = R.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], mask, kind, 3.0, solver="pcg")
    er, et = G.rel_error(a["poses"], b["poses"])
    assert er < 1e-7 and et < 1e-6, (er, et)
    assert abs(a["cost_final"] - b["cost_final"]) < 1e-6 * a["cost_final"]


def test_gauge_a_rigid_motion_of_the_input_moves_the_output():
    g = G.graph(20, 5, seed=7, noise=1.0)
    M = G.se3([0.3, -0.2, 1.1], [40.0, -25.0, 3.0])
    a = R.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"])
    b = R.optimize(G.moved(g["init"], M), g["fixed"], g["src"], g["tgt"], g["Z"], g["info"])
    d = np.abs(G.moved(a["poses"], M) - b["poses"]).max()
    assert d < 1e-6, d
    assert np.array_equal(b["poses"][0], G.moved(g["init"], M)[0])      # the fixed node: bit for bit


def test_fixed_and_edgeless_nodes_keep_their_poses():
    g = G.graph(12, 3, seed=5, noise=1.0)
    init = np.concatenate([g["init"], [G.se3([0.1, 0.2, 0.3], [1.0, 2.0, 3.0])]])     # node 12 has no edge
    fixed = np.concatenate([g["fixed"], [0]]).astype(np.uint8)
    fixed[6] = 1
    out = R.optimize(init, fixed, g["src"], g["tgt"], g["Z"], g["info"])
    for k in (0, 6, 12):
        assert np.array_equal(out["poses"][k], init[k])
    out = R.optimize(init, np.ones(13, np.uint8), g["src"], g["tgt"], g["Z"], g["info"])
    assert out["status"] == 2 and out["iters"] == 0
