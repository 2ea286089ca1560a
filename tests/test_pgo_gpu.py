"""GPU: the pose-graph optimisation (gloc_pgo_*) against tests/pgo_ref.py.

Linearise.  The reference evaluates each case in float64 and in numpy.longdouble; the difference is the formula's rounding
scale, and the device is allowed 8 x that per output (another summation order, another libm), with a floor of 4 ulp of the
output's largest magnitude.  Scales measured for these cases (max over the case's outputs of |float64 - longdouble|; the
test recomputes them, these are for the reader -- DESIGN.md section 14 has the same table):
    case        r        s2       weight   g        Hdiag    cost
    pair        8.5e-17  7.2e-16  0        2.1e-13  1.1e-11  7.2e-16
    loop5       4.3e-16  1.6e-13  0        6.6e-12  5.1e-11  1.1e-14
    hub1        8.5e-16  1.9e-13  0        1.4e-11  7.5e-11  1.9e-13
    hub63       8.2e-15  1.2e-11  0        6.8e-10  1.8e-08  2.4e-12
    hub64       6.1e-15  1.9e-11  0        4.7e-09  2.2e-08  8.0e-12
    hub65       8.0e-15  1.2e-11  0        2.4e-09  4.0e-08  2.2e-11
    hub300      9.6e-15  1.5e-11  0        1.2e-09  9.1e-08  4.6e-11
    n257        1.0e-13  2.2e-09  0        2.5e-08  1.6e-07  2.5e-09
    robust1-4   1.0e-15  1.1e-11  6.9e-15  1.4e-11  4.4e-10  5.5e-13
(the drifted starts have s2 up to 1e6 and H entries up to 1e9: the scales are a few 1e-16 of those magnitudes)

Optimise.  Agreement with the reference's DENSE solve is asked to 10 x the disagreement of the reference's own dense and
PCG solves on the same case at the same stops (TIGHT below), measured on the CPU: DENSE_VS_PCG.
"""
import numpy as np
import pytest

import pgo_cases as G
import pgo_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
OUTS = ("r", "s2", "weight", "g", "Hdiag", "cost")


@pytest.fixture(scope="module")
def opt(capi):
    o = capi.PoseGraphOptimizer()
    yield o
    o.close()


def _robust(capi, kind, scale=3.0):
    return None if kind == R.NONE else capi.default_robust_params(kind=kind, scale=scale)


def _ref_lin(g, kind=R.NONE, scale=3.0, mask=None, dt=np.float64):
    L = R.linearize(g["init"], g["fixed"], g["src"].astype(np.int64), g["tgt"].astype(np.int64), g["Z"], g["info"], mask, kind, scale, dt)
    return dict(r=L.r, s2=L.s2, weight=L.w, g=L.g, Hdiag=np.array([R.sym_from_upper(h) for h in L.Hd]), cost=np.array(L.F), rho=L.rho)


def _check_lin(opt, capi, g, kind=R.NONE, mask=None, name=""):
    a, b = _ref_lin(g, kind, 3.0, mask), _ref_lin(g, kind, 3.0, mask, LD)
    d = opt.linearize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], mask, robust=_robust(capi, kind))
    bad = []
    for k in OUTS:
        scale = float(np.abs(a[k].astype(LD) - b[k]).max())
        if k == "cost":
            # one number, so one sample of the rounding: where the terms' errors happen to cancel in float64 the difference
            # says nothing about the formula.  A sum is no more exact than its least exact term: at least the terms' scale.
            scale = max(scale, float(np.abs(a["rho"].astype(LD) - b["rho"]).max()))
        tol = max(8.0 * scale, 4.0 * np.finfo(np.float64).eps * float(np.abs(a[k]).max()))
        err = float(np.abs(np.asarray(d[k]) - a[k]).max())
        print(f"pgo linearize {name:10s} {k:6s} scale {scale:.2e} tol {tol:.2e} device-vs-ref {err:.2e}")
        if not err <= tol:
            bad.append((k, err, tol))
    assert not bad, bad


def test_linearize_one_edge(opt, capi):
    g = G.graph(2, 0, seed=1, noise=1.0, loop=False)
    assert len(g["src"]) == 1
    _check_lin(opt, capi, g, name="pair")


def test_linearize_loop_with_a_reversed_and_a_duplicated_edge(opt, capi):
    _check_lin(opt, capi, G.loop5(), name="loop5")


@pytest.mark.parametrize("degree", [1, 63, 64, 65, 300])
def test_linearize_hub(opt, capi, degree):
    """The hub's row: below, at and above one round of the wave, and five rounds."""
    _check_lin(opt, capi, G.hub(degree, seed=degree), name=f"hub{degree}")


def test_linearize_block_boundaries_a_fixed_node_in_the_middle_and_an_edgeless_node(opt, capi):
    g = G.n257()
    _check_lin(opt, capi, g, name="n257")
    d = opt.linearize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"])
    assert not d["g"][256].any() and not d["Hdiag"][256].any()


@pytest.mark.parametrize("kind", [R.HUBER, R.CAUCHY, R.TUKEY, R.GEMAN_MCCLURE])
def test_linearize_every_robust_kind_with_a_mask(opt, capi, kind):
    g, mask = G.robust_case()
    _check_lin(opt, capi, g, kind, mask, name=f"robust{kind}")
    d = opt.linearize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], mask, robust=_robust(capi, kind))
    assert (d["weight"][g["odo"]] == 1.0).all() and (d["weight"][~g["odo"]] < 1.0).any()


# ---- optimise ----------------------------------------------------------------------------------------------------------
TIGHT = dict(max_iters=20, rot_eps=0.0, trans_eps=0.0, grad_eps=0.0, pcg_tol=1e-10, pcg_max_iters=400)
# the reference's dense solve against its own PCG at TIGHT: max |pose entry difference|, measured on the CPU
DENSE_VS_PCG = {"plain": 1.19e-10, "cauchy": 1.95e-9}
NOISY = {"plain": (R.NONE, 0.0, 21), "cauchy": (R.CAUCHY, 0.2, 24)}


def _noisy(which):
    kind, outliers, seed = NOISY[which]
    g = G.graph(30, 10, seed=seed, noise=1.0, outliers=outliers)
    return g, kind, (~g["odo"]).astype(np.uint8)


@pytest.fixture(scope="module")
def dense(request):
    """The reference's dense Levenberg-Marquardt on the two noisy graphs, computed once."""
    out = {}
    for which in NOISY:
        g, kind, mask = _noisy(which)
        out[which] = R.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], mask, kind, 3.0, solver="dense", **TIGHT)
    return out


def _run(opt, capi, g, kind=R.NONE, mask=None, init=None, **over):
    return opt.optimize(g["init"] if init is None else init, g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], mask,
                        capi.default_pgo_params(**over), _robust(capi, kind))


@pytest.mark.parametrize("which", ["plain", "cauchy"])
def test_optimize_agrees_with_the_dense_reference(opt, capi, dense, which):
    g, kind, mask = _noisy(which)
    P, s2, w, res = _run(opt, capi, g, kind, mask, **TIGHT)
    err = float(np.abs(P - dense[which]["poses"]).max())
    print(f"pgo optimize {which}: device-vs-dense {err:.3e} allowed {10 * DENSE_VS_PCG[which]:.3e} cost {res.cost_final!r} dense {dense[which]['cost_final']!r} "
          f"accepted {res.accepted} pcg {res.pcg_iters}")
    assert err <= 10 * DENSE_VS_PCG[which]


@pytest.mark.parametrize("which", ["plain", "cauchy"])
def test_optimize_is_stationary_by_the_reference(opt, capi, which):
    g, kind, mask = _noisy(which)
    eps = 1e-3 if kind else 1e-6
    P, s2, w, res = _run(opt, capi, g, kind, mask, max_iters=50, grad_eps=eps, rot_eps=0.0, trans_eps=0.0)
    at = dict(g, init=P)
    a, b = _ref_lin(at, kind, 3.0, mask), _ref_lin(at, kind, 3.0, mask, LD)
    free = R.free_nodes(g["fixed"], g["src"], g["tgt"], len(P))
    ginf = float(np.abs(a["g"][free]).max())
    scale = max(float(abs(a["cost"].astype(LD) - b["cost"])), float(np.abs(a["rho"].astype(LD) - b["rho"]).max()))     # as _check_lin
    tol = max(8.0 * scale, 4.0 * np.finfo(np.float64).eps * float(a["cost"]))
    print(f"pgo stationarity {which}: status {res.status} device ginf {res.grad_inf:.3e} reference ginf {ginf:.3e} cost diff {abs(float(a['cost']) - res.cost_final):.2e} tol {tol:.2e}")
    assert res.status == 3 and res.grad_inf <= eps
    assert ginf <= eps
    assert abs(float(a["cost"]) - res.cost_final) <= tol
    assert res.cost_final < res.cost_initial


def test_optimize_recovers_a_consistent_loop(opt, capi):
    """1025 nodes, 40 closures, Z cut from the truth (rounded to float32), a drifted start.  What is left is Z's float32
    rounding carried round the loop: 6e-8 rad per edge x sqrt(1025) edges x a 330-m lever arm ~ 1e-3 m.  The block-Jacobi
    PCG needs thousands of iterations per step on a loop this long (the reference: 71 242 over 15 steps), so its cap is
    raised: at the default 200 every solve is cut short and 30 steps leave 45 m."""
    g = G.graph(1025, 40, seed=31)
    e0 = G.rel_error(g["init"], g["truth"])
    P, s2, w, res = _run(opt, capi, g, max_iters=30, pcg_max_iters=8000, rot_eps=1e-8, trans_eps=1e-7, grad_eps=1e-4)
    er, et = G.rel_error(P, g["truth"])
    print(f"pgo loop1025: start {e0} end {(er, et)} status {res.status} iters {res.iters} accepted {res.accepted} pcg {res.pcg_iters} cost {res.cost_initial:.3e} -> {res.cost_final:.3e}")
    assert e0[1] > 0.5 and er < 2e-5 and et < 5e-3
    assert res.cost_final < 1e-6 * res.cost_initial


def test_optimize_returns_fixed_and_edgeless_nodes_bit_for_bit(opt, capi):
    g = G.graph(12, 3, seed=5, noise=1.0)
    init = np.concatenate([g["init"], [G.se3([0.1, 0.2, 0.3], [1.0, 2.0, 3.0])]])
    g["fixed"] = np.append(g["fixed"], 0).astype(np.uint8)
    g["fixed"][6] = 1
    P, _, _, res = _run(opt, capi, g, init=init)
    for k in (0, 6, 12):
        assert P[k].tobytes() == init[k].tobytes()
    assert res.accepted > 0 and not np.array_equal(P[3], init[3])
    g["fixed"][:] = 1
    P, _, _, res = _run(opt, capi, g, init=init)
    assert (res.status, res.iters, res.pcg_iters) == (2, 0, 0) and P.tobytes() == init.tobytes() and res.cost_final == res.cost_initial


def test_optimize_a_component_without_a_fixed_node(opt, capi):
    a, b = G.graph(8, 2, seed=8), G.graph(6, 2, seed=9)                            # b hangs free: consistent, drifted
    n = len(a["init"])
    g = dict(init=np.concatenate([a["init"], b["init"]]), fixed=np.concatenate([a["fixed"], np.zeros(6, np.uint8)]),
             src=np.concatenate([a["src"], b["src"] + n]).astype(np.uint32), tgt=np.concatenate([a["tgt"], b["tgt"] + n]).astype(np.uint32),
             Z=np.concatenate([a["Z"], b["Z"]]), info=np.concatenate([a["info"], b["info"]]))
    P, s2, w, res = _run(opt, capi, g, max_iters=50)
    assert np.isfinite(P).all() and res.status in (1, 3)
    er, et = G.rel_error(P[n:], b["truth"])
    print(f"pgo free component: status {res.status} rel err {(er, et)} s2 max {s2.max():.2e}")
    assert er < 1e-5 and et < 1e-4 and s2.max() < 1e-6                             # (float32 Z: as the CPU test of the reference)


def test_optimize_twice_gives_the_same_bits(opt, capi):
    g, kind, mask = _noisy("cauchy")
    one, two = _run(opt, capi, g, kind, mask), _run(opt, capi, g, kind, mask)
    for x, y in zip(one[:3], two[:3]):
        assert x.tobytes() == y.tobytes()
    assert bytes(one[3]) == bytes(two[3])
    h = G.hub(300, seed=300)
    assert _run(opt, capi, h)[0].tobytes() == _run(opt, capi, h)[0].tobytes()


def test_cauchy_switches_the_outlier_closures_off(opt, capi, dense):
    g, kind, mask = _noisy("cauchy")
    inl = (~g["odo"]) & (~g["outlier"])
    wr = dense["cauchy"]["weight"]
    assert g["outlier"].sum() >= 2 and wr[g["outlier"]].max() < 0.1 and wr[inl].min() > 0.5      # the reference shows it on this seed
    _, s2, w, res = _run(opt, capi, g, kind, mask, **TIGHT)
    print(f"pgo cauchy weights: outliers {w[g['outlier']]} inlier closures min {w[inl].min():.3f}")
    assert w[g["outlier"]].max() < 0.1 and w[inl].min() > 0.5 and (w[g["odo"]] == 1.0).all()


@pytest.mark.parametrize("which", ["plain", "cauchy"])
def test_the_translation_offset_does_not_matter(opt, capi, which):
    g, kind, mask = _noisy(which)
    shift = np.array([4000.0, -3000.0, 50.0])
    far = g["init"].copy()
    far[:, :3, 3] += shift
    P, _, _, _ = _run(opt, capi, g, kind, mask, **TIGHT)
    Q, _, _, _ = _run(opt, capi, g, kind, mask, init=far, **TIGHT)
    Q[:, :3, 3] -= shift
    err = float(np.abs(P - Q).max())
    print(f"pgo offset {which}: {err:.3e} allowed {10 * DENSE_VS_PCG[which]:.3e}")
    assert err <= 10 * DENSE_VS_PCG[which]
