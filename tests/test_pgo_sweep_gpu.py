"""GPU: the pose-graph optimisation (gloc_pgo_*) where tests/test_pgo_gpu.py does not reach -- grids that stride, rejected
Levenberg-Marquardt steps, every stop and counter, the residual's series and negative-cosine branches, a late origin.
tests/pgo_ref.py is the contract and tests/test_pgo_sweep_cpu.py shows on the reference alone what is taken for granted
here (margins behind every count compared exactly, the branches each case reaches, the recorded figures).

Tiled graphs (A).  pgo_cases.tiled makes K copies of a base graph with identical pose values.  Per-edge and per-node work
is a function of its operands and the PCG's scalars are global, so every copy's outputs equal copy 0's BIT FOR BIT whatever
round of a strided launch the copy falls in, and copy 0 is held to the reference on the base graph alone.  Only the
objective is a sum in another order: it is allowed d eps sum(rho) + 8 (the base's rho scale) m, d = pgo_cases.sum_depth(m)
counted from the order G9 and DESIGN.md section 14 document -- a lane's strided sum, ceil(m / (256 x min(ceil(m / 256),
1024))) additions; the butterfly, 6; the four waves, 3; and over the at most 1024 partials ceil(groups / 256) + 6 + 3 more:
d = 20 for every m <= 65 536 here and 24 at m = 344 400.

Linearise: test_pgo_gpu._check_lin's rule (8 x |float64 - longdouble| of the reference per output, floor 4 ulp).  Scales
of the new cases, max over the output of |float64 - longdouble| (recomputed by the tests; DESIGN.md section 14 has the
same table):
    case              r        s2       weight   g        Hdiag    cost     rho
    base30            4.2e-15  1.3e-12  0        1.5e-10  4.2e-10  2.7e-12  1.3e-12
    base16            2.4e-15  1.6e-12  0        4.3e-11  7.9e-11  3.9e-13  1.6e-12
    hub65             8.0e-15  1.2e-11  0        2.4e-09  4.0e-08  2.2e-11  1.2e-11
    exact             0        0        0        0        6.5e-11  0        0
    turned 3e-9       8.5e-16  4.9e-20  0        2.1e-11  1.3e-10  2.5e-20  4.9e-20
    turned 3e-8       1.2e-15  8.9e-19  0        4.4e-11  1.1e-10  1.2e-18  8.9e-19
    turned 3e-7       1.2e-15  2.3e-18  0        5.3e-11  5.9e-11  4.8e-18  2.3e-18
    turned 3e-6       1.5e-15  1.6e-16  0        6.5e-11  1.2e-10  2.2e-16  1.6e-16
    pair 1.6 rad      7.6e-16  1.5e-11  0        4.1e-12  1.1e-11  1.5e-11  1.5e-11
    pair 2.5 rad      3.4e-16  6.7e-11  0        2.9e-11  1.8e-11  6.7e-11  6.7e-11
    pair 3.0 rad      1.4e-15  3.1e-11  0        9.5e-11  5.2e-11  3.1e-11  3.1e-11
    loop5 1.6 rad     6.8e-16  1.5e-11  0        3.2e-11  4.9e-11  8.6e-12  1.5e-11
    loop5 2.5 rad     4.5e-16  1.1e-10  0        1.1e-10  6.4e-11  3.6e-10  1.1e-10
    loop5 3.0 rad     1.2e-15  9.7e-11  0        1.5e-10  1.1e-10  4.5e-11  9.7e-11
    last_fixed_257    1.0e-13  2.1e-09  0        2.8e-08  2.0e-07  4.9e-09  2.1e-09

Optimise: the poses agree with the reference's DENSE run to 10 x the disagreement of the reference's own dense and PCG runs
on the same case at the same stops, pgo_cases.RECORDED (measured on the CPU, re-measured by the CPU file).  Counts
(attempts, accepted steps, PCG iterations, the status) are compared exactly with the reference's PCG run, and only where
the CPU file shows every decision behind them has a factor 2 to spare (gains: |gain| >= 0.01).  No number in this file
comes from the device.
"""
import functools

import numpy as np
import pytest

import pgo_cases as G
import pgo_ref as R
import test_pgo_gpu as T

pytestmark = pytest.mark.gpu

LD, EPS = np.longdouble, float(np.finfo(np.float64).eps)
LIB = dict(rot_eps=1e-6, trans_eps=1e-6, grad_eps=1e-6)     # gloc_pgo_default_params where pgo_ref.DEFAULTS is tighter
BASES = {"base30": G.base30, "base16": G.base16, "hub65": lambda: G.hub(65, seed=65)}


@pytest.fixture(scope="module")
def opt(capi):
    o = capi.PoseGraphOptimizer()
    yield o
    o.close()


def _ref(g, solver, mask=None, kind=R.NONE, **over):
    """The reference at the library's default stops, then `over` (T._run gives the device the same)."""
    return R.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], mask, kind, 3.0, solver=solver, **dict(LIB, **over))


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def _copies_equal(x, K, layout):
    v = _bits(G.copies(x, K, layout))
    return bool((v == v[:1]).all())


@functools.lru_cache(maxsize=None)
def _base(name):
    """The base graph, the reference's float64 linearisation of it and _check_lin's tolerances, computed once."""
    g = BASES[name]()
    a, b = T._ref_lin(g), T._ref_lin(g, dt=LD)
    tol = {k: max(8.0 * float(np.abs(a[k].astype(LD) - b[k]).max()), 4.0 * EPS * float(np.abs(a[k]).max())) for k in T.OUTS if k != "cost"}
    return g, a, tol, b["rho"].sum(dtype=LD), float(np.abs(a["rho"].astype(LD) - b["rho"]).max())


@functools.lru_cache(maxsize=None)
def _tiled(name, K, layout):
    return G.tiled(_base(name)[0], K, layout)


def _lin(o, g, **kw):
    return o.linearize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], **kw)


# ---- A. tiled graphs: the strides -----------------------------------------------------------------------------------------
TILINGS = [("base30", 136, "blocks"), ("base30", 136, "interleaved"),       # n = 4080: every wave-per-node launch in one round
           ("base30", 137, "blocks"), ("base30", 137, "interleaved"),       # n = 4110: a second round of 14 nodes
           ("base30", 274, "blocks"), ("base30", 274, "interleaved"),       # n = 8220: two full rounds and a third of 28
           ("base16", 16400, "blocks"), ("base16", 16400, "interleaved"),   # n = 262 400, m = 344 400: every launch strides, three sort passes
           ("hub65", 64, "interleaved")]                                    # 64 hubs with two-round rows, on as many waves


@pytest.mark.parametrize("name,K,layout", TILINGS)
def test_tiled_linearize(opt, name, K, layout):
    g, a, tol, sum_rho, rho_scale = _base(name)
    t = _tiled(name, K, layout)
    d = _lin(opt, t)
    m = len(t["src"])
    bad = [k for k in ("r", "s2", "weight", "g", "Hdiag") if not _copies_equal(d[k], K, layout)]
    assert not bad, f"copies differ from copy 0 in {bad}"
    for k in ("r", "s2", "weight", "g", "Hdiag"):
        err = float(np.abs(G.copies(d[k], K, layout)[0] - a[k]).max())
        print(f"pgo tiled {name} x{K} {layout:11s} {k:6s} tol {tol[k]:.2e} copy 0 vs ref {err:.2e}")
        if not err <= tol[k]:
            bad.append((k, err, tol[k]))
    depth = G.sum_depth(m)
    cost_tol = float(depth * EPS * K * sum_rho + 8.0 * rho_scale * m)
    err = float(abs(LD(d["cost"]) - K * sum_rho))
    print(f"pgo tiled {name} x{K} {layout:11s} cost   depth {depth} tol {cost_tol:.2e} device vs long-double sum {err:.2e}; "
          f"equals its own s2 in the documented order: {d['cost'] == G.device_order_sum(d['s2'])}")
    assert not bad, bad
    assert err <= cost_tol


def _tiled_optimize(opt, capi, name, K, layout, recorded, **over):
    g = _base(name)[0]
    t = _tiled(name, K, layout)
    dense = _ref(g, "dense", **over)
    P, s2, w, res = T._run(opt, capi, t, **over)
    bad = [k for k, x in (("poses", P), ("s2", s2), ("weight", w)) if not _copies_equal(x, K, layout)]
    err = float(np.abs(G.copies(P, K, layout)[0] - dense["poses"]).max())
    print(f"pgo tiled optimize {name} x{K}: copy 0 vs dense {err:.3e} allowed {10 * recorded:.3e} status {res.status} iters {res.iters} "
          f"accepted {res.accepted} pcg {res.pcg_iters}")
    assert not bad, f"copies differ from copy 0 in {bad}"
    assert err <= 10 * recorded
    return res


def test_tiled_optimize_with_a_second_round_of_waves(opt, capi):
    _tiled_optimize(opt, capi, "base30", 137, "interleaved", G.RECORDED["base30"], **T.TIGHT)


def test_tiled_optimize_with_every_launch_striding(opt, capi):
    """n = 262 400, m = 344 400 at the library's default stops.  The reference ends base16 with status 1 after 4 accepted
    attempts: the last step passes the test by 180 x, the one before fails it by 2.8 x, the gains are 0.83 to 1.0."""
    res = _tiled_optimize(opt, capi, "base16", 16400, "interleaved", G.RECORDED["base16_default8"], max_iters=8)
    ref = _ref(_base("base16")[0], "pcg", max_iters=8)
    assert (res.status, res.iters, res.accepted) == (ref["status"], ref["iters"], ref["accepted"]) == (1, 4, 4)


# ---- B. rejected steps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rejecting", "rejecting_twice"])
def test_rejected_steps_and_the_damping_follow_the_reference(opt, capi, name):
    """rejecting: an accepted step, four rejected in a row (lambda x 2, 4, 8, 16 from the kept linearisation while the
    trial set holds a discarded one), eight accepted: 13 attempts, 9 accepted, status 1.  rejecting_twice: six rejected,
    four accepted, one rejected -- lambda x 2, not x 128: nu went back to 2 --, ten accepted: 21 attempts, 14 accepted."""
    g, over = G.recorded_case(name)
    dense, ref = _ref(g, "dense", **over), _ref(g, "pcg", **over)
    P, s2, w, res = T._run(opt, capi, g, **over)
    err = float(np.abs(P - dense["poses"]).max())
    print(f"pgo {name}: device iters {res.iters} accepted {res.accepted} status {res.status} pcg {res.pcg_iters} lambda {res.lam!r}; reference "
          f"{ref['iters']} {ref['accepted']} {ref['status']} {ref['pcg_iters']} {ref['lam']!r} dense {dense['lam']!r}; poses vs dense {err:.3e}")
    assert ref["iters"] - ref["accepted"] >= 3
    assert (res.iters, res.accepted, res.status) == (ref["iters"], ref["accepted"], ref["status"])
    assert err <= 10 * G.RECORDED[name]
    assert abs(res.lam - dense["lam"]) <= 10 * G.REJECTING_LAMBDA_REL[name] * dense["lam"]


# ---- C. stops and counters -----------------------------------------------------------------------------------------------------
def test_attempt_cap_gives_status_0(opt, capi):
    _, _, _, res = T._run(opt, capi, G.base30(), max_iters=1)
    assert (res.status, res.iters) == (0, 1)


@pytest.mark.parametrize("cap,attempts", [(3, 4), (17, 3)])
def test_pcg_cap_is_counted_exactly(opt, capi, cap, attempts):
    """A cap below a chunk of 16 and one a single iteration past it; pcg_tol = 1e-30 is never met, and the reference shows
    no breakdown, so every solve runs to the cap."""
    _, _, _, res = T._run(opt, capi, G.base30(), pcg_max_iters=cap, pcg_tol=1e-30, max_iters=attempts)
    ref = _ref(G.base30(), "pcg", pcg_max_iters=cap, pcg_tol=1e-30, max_iters=attempts)
    assert (res.status, res.iters, res.pcg_iters) == (0, attempts, attempts * cap) == (ref["status"], ref["iters"], ref["pcg_iters"])


def test_pcg_stops_inside_a_chunk_at_the_reference_iteration(opt, capi):
    """hub(65) at pcg_tol = 3e-3: the reference's six solves stop after 4, 10, 14, 14, 14, 13 iterations, each with
    rr / (tol^2 g2) a factor >= 2.39 from 1 at the stop and before it.  (The issue's graph(30, 10, seed=21) has no
    tolerance with such a margin, see the CPU file.)  The status is 3 in the reference, by a gradient test passed 9 x
    over after a step that misses the step test by 1.1 x: 1 is accepted too, the counts do not depend on it."""
    g = G.hub(65, seed=65)
    _, _, _, res = T._run(opt, capi, g, pcg_tol=G.PCG_STOP_TOL)
    ref = _ref(g, "pcg", pcg_tol=G.PCG_STOP_TOL)
    print(f"pgo pcg stop: device iters {res.iters} pcg {res.pcg_iters} status {res.status}; reference {ref['iters']} {ref['pcg_iters']} {ref['status']}")
    assert (res.iters, res.accepted, res.pcg_iters) == (ref["iters"], ref["accepted"], ref["pcg_iters"]) and res.status in (1, 3)


def test_step_stop_alone_gives_status_1(opt, capi):
    over = dict(grad_eps=0.0, rot_eps=1e-5, trans_eps=1e-5)
    _, _, _, res = T._run(opt, capi, G.base30(), **over)
    ref = _ref(G.base30(), "pcg", **over)
    assert (res.status, res.iters, res.accepted) == (1, ref["iters"], ref["accepted"])


def test_a_leaf_of_zero_information_ends_the_call_by_the_pivot_rule(opt, capi):
    g = G.with_a_leaf_of_zero_information()
    ref = _ref(g, "pcg")
    P, _, _, res = T._run(opt, capi, g)
    assert (res.status, res.iters, res.accepted, res.pcg_iters) == (2, 1, 0, 0) == (ref["status"], ref["iters"], ref["accepted"], ref["pcg_iters"])
    assert res.cost_final == res.cost_initial
    assert P.tobytes() == ref["poses"].tobytes()                                     # (t - origin) + origin in float64 on both sides


def test_every_weight_zero_beyond_tukeys_cutoff(opt, capi):
    g = G.beyond_tukey()
    rob = capi.default_robust_params(kind=R.TUKEY, scale=3.0)
    d = _lin(opt, g, robust=rob)
    assert not d["weight"].any() and not d["g"].any() and not d["Hdiag"].any() and d["cost"] == 120.0
    ref = _ref(g, "pcg", kind=R.TUKEY)
    P, _, w, res = opt.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], None, capi.default_pgo_params(), rob)
    assert (res.status, res.iters, res.cost_initial, res.cost_final) == (3, 0, 120.0, 120.0) and not w.any()
    assert P.tobytes() == ref["poses"].tobytes()
    ref = _ref(g, "pcg", kind=R.TUKEY, grad_eps=0.0)
    P, _, _, res = opt.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], None, capi.default_pgo_params(grad_eps=0.0), rob)
    assert (res.status, res.iters, res.accepted, res.cost_final) == (2, 1, 0, 120.0) == (ref["status"], ref["iters"], ref["accepted"], ref["cost_final"])
    assert P.tobytes() == ref["poses"].tobytes()


# ---- D. residual branches --------------------------------------------------------------------------------------------------------
def test_linearize_a_zero_residual(opt, capi):
    """theta = 0 exactly: the series of the logarithm at |v| = 0 and the 1/12 of Jl^-1."""
    g = G.exact()
    d = _lin(opt, g)
    assert not d["r"][:, :3].any() and not d["g"].any()
    T._check_lin(opt, capi, g, name="exact")


@pytest.mark.parametrize("theta", [3e-9, 3e-8, 3e-7, 3e-6])
def test_linearize_small_rotations_either_side_of_the_series_thresholds(opt, capi, theta):
    T._check_lin(opt, capi, G.turned(G.exact(), theta), name=f"turned{theta:g}")


@pytest.mark.parametrize("theta", [1.6, 2.5, 3.0])
def test_linearize_large_rotations_with_a_negative_cosine(opt, capi, theta):
    T._check_lin(opt, capi, G.large_pair(theta), name=f"pair{theta}")
    T._check_lin(opt, capi, G.large_loop5(theta), name=f"loop5_{theta}")


def test_retraction_at_theta_zero(opt, capi):
    """translation_only(): nodes 8-13 are free with g = 0 exactly, so every step retracts them by x = 0 -- exp(0) = I and
    their (integer-valued) poses come back bit for bit, as the reference's do; nodes 1-6 lose their translation errors."""
    g = G.translation_only()
    dense = _ref(g, "dense", **T.TIGHT)
    P, _, _, res = T._run(opt, capi, g, **T.TIGHT)
    err = float(np.abs(P - dense["poses"]).max())
    orth = max(float(np.abs(P[k, :3, :3] @ P[k, :3, :3].T - np.eye(3)).max()) for k in range(14) if not g["fixed"][k])
    print(f"pgo translation only: vs dense {err:.3e} allowed {10 * G.RECORDED['translation_only']:.3e} orthonormality {orth:.2e} accepted {res.accepted}")
    assert res.accepted >= 3 and np.isfinite(P).all()
    assert P[7:].tobytes() == dense["poses"][7:].tobytes() == g["init"][7:].tobytes()
    assert orth <= 4 * EPS
    assert err <= 10 * G.RECORDED["translation_only"]


# ---- E. small items ----------------------------------------------------------------------------------------------------------------
def test_only_the_last_node_fixed(opt, capi):
    """The origin of G4 is node 255 of 257, and node 29 of 30 at 4000 m."""
    T._check_lin(opt, capi, G.last_fixed_257(), name="last257")
    g = G.last_fixed_30()
    dense = _ref(g, "dense", **T.TIGHT)
    P, _, _, res = T._run(opt, capi, g, **T.TIGHT)
    err = float(np.abs(P - dense["poses"]).max())
    print(f"pgo last fixed: vs dense {err:.3e} allowed {10 * G.RECORDED['last_fixed_30']:.3e}")
    assert P[29].tobytes() == g["init"][29].tobytes() and err <= 10 * G.RECORDED["last_fixed_30"]


@pytest.mark.parametrize("name", ["loop5", "hub65", "hub300"])
def test_optimize_agrees_with_the_dense_reference_on_other_topologies(opt, capi, name):
    g, _ = G.recorded_case(name)
    dense = _ref(g, "dense", **T.TIGHT)
    P, _, _, res = T._run(opt, capi, g, **T.TIGHT)
    err = float(np.abs(P - dense["poses"]).max())
    print(f"pgo optimize {name}: device-vs-dense {err:.3e} allowed {10 * G.RECORDED[name]:.3e} accepted {res.accepted} pcg {res.pcg_iters}")
    assert err <= 10 * G.RECORDED[name]


def test_one_handle_after_a_large_graph_answers_as_a_fresh_one(capi):
    big, small, hub = _tiled("base16", 16400, "interleaved"), G.loop5(), G.hub(65, seed=65)

    def outputs(o, which):
        if which == 0:
            d = _lin(o, big)
            return [d[k] for k in ("r", "s2", "weight", "g", "Hdiag")] + [np.array(d["cost"])]
        if which == 1:
            P, s2, w, res = T._run(o, capi, small)
            return [P, s2, w, np.frombuffer(bytes(res), np.uint8)]
        P, s2, w, res = T._run(o, capi, hub)
        d = _lin(o, hub)
        return [P, s2, w, np.frombuffer(bytes(res), np.uint8), d["g"], d["Hdiag"], np.array(d["cost"])]

    one = capi.PoseGraphOptimizer()
    try:
        used = [outputs(one, which) for which in range(3)]
    finally:
        one.close()
    for which in range(3):
        fresh = capi.PoseGraphOptimizer()
        try:
            want = outputs(fresh, which)
        finally:
            fresh.close()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(used[which], want)), which


def test_mask_without_a_kind_and_kind_without_a_mask(opt, capi):
    g, mask = G.robust_case()
    ones = np.ones(len(mask), np.uint8)
    plain = dict(mask=None, robust=None)
    for other in (dict(mask=mask, robust=None), dict(mask=mask, robust=capi.default_robust_params(kind=R.NONE, scale=3.0))):
        a, b = _lin(opt, g, **plain), _lin(opt, g, **other)
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in T.OUTS)
        a = opt.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], None, None, None)
        b = opt.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], other["mask"], None, other["robust"])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and bytes(a[3]) == bytes(b[3])
    rob = capi.default_robust_params(kind=R.CAUCHY, scale=3.0)
    a, b = _lin(opt, g, mask=None, robust=rob), _lin(opt, g, mask=ones, robust=rob)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in T.OUTS) and (a["weight"] < 1.0).all()
    a = opt.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], None, None, rob)
    b = opt.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], ones, None, rob)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and bytes(a[3]) == bytes(b[3])
