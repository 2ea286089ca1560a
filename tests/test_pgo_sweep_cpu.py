"""CPU: what tests/test_pgo_sweep_gpu.py takes for granted, shown on the reference (tests/pgo_ref.py) alone -- that a tiled
graph is the base's computation K times over, that the cases reach the branches they are named after, that the counts the
GPU tests compare exactly (attempts, accepted steps, PCG iterations, the status) are decided with a margin no rounding
closes, and that the recorded dense-versus-PCG disagreements (pgo_cases.RECORDED) are what the reference gives."""
import numpy as np
import pytest

import pgo_cases as G
import pgo_ref as R
from test_pgo_gpu import TIGHT, DENSE_VS_PCG

LD = np.longdouble
LIB = dict(rot_eps=1e-6, trans_eps=1e-6, grad_eps=1e-6)     # gloc_pgo_default_params where pgo_ref.DEFAULTS is tighter


def _opt(g, solver="pcg", mask=None, kind=R.NONE, trace=None, **over):
    return R.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], mask, kind, 3.0, solver=solver, trace=trace, **dict(LIB, **over))


def _lin(g, kind=R.NONE, mask=None, dt=np.float64):
    return R.linearize(g["init"], g["fixed"], g["src"].astype(np.int64), g["tgt"].astype(np.int64), g["Z"], g["info"], mask, kind, 3.0, dt)


def _lm_margins(tr, over=None):
    """(the smallest |gain|, the factor by which the last accepted step passes its stop test, the smallest factor by which
    an earlier accepted step fails both stop tests) at the library's default eps (or over's)."""
    p = dict(LIB, **(over or {}))
    ok = [s for s in tr if s["accepted"]]
    step = lambda s: max(s["max_w"] / p["rot_eps"], s["max_v"] / p["trans_eps"])      # <= 1: status 1
    grad = lambda s: s["grad_inf"] / p["grad_eps"] if p["grad_eps"] > 0 else np.inf   # <= 1: status 3
    fails = min([min(step(s), grad(s)) for s in ok[:-1]] or [np.inf])
    return min(abs(s["gain"]) for s in tr), step(ok[-1]), grad(ok[-1]), fails


# ---- A. tiled graphs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["blocks", "interleaved"])
def test_tiled_is_the_base_computation_k_times(layout):
    g, K = G.base16(), 3
    n0, m0 = len(g["init"]), len(g["src"])
    t = G.tiled(g, K, layout)
    assert len(t["init"]) == K * n0 and len(t["src"]) == K * m0 and t["src"].dtype == np.uint32
    node = (lambda k, c: c * n0 + k) if layout == "blocks" else (lambda k, c: k * K + c)
    edge = (lambda e, c: c * m0 + e) if layout == "blocks" else (lambda e, c: e * K + c)
    for c in range(K):
        for e in range(m0):
            q = edge(e, c)
            assert t["src"][q] == node(g["src"][e], c) and t["tgt"][q] == node(g["tgt"][e], c)
            assert t["Z"][q].tobytes() == g["Z"][e].tobytes() and t["info"][q].tobytes() == g["info"][e].tobytes()
        for k in range(n0):
            assert t["init"][node(k, c)].tobytes() == g["init"][k].tobytes() and t["fixed"][node(k, c)] == g["fixed"][k]
            # a node's incident edges in ascending index are the base's, copy by copy (G3's summation order)
            inc = [q for q in range(K * m0) if t["src"][q] == node(k, c) or t["tgt"][q] == node(k, c)]
            assert inc == [edge(e, c) for e in range(m0) if g["src"][e] == k or g["tgt"][e] == k]
    first = int(np.flatnonzero(t["fixed"])[0])
    assert first == node(int(np.flatnonzero(g["fixed"])[0]), 0)                      # the origin is copy 0's
    a, b = _lin(g), _lin(t)
    for x, y in ((a.r, b.r), (a.s2, b.s2), (a.w, b.w), (a.g, b.g), (a.Hd, b.Hd)):
        v = G.copies(y, K, layout)
        assert all(v[c].tobytes() == x.tobytes() for c in range(K))


def test_tiled_sizes_cross_the_grid_caps():
    """wave-per-node launches: 1024 work-groups x 4 waves = 4096 nodes a round; lane-per-node and lane-per-edge ones:
    262 144; the CSR sort's third pass: n - 1 >= 2^16."""
    n0, m0 = len(G.base30()["init"]), len(G.base30()["src"])
    assert (n0, m0) == (30, 40)
    assert 136 * n0 <= 4096 < 137 * n0 < 4096 + 64 and 2 * 4096 <= 274 * n0 < 2 * 4096 + 64
    g = G.base16()
    n0, m0 = len(g["init"]), len(g["src"])
    assert (n0, m0) == (16, 21)
    assert 16400 * n0 > 262144 and 16400 * m0 > 262144 and 16400 * n0 - 1 >= 1 << 16 and 16400 * n0 <= 1 << 20 and 16400 * m0 <= 1 << 22
    h = G.hub(65, seed=65)
    assert np.bincount(np.concatenate([h["src"], h["tgt"]])).max() == 65             # the hub's row: two rounds of a wave


@pytest.mark.parametrize("m", [21, 40, 40 * 137, 40 * 274, 21 * 16400, 65 * 64])
def test_the_documented_summation_order_stays_within_its_depth(m):
    """sum_depth counted from the documentation: a lane's strided sum (ceil(m / (256 x groups)) additions), the butterfly
    (6), the waves (3), and over the partials ceil(groups / 256) + 6 + 3 more -- d = 20 up to m = 65 536, 24 at
    m = 344 400.  The sum in that order is within d eps sum|x| of the long-double sum."""
    ge = min(-(-m // 256), 1024)
    assert G.sum_depth(m) == -(-m // (ge * 256)) + -(-ge // 256) + 18
    assert G.sum_depth(40 * 274) == 20 and G.sum_depth(21 * 16400) == 24
    x = np.random.default_rng(m).gamma(2.0, 30.0, m)
    assert abs(LD(G.device_order_sum(x)) - x.astype(LD).sum()) <= G.sum_depth(m) * np.finfo(np.float64).eps * x.sum()
    assert G.device_order_sum(np.ones(m)) == m


def test_base16_at_the_default_stops_ends_with_margins():
    """What the K = 16 400 optimise compares exactly: 4 accepted attempts, status 1."""
    tr = []
    b = _opt(G.base16(), trace=tr, max_iters=8)
    gain_min, passes, _, fails = _lm_margins(tr)
    assert (b["status"], b["iters"], b["accepted"]) == (1, 4, 4) and gain_min >= 0.01 and passes <= 0.5 and fails >= 2.0
    a = _opt(G.base16(), "dense", max_iters=8)
    assert (a["status"], a["iters"], a["accepted"]) == (1, 4, 4)


# ---- the recorded reference-versus-reference figures ---------------------------------------------------------------------
def _dense_vs_pcg(g, **over):
    a, b = _opt(g, "dense", **over), _opt(g, "pcg", **over)
    return a, b, float(np.abs(a["poses"] - b["poses"]).max())


@pytest.mark.parametrize("name", sorted(G.RECORDED))
def test_recorded_dense_versus_pcg(name):
    """Each figure in pgo_cases.RECORDED is the reference's own disagreement, rounded up: not above it by more than 2 x."""
    g, over = G.recorded_case(name)
    a, b, d = _dense_vs_pcg(g, **(TIGHT if over is None else over))
    print(f"dense-vs-PCG {name}: {d:.3e} recorded {G.RECORDED[name]:.3e}")
    assert G.RECORDED[name] / 2 <= d <= G.RECORDED[name]
    if name == "base30":
        assert G.RECORDED[name] == DENSE_VS_PCG["plain"]


# ---- B. rejected steps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,counts,pattern", [("rejecting", (13, 9, 1), "ArrrrAAAAAAAA"), ("rejecting_twice", (21, 14, 1), "rrrrrrAAAArAAAAAAAAAA")])
def test_rejecting_cases_have_margins_for_exact_counts(name, counts, pattern):
    """rejecting: an accepted step, then four rejected in a row (the trial set is the one the run started in).
    rejecting_twice: a rejection after accepted steps after rejections, where lambda x 2 shows that nu went back to 2."""
    g, over = G.recorded_case(name)
    tr = []
    b, a = _opt(g, "pcg", trace=tr, **over), _opt(g, "dense", **over)
    acc = [s["accepted"] for s in tr]
    gain_min, passes, _, fails = _lm_margins(tr)
    print(f"{name}: attempts {b['iters']} accepted {b['accepted']} status {b['status']} gains {[round(s['gain'], 3) for s in tr]} "
          f"final passes x{1 / passes:.1f} earlier fail x{fails:.1f} lambda pcg {b['lam']!r} dense {a['lam']!r}")
    assert (b["iters"], b["accepted"], b["status"]) == counts == (a["iters"], a["accepted"], a["status"])
    assert "".join("A" if x else "r" for x in acc) == pattern
    assert acc.count(False) >= 3 and acc[-1] and "rr" in pattern                             # rejections (nu doubled), accepted again
    assert gain_min >= 0.01
    assert passes <= 0.5 and fails >= 2.0
    assert not any(s["pcg"]["breakdown"] for s in tr)
    rel = abs(a["lam"] - b["lam"]) / a["lam"]
    assert G.REJECTING_LAMBDA_REL[name] / 2 <= rel <= G.REJECTING_LAMBDA_REL[name]
    if name == "rejecting_twice":                                                             # nu = 2 at the late rejection
        k = pattern.rindex("r")
        assert tr[k + 1]["lam"] == 2.0 * tr[k]["lam"]


# ---- C. stops and counters ---------------------------------------------------------------------------------------------------
def test_attempt_cap_gives_status_0():
    b = _opt(G.base30(), max_iters=1)
    assert (b["status"], b["iters"]) == (0, 1)


@pytest.mark.parametrize("cap,attempts", [(3, 4), (17, 3)])
def test_pcg_cap_counts_are_exact_without_a_breakdown(cap, attempts):
    tr = []
    b = _opt(G.base30(), trace=tr, pcg_max_iters=cap, pcg_tol=1e-30, max_iters=attempts)
    assert not any(s["pcg"]["breakdown"] for s in tr)
    assert (b["status"], b["iters"], b["pcg_iters"]) == (0, attempts, attempts * cap)
    assert min(abs(s["gain"]) for s in tr) >= 0.01


def test_a_pcg_stop_inside_a_chunk_with_a_margin():
    """The issue's base (graph(30, 10, seed=21)) does not have the margin it asks for: at pcg_tol 3e-2, 1e-2, 3e-3 the
    worst rr / (tol^2 g2) at a stop is 0.92, 0.989, 0.91, and none of 121 tolerances from 1e-1 to 1e-4 has a factor 1.5 in
    every solve (block-Jacobi PCG on a loop lowers rr by a few per cent an iteration).  On a hub the PCG converges in a
    dozen iterations, rr falls several-fold in each: hub(65) at 3e-3 has a factor 2.39 at every stop and before it."""
    g, tol = G.hub(65, seed=65), G.PCG_STOP_TOL
    tr = []
    b = _opt(g, trace=tr, pcg_tol=tol)
    its, worst = [], np.inf
    for s in tr:
        h = s["pcg"]
        q = np.array(h["rr"]) / (tol * tol * h["g2"])
        its.append(len(q) - 1)
        worst = min(worst, 1.0 / q[-1], q[-2])
        assert not h["breakdown"] and q[-1] <= 0.5 and q[-2] >= 2.0
    gain_min, passes, grad, fails = _lm_margins(tr)
    print(f"pcg stop: iterations {its} worst factor {worst:.2f} status {b['status']} final step x{passes:.3g} grad x{grad:.3g} earlier fail x{fails:.3g}")
    assert all(k % 16 for k in its)                                                     # every stop inside a chunk of 16
    assert (b["status"], b["iters"], b["pcg_iters"]) == (3, 6, 69) and sum(its) == b["pcg_iters"]
    # (the last accepted step passes the gradient test by 9 x and misses the step test by 1.1 x: the status, 3 here, has
    # no factor 2, but both tests follow the same step, so the counts do not depend on which of them fires)
    assert gain_min >= 0.01 and fails >= 2.0 and min(passes, grad) <= 0.5


def test_step_stop_alone_gives_status_1():
    tr = []
    over = dict(grad_eps=0.0, rot_eps=1e-5, trans_eps=1e-5)
    b = _opt(G.base30(), trace=tr, **over)
    gain_min, passes, _, fails = _lm_margins(tr, over)
    assert b["status"] == 1 and passes <= 0.5 and fails >= 2.0 and gain_min >= 0.01
    assert (b["iters"], b["accepted"]) == (4, 4)


def test_a_leaf_of_zero_information_fails_the_pivot_rule():
    g = G.with_a_leaf_of_zero_information()
    L = _lin(g)
    assert not L.Hd[30].any() and R.chol6(L.Hd[30]) is None
    assert all(R.chol6(L.Hd[k]) is not None for k in range(1, 30))
    b = _opt(g)
    assert (b["status"], b["iters"], b["accepted"], b["pcg_iters"]) == (2, 1, 0, 0) and b["cost_final"] == b["cost_initial"]
    assert np.array_equal(b["poses"][:, :3, :3], g["init"][:, :3, :3]) and np.abs(b["poses"] - g["init"]).max() < 1e-13


def test_beyond_tukeys_cutoff_every_weight_is_zero():
    g = G.beyond_tukey()
    L = _lin(g, R.TUKEY)
    assert len(g["src"]) == 40 and L.s2.min() > 2 * 9.0
    assert not L.w.any() and not L.g.any() and not L.Hd.any() and float(L.F) == 120.0
    b = _opt(g, kind=R.TUKEY)
    assert (b["status"], b["iters"], b["cost_final"]) == (3, 0, 120.0)
    assert np.array_equal(b["poses"][:, :3, :3], g["init"][:, :3, :3])
    b = _opt(g, kind=R.TUKEY, grad_eps=0.0)
    assert (b["status"], b["iters"], b["accepted"], b["cost_final"]) == (2, 1, 0, 120.0)


# ---- D. residual branches ------------------------------------------------------------------------------------------------------
def _rot(L):
    return np.linalg.norm(L.r[:, :3], axis=1)


def test_exact_graph_has_a_zero_residual():
    g = G.exact()
    assert np.array_equal(g["Z"].astype(np.float64), np.round(g["Z"])) and np.abs(g["init"]).max() <= 6
    for dt in (np.float64, LD):
        L = _lin(g, dt=dt)
        assert not L.r.any() and not L.g.any() and not L.s2.any() and L.Hd[1:].any()


@pytest.mark.parametrize("theta,below,above", [(3e-9, 1e-8, None), (3e-8, 1e-6, 1e-8), (3e-7, 1e-6, 1e-8), (3e-6, None, 1e-6)])
def test_turned_graphs_straddle_the_series_thresholds(theta, below, above):
    """|v| < 1e-8 in the logarithm, theta < 1e-6 in Jl^-1: 3e-9 lies below both, 3e-8 has edges either side of the first,
    3e-7 lies between them, 3e-6 has edges either side of the second."""
    th = _rot(_lin(G.turned(G.exact(), theta)))
    assert th.min() > 0
    if below is not None:
        assert (th < below).any() and (theta not in (3e-9, 3e-7) or (th < below).all())
    if above is not None:
        assert (th > above).any() and (theta != 3e-7 or (th > above).all())
    if theta == 3e-8:
        assert (th < 1e-8).any()
    if theta == 3e-6:
        assert (th < 1e-6).any()


@pytest.mark.parametrize("theta", [1.6, 2.5, 3.0])
def test_large_rotations_reach_the_negative_cosine_quadrant(theta):
    for g, edges in ((G.large_pair(theta), 1), (G.large_loop5(theta), 3)):
        L = _lin(g)
        big = np.abs(_rot(L) - theta) < (1e-6 if edges == 1 else 0.05)                  # (Z is float32; loop5's Z is noisy)
        assert big.sum() == edges and np.cos(_rot(L)[big]).max() < 0


def test_translation_only_case_retracts_at_theta_zero():
    g = G.translation_only()
    L = _lin(g)
    assert not L.r[:, :3].any() and np.abs(L.r[:, 3:]).max() >= 1.0 and not L.g[7:].any()
    free = R.free_nodes(g["fixed"], g["src"], g["tgt"], 14)
    assert free[8:].all() and free[1:7].all()
    for solver in ("dense", "pcg"):
        b = _opt(g, solver, **TIGHT)
        assert b["accepted"] >= 3 and b["cost_final"] < 1e-20 * b["cost_initial"]
        assert b["poses"][7:].tobytes() == g["init"][7:].tobytes()                       # x = 0 exactly: exp(0) = I exactly
        for k in range(14):
            Rk = b["poses"][k, :3, :3]
            assert np.abs(Rk @ Rk.T - np.eye(3)).max() <= 4 * np.finfo(np.float64).eps


# ---- E. small items ------------------------------------------------------------------------------------------------------------
def test_last_fixed_cases_have_a_late_origin():
    g = G.last_fixed_257()
    assert np.flatnonzero(g["fixed"]).tolist() == [255] and np.array_equal(R.origin_of(g["init"], g["fixed"]), g["init"][255, :3, 3])
    g = G.last_fixed_30()
    assert np.flatnonzero(g["fixed"]).tolist() == [29] and np.linalg.norm(R.origin_of(g["init"], g["fixed"])) > 4000.0


def test_mask_and_kind_on_the_reference():
    g, mask = G.robust_case()
    a, b = _lin(g, R.NONE, None), _lin(g, R.NONE, mask)
    assert a.w.tobytes() == b.w.tobytes() and a.g.tobytes() == b.g.tobytes() and float(a.F) == float(b.F)
    a, b = _lin(g, R.CAUCHY, None), _lin(g, R.CAUCHY, np.ones(len(mask), np.uint8))
    assert a.w.tobytes() == b.w.tobytes() and a.g.tobytes() == b.g.tobytes() and (a.w < 1).all()
