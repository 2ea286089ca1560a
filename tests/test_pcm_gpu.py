"""GPU: the pose graph's closure selection (gloc_pgo_consistency) against tests/pcm_ref.py and against closed forms.

Restated cases (pcm_cases.NOISY, L = 65, 130, 258).  Everything that is an integer or a decision -- status, the matrix
(through degree and through out_s2 < chi2 bit for bit), score, seeds, clique sizes, mask, winner, ok -- equals the reference
exactly; tests/test_pcm_cases_cpu.py shows that no pair of these cases is within 1e-6 of the threshold and that the
longdouble evaluation decides the same.  out_s2 is held to the rule of tests/test_pgo_gpu.py: the reference evaluates the
case in float64 and in numpy.longdouble, the largest difference over the finite entries is the formula's rounding scale,
and EVERY entry of the device's matrix is allowed 8 x that, with a floor of 4 ulp of the largest finite entry.  Scales
measured on the reference's own two precisions (the test recomputes them; DESIGN.md section 15 has the same table):
    case            largest finite s2   max |float64 - longdouble|
    n60_undrifted   4.3e5               8.6e-10
    n60_drift0      4.3e5               5.9e-10
    n60_own         5.5e4               7.5e-11
    n120_drift0     3.7e6               5.6e-8
    n120_own        1.5e5               1.8e-10
    n200_drift0     5.7e6               3.3e-7
    n200_own        1.5e5               4.8e-10

The closed-form family (pcm_cases.cliques) has no restatement in between: its expected results follow from its groups.
"""
import numpy as np
import pytest

import pcm_cases as PC
import pcm_ref as M
import pgo_cases as G

pytestmark = pytest.mark.gpu

INTS = ("status", "degree", "score", "seeds", "clique_sizes", "mask")


@pytest.fixture(scope="module")
def opt(capi):
    o = capi.PoseGraphOptimizer()
    yield o
    o.close()


def _run(opt, capi, c, want_s2=False, **over):
    return opt.consistency(c["poses"], c["src"], c["tgt"], c["Z"], c["info"], c.get("path"), capi.default_pgo_consistency_params(**over), want_s2)


def _same(a, b, keys=INTS + ("clique_size", "winner_rank", "ok")):
    return [k for k in keys if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


@pytest.mark.parametrize("name", list(PC.NOISY))
def test_restated_cases(opt, capi, name):
    c, prm = PC.noisy(name)
    a, b = PC.restated(name), PC.restated(name, long=True)
    d = _run(opt, capi, c, want_s2=True, **prm)
    assert not _same(d, dict(a, mask=a["mask"].astype(bool), ok=bool(a["ok"])))
    fin = np.isfinite(a["s2"])
    assert (np.isfinite(d["s2"]) == fin).all() and np.isposinf(d["s2"][~fin]).all()
    assert ((d["s2"] < M.CHI2_99_6) == a["C"]).all() and (d["s2"] == d["s2"].T).all()
    scale = float(np.abs(a["s2"][fin].astype(PC.LD) - b["s2"][fin]).max())
    big = float(a["s2"][fin].max())
    tol = max(8.0 * scale, 4.0 * np.finfo(np.float64).eps * big)
    err = float(np.abs(d["s2"][fin] - a["s2"][fin]).max())
    near = fin & (a["s2"] < 50.0)
    rel = float((np.abs(d["s2"][near] - a["s2"][near]) / a["s2"][near]).max())
    print(f"pcm {name}: L {len(a['mask'])} largest s2 {big:.2e} scale {scale:.2e} tol {tol:.2e} device-vs-ref {err:.2e}; below 50: worst relative {rel:.2e}; "
          f"clique {d['clique_size']} rank {d['winner_rank']}")
    assert err <= tol


# ---- the closed-form family ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [270, 1025, 4097])
def test_groups_of_closures_that_agree_among_themselves(opt, capi, L):
    """270: the groups 130, 65, 64, 5, 3, 2, 1; 1025: a row of 17 words; 4097: 65 words, the streaming branch of the score
    and clique kernels.  Every seed's clique is its group."""
    c = PC.cliques(L)
    e = PC.cliques_expected(c)
    d = _run(opt, capi, c, n_seeds=1024)
    assert (d["status"] == 0).all()
    assert (d["degree"] == e["degree"]).all() and (d["score"] == e["score"]).all()
    key = e["score"].astype(np.int64) + e["degree"]
    assert (d["seeds"] == M.seeds_of(key, 1024)).all()
    live = d["seeds"] != M.NONE
    assert live.sum() == min(L, 1024)
    assert (d["clique_sizes"][live] == c["sizes"][c["group"][d["seeds"][live]]]).all() and (d["clique_sizes"][~live] == 0).all()
    assert d["winner_rank"] == 0 and d["seeds"][0] == e["winner_seed"] and d["clique_size"] == e["clique_size"] and d["ok"]
    assert (d["mask"] == e["mask"].astype(bool)).all()


def test_every_group_is_found_from_its_own_seed(opt, capi):
    """One seed: the winner is the first member of the largest group whatever else there is.  Then the largest group's
    closures are taken out one group at a time: the next group wins."""
    c = PC.cliques()
    keep = np.ones(len(c["group"]), bool)
    for g in range(len(c["sizes"]) - 1):
        sub = {k: (v[keep] if k in ("src", "tgt", "Z", "info", "group") else v) for k, v in c.items()}
        d = _run(opt, capi, sub, n_seeds=1)
        assert d["ok"] == (c["sizes"][g] >= 2) and d["clique_size"] == c["sizes"][g]
        if d["ok"]:
            assert (d["mask"] == (sub["group"] == g)).all()
        keep &= c["group"] != g


# ---- edges ----------------------------------------------------------------------------------------------------------------------
def _dense(L, seed=3):
    """L closures cut from the truth: all mutually consistent."""
    rng = np.random.default_rng(seed)
    truth = G.trajectory(20, rng)
    src = rng.integers(0, 20, L)
    tgt = (src + rng.integers(2, 18, L)) % 20
    Z = np.array([np.linalg.inv(truth[j]) @ truth[i] for i, j in zip(src, tgt)]).astype(np.float32)
    return dict(poses=truth, src=src.astype(np.uint32), tgt=tgt.astype(np.uint32), Z=Z, info=G.random_info(rng, L), path=None)


def _apart(L, seed=4):
    """L closures each off the truth by a motion of its own, metres apart: none consistent with another."""
    c = _dense(L, seed)
    for a in range(L):
        c["Z"][a] = (c["Z"][a].astype(np.float64) @ G.se3([0.0, 0.0, 0.1 * a], [3.0 * (a + 1), 0.0, 0.0])).astype(np.float32)
    return c


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65])
def test_all_consistent_around_the_word(opt, capi, L):
    d = _run(opt, capi, _dense(L), want_s2=True)
    off = ~np.eye(L, dtype=bool)
    assert (d["s2"][off] < 1e-4).all() and np.isposinf(np.diag(d["s2"])).all()
    assert (d["degree"] == L - 1).all() and (d["score"] == (L - 1) * max(L - 2, 0)).all()
    assert (d["seeds"][:min(L, 64)] == np.arange(min(L, 64))).all() and (d["seeds"][L:] == M.NONE).all()
    assert (d["clique_sizes"][:min(L, 64)] == L).all() and (d["clique_sizes"][L:] == 0).all()
    assert d["clique_size"] == L and d["winner_rank"] == 0 and d["ok"] == (L >= 2) and (d["mask"] == (L >= 2)).all()
    if L == 1:                                            # one closure is a clique of one: min_clique 1 accepts it
        d = _run(opt, capi, _dense(L), min_clique=1)
        assert d["ok"] and d["mask"].all() and d["clique_size"] == 1


@pytest.mark.parametrize("L", [2, 64, 65])
def test_none_consistent(opt, capi, L):
    d = _run(opt, capi, _apart(L), want_s2=True)
    assert (d["s2"] > 1e3).all()
    assert (d["degree"] == 0).all() and (d["score"] == 0).all() and (d["seeds"][:min(L, 64)] == np.arange(min(L, 64))).all()
    assert (d["clique_sizes"][:min(L, 64)] == 1).all() and d["clique_size"] == 1 and d["winner_rank"] == 0
    assert not d["ok"] and not d["mask"].any()


def test_a_zero_information_matrix_is_status_1_and_a_zero_row(opt, capi):
    c = _dense(70)
    c["info"][[5, 69]] = 0.0
    d = _run(opt, capi, c, want_s2=True)
    bad = np.zeros(70, bool)
    bad[[5, 69]] = True
    assert (d["status"] == bad).all() and (d["degree"] == np.where(bad, 0, 67)).all()
    assert np.isposinf(d["s2"][bad]).all() and np.isposinf(d["s2"][:, bad]).all()
    assert d["clique_size"] == 68 and (d["mask"] == ~bad).all()


def test_duplicate_closures_are_consistent_with_each_other(opt, capi):
    c = _apart(6)
    for k in ("src", "tgt", "Z", "info"):
        c[k] = np.concatenate([c[k], c[k][[2, 2, 4]]])
    d = _run(opt, capi, c)
    assert list(d["degree"]) == [0, 0, 2, 0, 1, 0, 2, 2, 1] and list(d["score"]) == [0, 0, 2, 0, 0, 0, 2, 2, 0]
    assert list(d["seeds"][:4]) == [2, 6, 7, 4] and d["clique_size"] == 3 and list(np.flatnonzero(d["mask"])) == [2, 6, 7]


@pytest.mark.parametrize("n_seeds", [1, 65, 1024])
def test_seed_counts(opt, capi, n_seeds):
    c, prm = PC.noisy("n120_own")
    a = PC.restated("n120_own")
    r = M.select(a["C"], n_seeds=n_seeds)
    d = _run(opt, capi, c, n_seeds=n_seeds, **prm)
    assert len(d["seeds"]) == n_seeds and not _same(d, dict(r, status=a["status"], mask=r["mask"].astype(bool), ok=bool(r["ok"])))


def test_min_clique_above_the_winner(opt, capi):
    c, prm = PC.noisy("n60_own")
    a = PC.restated("n60_own")
    d = _run(opt, capi, c, min_clique=a["clique_size"] + 1, **prm)
    assert not d["ok"] and not d["mask"].any() and d["clique_size"] == a["clique_size"] and d["winner_rank"] == a["winner_rank"]
    d = _run(opt, capi, c, min_clique=a["clique_size"], **prm)
    assert d["ok"] and (d["mask"] == a["mask"].astype(bool)).all()


def test_a_null_path_is_all_zeros_and_two_calls_give_the_same_bits(opt, capi):
    c, _ = PC.noisy("n120_own")
    prm = dict(drift_rot=0.01, drift_trans=0.1)
    one = _run(opt, capi, dict(c, path=None), want_s2=True, **prm)
    two = _run(opt, capi, dict(c, path=np.zeros(len(c["poses"]))), want_s2=True, **prm)
    three = _run(opt, capi, c, want_s2=True, **prm)
    again = _run(opt, capi, c, want_s2=True, **prm)
    for k in INTS + ("s2",):
        assert one[k].tobytes() == two[k].tobytes(), k
        assert three[k].tobytes() == again[k].tobytes(), k
    assert three["s2"].tobytes() != one["s2"].tobytes()                  # (the drift term is in: the path matters)


def test_the_optimiser_is_undisturbed_on_the_same_handle(opt, capi):
    g = G.graph(30, 10, seed=24, noise=1.0, outliers=0.2)
    mask = (~g["odo"]).astype(np.uint8)
    rob = capi.default_robust_params(kind=2, scale=3.0)
    run = lambda: opt.optimize(g["init"], g["fixed"], g["src"], g["tgt"], g["Z"], g["info"], mask, capi.default_pgo_params(), rob)
    one = run()
    c = PC.closures_of(g)
    d = _run(opt, capi, c)
    two = run()
    for x, y in zip(one[:3], two[:3]):
        assert x.tobytes() == y.tobytes()
    assert bytes(one[3]) == bytes(two[3])
    assert _run(opt, capi, c)["mask"].tobytes() == d["mask"].tobytes()


# ---- PoseGraph.select_consistent ------------------------------------------------------------------------------------------
def test_select_consistent_keeps_no_outlier_and_helps_the_optimiser(capi):
    """robust_case()'s recipe (noise, 40 % gross-outlier closures) on 40 nodes at an undrifted start: the kept set has no
    outlier, and the optimisation after the selection ends nearer the truth than the one without it."""
    from gloc3d_amd.pose_graph import PoseGraph
    g = G.graph(40, 30, seed=6, noise=1.0, outliers=0.4, drift=(0, 0))
    assert g["outlier"].sum() >= 5

    def build():
        pg = PoseGraph()
        for k, T in enumerate(g["init"]):
            pg.add_node(T, fixed=bool(g["fixed"][k]))
        for e in range(len(g["src"])):
            pg.add_edge(int(g["src"][e]), int(g["tgt"][e]), g["Z"][e], g["info"][e], robust=not g["odo"][e])
        return pg

    plain = build()
    P0, _, _ = plain.optimize()
    plain.close()
    pg = build()
    closures = np.flatnonzero(~g["odo"])
    dry = pg.select_consistent(apply=False)
    assert pg.n_edges == len(g["src"]) and len(dry) >= 2 and not g["outlier"][dry].any() and set(dry) <= set(closures)
    kept = pg.select_consistent()
    assert len(kept) == len(dry) and pg.n_edges == int(g["odo"].sum()) + len(kept)
    assert all(pg.robust[e] for e in kept) and sum(pg.robust) == len(kept)
    assert [(pg.src[e], pg.tgt[e]) for e in kept] == [(int(g["src"][e]), int(g["tgt"][e])) for e in dry]
    P1, _, _ = pg.optimize()
    pg.close()
    e0, e1 = G.rel_error(P0, g["truth"]), G.rel_error(P1, g["truth"])
    print(f"pcm select_consistent: {len(kept)} of {len(closures)} closures kept ({int(g['outlier'].sum())} outliers planted); rel_error without {e0} with {e1}")
    assert e1[0] < e0[0] and e1[1] < e0[1]
