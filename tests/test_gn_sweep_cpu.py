"""CPU: the alignment cases of tests/gn_cases.py judged by the float64 restatements alone (tests/p2l_ref.py,
tests/gicp_ref.py), before any of them is held against the device (tests/test_gn_sweep_gpu.py): at least 90 % of the cases
are stable under a second summation order (and inverse), the stable ones between them take every branch of the shared
Gauss-Newton loop that p2l_ref.EVENTS names, on both sides of the host's look every 4 passes, and the restatements skip
or keep each edge input as their docstrings say.

Run time: about a minute on one core (two runs of a restatement per case, ~12 k points a scan)."""
import numpy as np

import gicp_ref as G
import gn_cases as GC
import p2l_ref as P


def test_cases_span_the_inputs():
    names = [c["name"] for c in GC.CASES]
    assert len(set(names)) == len(names) >= 60
    for m in ("p2l", "gicp"):
        cs = [c for c in GC.CASES if c["method"] == m]
        assert {c["src"][0] for c in cs} >= set(GC.WORLDS) and len({c["tgt"] for c in cs if len(c["tgt"]) == 2}) >= 6
        assert {GC.params(c)["max_iters"] for c in cs} >= {1, 3, 4, 5, 8, 9}
        eps = {(GC.params(c)["trans_eps"] > 0, GC.params(c)["rot_eps"] > 0) for c in cs}
        assert eps == {(False, False), (True, False), (False, True), (True, True)}
        assert {c["src"] for c in cs} >= {"a2_odd", "a0_dup", "a2_n1", "a2_n5", "a2_n64", "a2_n257"}
        assert {c["tgt"] for c in cs} >= {"a0_odd", "a0_dup", "a0_zn", "empty"}
        assert max(abs(c["off"][0]) for c in cs) >= 60 and min(abs(c["off"][0]) for c in cs if c["off"][0]) <= 0.5
    for n in GC.SIZES:
        assert len(GC.cloud("a2_n%d" % n)) == n
    for name in ("a2_odd", "a0_odd"):
        x = GC.cloud(name)
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and (x[120:130] == x[20:30]).all()
    assert len(GC.cloud("empty")) == 0


def test_most_cases_are_stable_and_every_branch_is_taken(oracle_mod):
    refs = GC.references(oracle_mod)
    stable = [c for c in GC.CASES if refs[c["name"]]["stable"]]
    unstable = [c["name"] for c in GC.CASES if not refs[c["name"]]["stable"]]
    share = len(stable) / len(GC.CASES)
    print("\nstable: %d of %d cases (%.1f %%); unstable: %s" % (len(stable), len(GC.CASES), 100 * share, unstable or "none"))
    print("%-20s %s" % ("event", "stable cases that take it (point-to-plane, generalized)"))
    for e in P.EVENTS:
        hits = [sum(1 for c in stable if c["method"] == m and e in refs[c["name"]]["events"]) for m in ("p2l", "gicp")]
        print("%-20s %d %d" % (e, hits[0], hits[1]))
        assert min(hits) >= 1, e
    assert share >= 0.9
    for m in ("p2l", "gicp"):
        mine = [c for c in stable if c["method"] == m]
        ends = lambda c: (refs[c["name"]]["events"][-1], refs[c["name"]]["ref"]["iters"])
        # the stop test on both sides of the host's look every 4 passes: jobs that stop at pass 4 and at pass 5 of 9 ...
        assert {ends(c)[1] for c in mine if ends(c)[0] == "converged" and GC.params(c)["max_iters"] == 9} >= {4, 5}, m
        assert ends(GC.by_name("a20_stop4_" + m)) == ("converged", 4) and ends(GC.by_name("a20_stop5_" + m)) == ("converged", 5)
        # ... every cap the issue names, reached
        assert {ends(c)[1] for c in mine if ends(c)[0] == "capped"} >= {1, 3, 4, 5, 8, 9}, m
        # one eps without the other never converges
        half = [c for c in mine if (GC.params(c)["trans_eps"] > 0) != (GC.params(c)["rot_eps"] > 0)]
        assert len(half) >= 2 and all(ends(c) == ("capped", GC.params(c)["max_iters"]) for c in half)
        # the mixed batches: one source and one parameter block each, between them every ending
        seen = set()
        for batch in GC.MIXED[m]:
            cs = [GC.by_name(n) for n in batch]
            assert len({c["src"] for c in cs}) == 1 and len({tuple(sorted(GC.params(c).items())) for c in cs}) == 1
            assert all(refs[n]["stable"] for n in batch)
            seen |= {ends(c) for c in cs}
        assert len({i for k, i in seen if k == "degenerate_later"}) >= 2
        # all four endings, converged at two different passes, in ONE call: the corner batch
        corner = {ends(GC.by_name(n)) for n in GC.MIXED[m][0]}
        assert {k for k, _ in corner} == {"capped", "converged", "degenerate_at_0", "degenerate_later"}, (m, corner)
        assert len({i for k, i in corner if k == "converged"}) >= 2, (m, corner)


def test_recording_events_changes_nothing(oracle_mod):
    for name in ("b31_it3_p2l", "b31_it3_gicp"):
        a, b = GC.run(GC.by_name(name), oracle_mod), GC.references(oracle_mod)[name]["ref"]
        assert (a["T"] == b["T"]).all() and a["iters"] == b["iters"] and a["status"] == b["status"] and a["rmse"] == b["rmse"]


def test_the_restatements_skip_or_keep_each_edge_input(oracle_mod):
    nn = GC.finite_nn(oracle_mod)
    I = np.eye(4)
    src, tgt = GC.cloud("a2_odd"), GC.cloud("a0_odd")
    sn, tn = GC.normals("a2_odd", oracle_mod), GC.normals("a0_odd", oracle_mod)
    fin_s, fin_t = np.isfinite(src).all(1), np.isfinite(tgt).all(1)
    assert 0 < (~fin_s).sum() < 200 and 0 < (~fin_t).sum() < 200
    assert not sn[~fin_s].any() and not tn[~fin_t].any()                     # a non-finite point has no normal
    zero_t = ~tn.any(1)
    idx, d2 = nn(P.move(I, src), tgt)
    assert (idx[~fin_s] == GC.NO_PAIR).all() and (idx[fin_s] < len(tgt)).all() and fin_t[idx[fin_s]].all()
    # non-finite sources are dropped by both; a zero-normal target is dropped by point-to-plane, kept by generalized ICP
    n_p2l, n_gicp = len(P.pairs(src, tgt, tn, I, nn)[0]), len(G.pairs(src, sn, tgt, tn, I, nn)[0])
    on_zero = int(zero_t[idx[fin_s]].sum())
    print("\nfinite sources %d of %d; matched to a target without a normal: %d; pairs: point-to-plane %d, generalized %d"
          % (fin_s.sum(), len(src), on_zero, n_p2l, n_gicp))
    assert n_gicp == fin_s.sum() and n_p2l == n_gicp - on_zero
    # ... on a target the device is given too: two finite points without a normal between NaN rows
    zt, zn = GC.cloud("a0_zn"), GC.normals("a0_zn", oracle_mod)
    assert np.isfinite(zt).all(1).sum() == 2 and not zn.any()
    full = GC.cloud("a2")
    T0 = GC.guess(GC.by_name("zero_nrm_tgt_p2l"))
    on_zero = len(G.pairs(full, GC.normals("a2", oracle_mod), zt, zn, T0, nn)[0])
    assert on_zero == len(full) > 0 and len(P.pairs(full, zt, zn, T0, nn)[0]) == 0
    refs = GC.references(oracle_mod)
    assert refs["zero_nrm_tgt_p2l"]["ref"]["status"] == 2 and refs["zero_nrm_tgt_p2l"]["ref"]["iters"] == 0
    assert refs["zero_nrm_tgt_gicp"]["stable"] and refs["zero_nrm_tgt_gicp"]["ref"]["iters"] >= 1
    # a target whose normals are ALL zero: nothing for point-to-plane, everything for generalized ICP (S = 2I - a m m^T)
    none = np.zeros_like(tn)
    assert len(P.pairs(src, tgt, none, I, nn)[0]) == 0 and P.system(src, tgt, none, I, nn)[3] == 0
    H, g, s, cnt = G.system(src, sn, tgt, none, I, nn)
    assert cnt == fin_s.sum() and np.isfinite(H).all() and P.cholesky_solve(H, g) is not None
    # duplicated points: the smallest index among equals, on both sides
    dup = GC.cloud("a0_dup")
    idx, d2 = nn(dup, dup)
    assert (d2 == 0).all() and (idx == (np.arange(len(dup)) // 3) * 3).all()
    # an empty target: no pairs, a zero system, degenerate at once with the guess returned
    e = GC.cloud("empty")
    assert P.system(src, e, e, I, nn)[3] == 0 and G.system(src, sn, e, e, I, nn)[3] == 0
    for m in ("p2l", "gicp"):
        r = GC.references(oracle_mod)["empty_tgt_" + m]["ref"]
        assert r["status"] == 2 and r["iters"] == 0 and r["rmse"] == 0.0
        assert (r["T"] == GC.guess(GC.by_name("empty_tgt_" + m)).astype(np.float64)).all()
    # the two summation orders are two evaluations of one system
    a, b = P.system(src, tgt, tn, I, nn), P.system(src, tgt, tn, I, nn, order="reversed")
    assert a[3] == b[3] and 0 < np.abs(a[0] - b[0]).max() <= 1e-12 * np.abs(a[0]).max()
