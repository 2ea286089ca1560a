"""CPU: the correspondence-graph case table is fit to test with before any device sees it (tests/pairgraph_cases.py,
tests/pairgraph_ref.py): no entry of any list sits on the compatibility threshold, the restatement alone locates the eight
same-world known-answer pairs, it recovers every planted set, the degenerate lists come out as defined, the dense lists
and the disjoint cliques come out as their closed forms, and evaluating G1 in row blocks changed no bit of it."""
import numpy as np
import pytest

import pairgraph_cases as K
import pairgraph_ref as G


@pytest.mark.parametrize("name", K.CASES + K.EXTRA)
def test_no_entry_on_the_threshold(name, oracle_mod):
    """The cap is zero: with no EDGE-flagged entry the bit matrix is decided, and everything up to the fits is integer."""
    r = K.result(name, oracle_mod)
    print(name, "M", r["n_pairs"], "density %.3f" % r["density"], "edge-flagged", r["edge"])
    assert r["edge"] == 0


def test_known_answer_pairs_are_located(oracle_mod):
    """The restatement alone at the defaults: all eight same-world pairs within 1 m / 5 degrees of ground truth."""
    for n in K.KNOWN:
        r = K.result("known:" + n, oracle_mod)
        print(n, "M", r["n_pairs"], "inliers", r["inliers"], "rank", r["winner_rank"], "ok", r["ok"], "err", r["err"], "density %.3f" % r["density"])
    assert len(K.SAME_WORLD) == 8
    for n in K.SAME_WORLD:
        assert K.result("known:" + n, oracle_mod)["located"], n


@pytest.mark.parametrize("m", [m for m in K.SIZES if m >= 63] + list(K.WIDE_SIZES))
def test_planted_set_is_recovered(m, oracle_mod):
    name = "planted%d" % m
    _, _, mask, T = K.pair_list(name, oracle_mod)
    r = K.result(name, oracle_mod)
    assert r["ok"] and (r["winner_mask"] | ~mask).all()           # winner's inliers contain the planted set
    assert r["inliers"] >= int(mask.sum())
    e = np.linalg.inv(T) @ r["T"]
    assert np.linalg.norm(e[:3, 3]) < 0.05 and np.abs(e[:3, :3] - np.eye(3)).max() < 2e-3


def test_degenerate_lists(oracle_mod):
    for m in (0, 1, 2):
        r = K.result("planted%d" % m, oracle_mod)
        assert (r["T"] == np.eye(4)).all() and not r["ok"] and r["inliers"] == 0 and r["winner_rank"] == G.NONE
        assert (r["seeds"][:m] == np.arange(m)).all() and (r["seeds"][m:] == G.NONE).all()
    r = K.result("planted3", oracle_mod)                            # three planted pairs: one triangle, S = 1 on every edge
    assert r["degree"].tolist() == [2, 2, 2] and r["score"].tolist() == [2, 2, 2] and r["set_sizes"][:3].tolist() == [3, 3, 3]
    assert r["ok"] and r["inliers"] == 3 and r["winner_rank"] == 0
    r = K.result("none", oracle_mod)
    assert not r["degree"].any() and not r["score"].any() and not r["set_sizes"].any() and not r["ok"]
    assert (r["T"] == np.eye(4)).all() and (r["seeds"] == np.arange(64)).all()
    r = K.result("all", oracle_mod)
    assert (r["degree"] == 129).all() and (r["score"] == 129 * 128).all() and (r["set_sizes"] == 130).all()
    assert r["ok"] and r["inliers"] == 130 and r["winner_rank"] == 0
    r = K.result("odd", oracle_mod)
    bad = [3, 10, 50, 64, 99]
    assert not r["degree"][bad].any() and not r["score"][bad].any() and not r["winner_mask"][bad].any() and r["ok"]
    r = K.result("dup", oracle_mod)
    assert r["ok"] and (r["degree"][:30] == r["degree"][90:120]).all() and (r["score"][:30] == r["score"][120:150]).all()


def _same_integers(r, x):
    for k in ("degree", "score", "seeds", "set_sizes", "seed_inliers"):
        assert r[k].dtype == x[k].dtype and (r[k] == x[k]).all(), k
    assert r["winner_rank"] == x["winner_rank"] and r["inliers"] == x["inliers"] and r["ok"] == x["ok"]


def _off_translation(T, truth):
    """(metres, radians) of a pose off a pure translation."""
    T = np.asarray(T, np.float64)
    c = np.clip((np.trace(T[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.linalg.norm(T[:3, 3] - truth[:3, 3])), float(np.arccos(c))


@pytest.mark.parametrize("m", K.ALL_SIZES)
def test_dense_lists_are_complete_graphs(m, oracle_mod):
    """all<M>: every row has degree M - 1 and the restatement gives the closed form, number for number."""
    name = "all%d" % m
    r = K.result(name, oracle_mod)
    assert r["n_pairs"] == m and (r["degree"] == m - 1).all() and r["density"] == 1.0
    _same_integers(r, K.all_expected(m))
    assert all(len(s) == m for s in r["sets"][:min(m, 64)]) and r["winner_mask"].all()
    e = _off_translation(r["T"], K.pair_list(name, oracle_mod)[3])
    assert e[0] <= 1e-4 and e[1] <= 1e-4


@pytest.mark.parametrize("n_seeds", (64, 272))
def test_cliques_are_their_closed_form(n_seeds, oracle_mod):
    """C is exactly the block structure meant, and the restatement gives the closed form: at 64 seeds all of them lie in
    the largest group; at 272 every pair is a seed (ranks 270, 271 are empty) and every group is seen."""
    over = {} if n_seeds == 64 else dict(n_seeds=n_seeds)
    r, x = K.result("cliques", oracle_mod, **over), K.cliques_expected(n_seeds)
    assert r["edge"] == 0 and (r["C"] == x["block"]).all()
    assert sorted(np.bincount(x["group"]).tolist()) == sorted(K.CLIQUES) and x["group"][x["seeds"][0]] == 0
    # every group lies across the 64-bit words of the bit rows (groups of one and two pairs aside)
    assert all(len(set(np.flatnonzero(x["group"] == g) // 64)) > 1 for g, n in enumerate(K.CLIQUES) if n >= 3)
    _same_integers(r, x)
    for rank, s in enumerate(x["seeds"]):
        members = None if s == G.NONE or K.CLIQUES[x["group"][s]] < 3 else np.flatnonzero(x["group"] == x["group"][s])
        assert (r["sets"][rank] is None) if members is None else (r["sets"][rank] == members).all()
    assert (r["winner_mask"] == (x["group"] == 0)).all()
    e = _off_translation(r["T"], K.pair_list("cliques", oracle_mod)[3])
    assert e[0] <= 1e-4 and e[1] <= 1e-4


def _compat_whole(P, Q, compat_thresh=0.6):
    """G1 as the restatement evaluated it before the row blocks: the whole [M, M, 3] difference at once."""
    def lengths(X):
        d = X[:, None, :] - X[None, :, :]
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    P, Q = np.asarray(P, np.float32).reshape(-1, 3), np.asarray(Q, np.float32).reshape(-1, 3)
    fin = np.isfinite(P).all(1) & np.isfinite(Q).all(1)
    both = fin[:, None] & fin[None, :] & ~np.eye(len(P), dtype=bool)
    thr = float(np.float32(compat_thresh))
    with np.errstate(all="ignore"):
        diff = np.abs(lengths(P.astype(np.float64)) - lengths(Q.astype(np.float64)))
        return (diff < thr) & both, int(((np.abs(diff - thr) < G.EDGE_EPS) & both).sum())


@pytest.mark.parametrize("name", ("planted257", "odd", "known:yaw90_3m"))
def test_row_blocks_change_no_bit(name, oracle_mod, monkeypatch):
    """compat() in row blocks (one short block, blocks that do not divide M, one block for all) is the whole-matrix form:
    the same C and the same edge count, also at another threshold with a band that DOES flag entries; S and the scores likewise."""
    P, Q, _, _ = K.pair_list(name, oracle_mod)
    C0, e0 = _compat_whole(P, Q)
    monkeypatch.setattr(G, "EDGE_EPS", 0.05)                     # (a band wide enough to flag entries of these lists)
    C1, e1 = _compat_whole(P, Q, 0.25)
    assert e1 > 0
    monkeypatch.undo()
    c = C0.astype(np.float64)
    S0 = np.where(C0, np.rint(c @ c), 0).astype(np.int64)
    for block in (G.ROW_BLOCK, 1, 100, len(P) + 7):
        monkeypatch.setattr(G, "ROW_BLOCK", block)
        C, e = G.compat(P, Q)
        assert C.dtype == np.bool_ and (C == C0).all() and e == e0
        monkeypatch.setattr(G, "EDGE_EPS", 0.05)
        C, e = G.compat(P, Q, 0.25)
        assert (C == C1).all() and e == e1
        monkeypatch.undo()
        if block != 1:
            S, score = G.second_order(C0)
            assert (S == S0).all() and (score == S0.sum(1).astype(np.uint64)).all()
            assert G.second_order(C0, keep=False)[0] is None and (G.second_order(C0, keep=False)[1] == score).all()
            assert (G.second_rows(C0, np.array([5, 0, 64])) == S0[[5, 0, 64]]).all()
    r = K.result(name, oracle_mod)
    assert (r["C"] == C0).all() and (r["S"] == S0).all() and r["edge"] == e0


def test_long_lists_keep_no_matrix(oracle_mod, monkeypatch):
    """Above KEEP_MATRICES the session's cache holds neither C nor S; the integers come out the same with or without them."""
    assert K.result("planted2049", oracle_mod)["C"] is None and K.result("planted2049", oracle_mod)["S"] is None
    assert K.result("planted1025", oracle_mod)["C"] is not None
    P, Q, _, _ = K.pair_list("planted129", oracle_mod)
    a = K.result("planted129", oracle_mod)
    monkeypatch.setattr(G, "KEEP_MATRICES", 0)
    b = G.graph(P, Q, oracle_mod, **K.PARAMS)
    assert b["C"] is None and b["S"] is None
    _same_integers(a, b)
    assert (a["T"] == b["T"]).all()


@pytest.mark.parametrize("name", ("known:yaw90_3m", "planted129", "dup", "odd"))
def test_symmetry(name, oracle_mod):
    r = K.result(name, oracle_mod)
    C, S = r["C"], r["S"]
    assert (C == C.T).all() and (S == S.T).all() and not C.diagonal().any() and not S.diagonal().any()
    assert (S[~C] == 0).all() and (r["degree"] == C.sum(1)).all()


def test_parameters_reach_the_rule(oracle_mod):
    """theta = 1/1 keeps only the row maxima; one seed is the top score alone; a ratio gate turns ok off."""
    a, b = K.result("planted257", oracle_mod), K.result("planted257", oracle_mod, theta_num=1, theta_den=1)
    assert (b["set_sizes"] <= a["set_sizes"]).all() and (b["set_sizes"] < a["set_sizes"]).any()
    one = K.result("planted257", oracle_mod, n_seeds=1)
    assert one["seeds"][0] == a["seeds"][0] and one["set_sizes"][0] == a["set_sizes"][0] and one["winner_rank"] == 0
    assert not K.result("planted257", oracle_mod, min_inlier_ratio=0.9)["ok"]
