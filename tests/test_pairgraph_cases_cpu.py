"""CPU: the correspondence-graph case table is fit to test with before any device sees it (tests/pairgraph_cases.py,
tests/pairgraph_ref.py): no entry of any list sits on the compatibility threshold, the restatement alone locates the eight
same-world known-answer pairs, it recovers every planted set, and the degenerate lists come out as defined."""
import numpy as np
import pytest

import pairgraph_cases as K
import pairgraph_ref as G


@pytest.mark.parametrize("name", K.CASES)
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


@pytest.mark.parametrize("m", [m for m in K.SIZES if m >= 63])
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
