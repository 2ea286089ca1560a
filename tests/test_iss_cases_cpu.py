"""CPU: the ISS case table is fit to test with before any device sees it (tests/iss_cases.py, tests/iss_ref.py): every
case has what it is meant to have under the restatement, every intended branch is reached, and the restatement's pieces
agree with second statements of themselves.  Where a condition fails the CASE is wrong, not the rule."""
import numpy as np
import pytest

import fpfh_cases as K
import iss_cases as IK
import iss_ref as I


@pytest.mark.parametrize("name", list(IK.CASES))
def test_every_case_has_what_it_is_meant_to_have(name, oracle_mod):
    prm, want = IK.CASES[name]
    s = IK.saliency(name, oracle_mod)
    k, n = len(s["kp"]), len(IK.cloud(name))
    print(name, "points", n, "salient", int((s["sal"] > 0).sum()), "K", k, "truncated lists", int((s["count"] > prm["max_nn"]).sum()))
    if want == "keypoints":
        assert k >= 3
    elif want == "none":
        assert k == 0
    else:
        assert k == want
    assert (np.diff(s["kp"].astype(np.int64)) > 0).all() and (s["sal"][s["kp"]] > 0).all()
    e = s["eig"]
    assert (e[:, 0] >= e[:, 1]).all() and (e[:, 1] >= e[:, 2]).all()
    short = np.minimum(s["count"], prm["max_nn"]) < prm["min_nn"]
    assert not (e[short] != 0).any() and not (s["sal"][short] != 0).any()


def test_branches_are_reached(oracle_mod):
    sizes = {n: len(IK.cloud(n)) for n in IK.CASES}
    assert [sizes[n] for n in ("empty", "n1", "n2", "n4", "u63", "u64", "u65", "uniform")] == [0, 1, 2, IK.D["min_nn"] - 1, 63, 64, 65, 4161]
    # too few points: every list is short, although the points are well within the radius of each other
    assert (IK.saliency("n4", oracle_mod)["count"] == 4).all()
    # the lattice: equal positive saliencies within the radius (the index decides) and neighbours exactly at r
    s, x = IK.saliency("lattice", oracle_mod), IK.cloud("lattice")
    prm = IK.CASES["lattice"][0]
    r2 = np.float32(prm["non_max_radius"]) ** 2
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    pos = s["sal"] > 0
    both = pos[:, None] & pos[None, :] & ~np.eye(len(x), dtype=bool)
    ties = both & (d2 <= r2) & (s["sal"][:, None] == s["sal"][None, :])
    assert ties.any() and (both & (d2 == r2)).any()
    assert (ties[s["kp"]].any(1)).any()                                    # a keypoint that won a tie ...
    for i in s["kp"]:
        assert not (ties[i] & (np.arange(len(x)) < i)).any()               # ... and none that should have lost one
    values, mult = np.unique(s["sal"][pos], return_counts=True)
    assert len(values) <= 4 and mult.max() >= 64
    # the plane: the smallest eigenvalue is exactly zero wherever there is a list
    s = IK.saliency("plane", oracle_mod)
    assert (s["eig"][:, 2] == 0).all() and (s["eig"][:, 0] > 0).any() and not (s["sal"] != 0).any()
    # duplicates: a point and its copy share lists, saliency and fate -- the copy with the smaller index may win, the other never
    s, x = IK.saliency("dups", oracle_mod), IK.cloud("dups")
    _, first, inv = np.unique(x, axis=0, return_index=True, return_inverse=True)
    twin = np.flatnonzero(first[inv.ravel()] != np.arange(len(x)))
    assert len(twin) == 40
    assert (s["sal"][twin].view(np.uint32) == s["sal"][first[inv.ravel()][twin]].view(np.uint32)).all()
    assert not s["keep"][twin].any() and (s["sal"][twin] > 0).any()
    # the NaN point: no list, no saliency, in nobody's list
    s = IK.saliency("nan", oracle_mod)
    assert s["count"][77] == 0 and s["sal"][77] == 0 and not (s["idx"] == 77).any()
    # the corner scene: every list truncated; the odd scan: non-finite rows and truncated and short lists together
    s = IK.saliency("corner", oracle_mod)
    assert (s["count"] > 128).all()
    s, x = IK.saliency("a_odd", oracle_mod), IK.cloud("a_odd")
    bad = ~np.isfinite(x).all(1)
    assert bad.any() and (s["count"][bad] == 0).all() and (s["count"] > 128).any() and ((s["count"] > 0) & (s["count"] < 5)).any()
    # not salient although the list is long enough: the gammas decide too
    s = IK.saliency("uniform", oracle_mod)
    assert ((s["sal"] == 0) & (s["eig"][:, 2] > 0)).any()


@pytest.mark.parametrize("name", ["u65", "lattice", "dups", "nan", "corner"])
def test_saliency_agrees_with_a_second_statement(name, oracle_mod):
    """The eigenvalues against numpy's symmetric eigensolver on the covariance of the same lists (summed by numpy, in its
    own order): equal to 1e-9 of the largest; and the saliency is l3 or 0 by the rule."""
    x, prm, s = IK.cloud(name).astype(np.float64), IK.CASES[name][0], IK.saliency(name, oracle_mod)
    g21, g32 = float(np.float32(prm["gamma_21"])), float(np.float32(prm["gamma_32"]))
    for i in range(len(x)):
        nb = s["idx"][i][s["idx"][i] != I.NONE]
        if len(nb) < prm["min_nn"]:
            assert s["sal"][i] == 0
            continue
        q = x[nb] - x[nb].mean(0)
        w = np.linalg.eigvalsh(q.T @ q)[::-1]
        assert np.abs(w - s["eig"][i]).max() <= 1e-9 * max(w[0], 1.0)
        l1, l2, l3 = s["eig"][i]
        assert s["sal"][i] == (np.float32(l3) if (l3 > 0 and l2 < g21 * l1 and l3 < g32 * l2) else 0)


@pytest.mark.parametrize("name", ["u65", "uniform", "lattice", "dups"])
def test_suppression_agrees_with_a_second_statement(name, oracle_mod):
    """Sequentially, strongest first (ties to the smaller index): a point is a keypoint iff it is not within r of a point
    that ranks before it -- whether or not that point is itself a keypoint."""
    x, prm, s = IK.cloud(name), IK.CASES[name][0], IK.saliency(name, oracle_mod)
    r2 = np.float32(prm["non_max_radius"]) * np.float32(prm["non_max_radius"])
    order = np.lexsort((np.arange(len(x)), -s["sal"].astype(np.float64)))
    rank = np.empty(len(x), np.int64)
    rank[order] = np.arange(len(x))
    keep = np.zeros(len(x), bool)
    for i in np.flatnonzero(s["sal"] > 0):
        d = x[i] - x
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep[i] = not ((d2 <= r2) & (rank < rank[i])).any()
    assert (keep == s["keep"]).all()


def test_restricted_tables():
    f = np.arange(1, 5 * 33 + 1, dtype=np.float32).reshape(5, 33)
    r = I.restrict(f, np.array([1, 3], np.uint32))
    assert (r[[1, 3]] == f[[1, 3]]).all() and not (r[[0, 2, 4]] != 0).any()
    assert not (I.restrict(f, np.zeros(0, np.uint32)) != 0).any()


@pytest.mark.parametrize("iss", list(IK.ISS_SETS))
def test_known_pairs_under_the_restatement(iss, oracle_mod):
    """What the keypoint entries are held to on the ten pairs, decided by the restatement alone: keypoint and pair counts,
    inliers, and how many of the eight same-world pairs are located (reported, not asserted: fewer is a result)."""
    located = 0
    for name in K.KNOWN:
        ks, kt = IK.known_keypoints(name, iss, oracle_mod)
        r = IK.known_result(name, None, iss, False, oracle_mod)
        truth = K.known_filtered(name)[2]
        err = None if truth is None else K.pose_error(r["T"], truth)
        ok = bool(err is not None and r["ok"] and err[0] <= K.OK_T and err[1] <= K.OK_R)
        located += ok
        print(iss, name, "keypoints", len(ks), len(kt), "pairs", r["n_pairs"], "inliers", r["inliers"], "ok", r["ok"], "err", err, "located", ok)
        assert len(ks) >= 3 and len(kt) >= 3 and r["n_pairs"] <= min(len(ks), len(kt))
    print(iss, "located", located, "of 8")
