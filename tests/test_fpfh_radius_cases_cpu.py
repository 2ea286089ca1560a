"""CPU: the radius-support FPFH case table is fit to test with before any device sees it (tests/fpfh_radius_cases.py,
tests/fpfh_radius_ref.py): the edge cap on every pairing, every intended branch of the search reached, the brute-force lists
against a second statement, and the known-answer set decided by the restatement alone."""
import numpy as np
import pytest

import fpfh_cases as K
import fpfh_radius_cases as RK
import fpfh_radius_ref as R
import fpfh_ref as F


@pytest.mark.parametrize("name,sup", RK.FEATURES)
def test_edge_cap(name, sup, oracle_mod):
    """At most 1 % of a cloud's points are edge-flagged under the support it is tested with (normal_min_nn >= 4 is what
    keeps this at zero: three points span an exact plane and the role test of F1 then hangs on the last bit)."""
    f = RK.features(name, sup, oracle_mod)
    n = len(RK.cloud(name))
    flagged = int(f["flagged"].sum())
    print(name, sup, "points", n, "edge-flagged", flagged, "with a normal", int((f["nrm"] != 0).any(1).sum()), "with a feature",
          int((f["feat"] != 0).any(1).sum()))
    assert flagged <= K.EDGE_CAP * n


def test_branches_are_reached(oracle_mod):
    """Truncated, short and too-short lists, empty lists, duplicates at d2 = 0, and the lattice's boundary ties."""
    f = RK.features("corner", "S_A", oracle_mod)
    assert int((f["count"] > RK.S_A[3]).sum()) == 417 and len(f["count"]) == 432 and int(f["count"].max()) <= 360
    f = RK.features("a", "S_RAW", oracle_mod)
    nmax, fmax, nmin = RK.S_RAW[2], RK.S_RAW[3], RK.S_RAW[4]
    assert (f["ncount"] > nmax).any() and (f["ncount"] < nmax).any() and (f["ncount"] < nmin).any()
    assert (f["count"] > fmax).any() and (f["count"] < fmax).any()
    assert not (f["nrm"][f["ncount"] < nmin] != 0).any() and (f["nrm"][f["ncount"] >= nmin] != 0).any(1).all()
    assert (f["ncount"] >= 1).all()                                        # a finite point is in its own neighbourhood
    f = RK.features("a_odd", "S_RAW", oracle_mod)
    x = RK.cloud("a_odd")
    bad = ~np.isfinite(x).all(1)
    assert bad.any() and (f["count"][bad] == 0).all() and (f["idx"][bad] == R.NONE).all() and (f["d2"][bad] == R.FLT_MAX).all()
    inside = f["idx"] != R.NONE
    assert not bad[f["idx"][inside]].any()                                 # ... and is in nobody's
    assert ((f["d2"] == 0) & inside).sum(1).max() >= 2                     # duplicates: itself and its copy at d2 = 0
    assert (f["count"][~bad] >= 1).all()
    # the lattice: r2 = 4 is reached exactly, and the cap of 16 cuts through the twelve ties at d2 = 2
    idx, d2, count = RK.lists("lattice", 2.0, 16)
    p = RK.cloud("lattice")
    interior = ((p >= 2) & (p <= 5)).all(1)
    assert interior.sum() == 64 and (count[interior] == 33).all()
    wide = R.radius_lists(p, 2.0, 40)
    assert ((wide[1] == 4.0).sum(1)[interior] == 6).all()
    assert ((d2[interior] == 2.0).sum(1) == 9).all() and ((wide[1][interior] == 2.0).sum(1) == 12).all()
    for i in np.flatnonzero(interior)[:8]:
        ties = np.sort(wide[0][i][wide[1][i] == 2.0])
        assert (idx[i][d2[i] == 2.0] == ties[:9]).all()                    # the nine smaller indices, ascending
    # the uniform cloud: many chunks, mostly short lists
    _, _, count = RK.lists("uniform", 1.5, 128)
    assert len(count) == 4161 and np.median(count) < 16 and count.max() < 128 and (count >= 1).all()


@pytest.mark.parametrize("name,r,max_nn", RK.LISTS)
def test_lists_agree_with_a_second_statement(name, r, max_nn, oracle_mod):
    """fp64 distances with a guard band: everything clearly inside r is counted, nothing clearly outside is; the rows are
    ascending in (d2, index); and where a neighbourhood has at most 16 members the list IS the checker's exact 16-NN list
    cut at its length."""
    x = RK.cloud(name)
    idx, d2, count = RK.lists(name, r, max_nn)
    n = len(x)
    assert idx.shape == (n, max_nn) and count.shape == (n,)
    if n == 0:
        return
    P = x.astype(np.float64)
    r2 = float(np.float32(r)) ** 2
    sure_in, sure_out = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for s in range(0, n, 512):
        with np.errstate(all="ignore"):
            D = ((P[s:s + 512, None, :] - P[None, :, :]) ** 2).sum(2)
            sure_in[s:s + 512], sure_out[s:s + 512] = (D <= r2 * (1 - 1e-5)).sum(1), (D <= r2 * (1 + 1e-5)).sum(1)
    assert (count >= sure_in).all() and (count <= sure_out).all()
    filled = (idx != R.NONE).sum(1)
    assert (filled == np.minimum(count, max_nn)).all()
    if max_nn > 1:
        dd, di = np.diff(d2.astype(np.float64), axis=1), np.diff(idx.astype(np.int64), axis=1)
        both = np.arange(1, max_nn)[None, :] < filled[:, None]
        assert (((dd > 0) | ((dd == 0) & (di > 0))) | ~both).all()
    with np.errstate(invalid="ignore"):
        assert (d2[idx != R.NONE] <= np.float32(r) * np.float32(r)).all()
    if n >= 16:
        kidx, kd2 = oracle_mod.ground_knn(x, 16)
        rows = np.flatnonzero((count <= min(16, max_nn)) & (count > 0))
        for i in rows:
            c = int(count[i])
            assert (idx[i, :c] == kidx[i, :c]).all() and (d2[i, :c].view(np.uint32) == kd2[i, :c].view(np.uint32)).all()
        print(name, r, max_nn, "rows checked against the 16-NN lists", len(rows), "of", n)


def test_features_are_histograms(oracle_mod):
    for name, sup in (("a_vox", "S_A"), ("a_odd", "S_RAW"), ("corner", "S_A"), ("zn", "S_A"), ("n1", "S_A")):
        f = RK.features(name, sup, oracle_mod)
        has = (f["feat64"] != 0).any(1)
        sums = f["feat64"].reshape(len(has), 3, 11).sum(2)
        assert np.allclose(sums[has], 100.0, atol=1e-9) and (sums[~has] == 0).all()
        assert not has[~(f["nrm"] != 0).any(1)].any()
        assert f["used"].max(initial=0) <= 127                             # the SPFH counts fit the device's bytes
    assert not (RK.features("zn", "S_A", oracle_mod)["feat"] != 0).any()


@pytest.mark.parametrize("sup", RK.KNOWN_SUPPORTS)
def test_known_answer_set(sup, oracle_mod):
    """The restatement alone on the ten pairs at this support: the located set is what the device is held to.  It must be
    non-empty and contain the two same-position pairs; the pairs of different worlds have no answer.  Nothing is asserted
    about radius against k."""
    located = RK.known_answer_cases(sup, oracle_mod)
    for n in K.KNOWN:
        r = RK.known_result(n, sup, oracle_mod)
        print(sup, n, "pairs", r["n_pairs"], "inliers", r["inliers"], "ok", r["ok"], "err", r["err"], "located", r["located"])
    assert located and "yaw90_0m" in located and "yaw180_0m" in located
    assert not any(len(K.KNOWN[n]) > 4 for n in located)
