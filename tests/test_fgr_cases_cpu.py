"""CPU: the Fast Global Registration case table is fit to test with before any device sees it (tests/fgr_cases.py,
tests/fgr_ref.py): no tuple edge of a synthetic list sits on the test's inequalities, the restatement recovers every planted
motion, hardly a pair sits on the inlier threshold, the degenerate lists come out as defined, the located set of known pairs
is the committed one, and no Cholesky pivot comes near the degeneracy rule but on the two rows that say so."""
import numpy as np
import pytest

import fgr_cases as K
import fgr_ref as R
import pairgraph_ref as G

ROWS = tuple(K.ROWS)


@pytest.mark.parametrize("name", K.SYNTH)
def test_no_tuple_edge_on_the_inequalities(name, oracle_mod):
    """The cap is zero on the synthetic lists at every parameter row the device is compared at: the multiplicities are then
    decided.  (Not asked of "all" at tuple_scale = 1: there s lp < lq and s lq < lp exclude each other, so no tuple can
    pass whatever the rounding.)"""
    for row in ROWS:
        r = K.result(name, oracle_mod, **K.ROWS[row])
        print(name, row, "M", r["n_pairs"], "tuples", r["n_tuples"], "active", int((r["mult"] > 0).sum()), "edge-flagged", r["edge"])
        assert r["edge"] == 0
    if name == "all":
        r = K.result(name, oracle_mod, **K.SCALE1)
        assert r["n_tuples"] == 0 and r["status"] == 2 and not r["ok"] and not r["mult"].any()


@pytest.mark.parametrize("m", [m for m in K.SIZES if m >= 3])
def test_planted_motion_is_recovered(m, oracle_mod):
    """Within 0.1 m / 0.5 degrees of the planted motion, every planted pair an inlier."""
    name = "planted%d" % m
    P, Q, mask, T = K.pair_list(name, oracle_mod)
    r = K.result(name, oracle_mod)
    e = np.linalg.inv(T) @ r["T64"]
    off = float(np.linalg.norm(e[:3, 3])), float(np.degrees(np.arccos(np.clip((np.trace(e[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))))
    print(name, "tuples", r["n_tuples"], "inliers", r["inliers"], "of planted", int(mask.sum()), "off the planted motion by", off)
    assert r["status"] == 0 and r["ok"] and off[0] <= 0.1 and off[1] <= 0.5
    inl = G.inlier_mask(P, Q, r["T"][:3, :3].reshape(9).astype(np.float32), r["T"][:3, 3].astype(np.float32), np.float32(K.PARAMS["inlier_thresh"]))
    assert (inl | ~mask).all() and r["inliers"] >= int(mask.sum())


@pytest.mark.parametrize("name", K.CASES)
def test_hardly_a_pair_on_the_inlier_threshold(name, oracle_mod):
    """The pairs whose fp64 residual lies within 1e-4 + 1e-4 |x| of inlier_thresh (the band a pose within the device's pose
    tolerance can move a residual by): none on the synthetic lists at any row but the three runs fgr_cases.NEAR_THRESH
    lists with their counts (1 to 5 pairs of some 4 096), at most EDGE_CAP of M on the known lists.  With so few against the
    inliers there, no flagged pair can decide ok anywhere on the table."""
    for row in ROWS:
        r = K.result(name, oracle_mod, **K.ROWS[row])
        print(name, row, "M", r["n_pairs"], "inliers", r["inliers"], "near the threshold", r["near"])
        assert r["near"] <= K.EDGE_CAP * r["n_pairs"]
        if name in K.SYNTH:
            assert r["near"] == K.NEAR_THRESH.get((name, row), 0)
        assert not K.ok_hangs_on_flagged_pairs(r)


def test_degenerate_lists(oracle_mod):
    for row in ROWS:
        for m in (0, 1, 2):
            r = K.result("planted%d" % m, oracle_mod, **K.ROWS[row])
            assert (r["T"] == np.eye(4)).all() and r["status"] == 2 and not r["ok"] and r["inliers"] == 0 and not r["mult"].any()
            assert not r["system"].any()
        r = K.result("line", oracle_mod, **K.ROWS[row])          # H[0][0] is a sum of exact zeros: degenerate at once
        assert r["system"][0] == 0.0 and r["pivot_fail"] == 0.0 and r["updates"] == 0
        assert (r["T"] == np.eye(4)).all() and r["status"] == 2 and not r["ok"] and r["inliers"] == 0
        if K.ROWS[row].get("tuple_tries", 1) and "max_tuples" not in K.ROWS[row]:
            assert r["n_tuples"] == 1000 and int(r["mult"].sum()) == 3000   # every tuple passes
        r = K.result("none", oracle_mod, **K.ROWS[row])          # no tuple passes; without the test, P on a line: as "line"
        assert r["n_tuples"] == 0 and (r["T"] == np.eye(4)).all() and r["status"] == 2 and not r["ok"] and r["inliers"] == 0
    r = K.result("odd", oracle_mod)
    assert not r["mult"][[3, 10, 50, 64, 99]].any() and r["ok"]
    r = K.result("odd", oracle_mod, tuple_tries=0)
    assert not r["mult"][[3, 10, 50, 64, 99]].any() and int(r["mult"].sum()) == 95 and r["n_tuples"] == 0
    r = K.result("all", oracle_mod)
    assert r["ok"] and r["inliers"] == 130 and r["n_tuples"] == 1000


def test_located_set_is_the_committed_one(oracle_mod):
    for n in K.KNOWN:
        r = K.result("known:" + n, oracle_mod)
        print(n, "M", r["n_pairs"], "tuples", r["n_tuples"], "inliers", r["inliers"], "ok", r["ok"], "err", r["err"], "located", r["located"])
    assert len(K.SAME_WORLD) == 8 and len(K.LOCATED) >= 6 and set(K.LOCATED) <= set(K.SAME_WORLD)
    assert tuple(n for n in K.KNOWN if K.result("known:" + n, oracle_mod)["located"]) == K.LOCATED


@pytest.mark.parametrize("name", K.CASES)
def test_pivots_stay_clear_of_the_rule(name, oracle_mod):
    """A Cholesky pivot d passes iff d > 1e-12 dmax.  Rounding moves d / dmax by some 1e-14 (a 6 x 6 elimination of sums of
    a few thousand products), so a pivot a factor 1e3 above the rule, or one that is exactly 0, is decided the same way by
    any correct evaluation; fgr_cases.NEAR_RULE lists the runs that are not."""
    for row in ROWS:
        r = K.result(name, oracle_mod, **K.ROWS[row])
        print(name, row, "updates", r["updates"], "status", r["status"], "smallest pivot / dmax", r["pivot_min"], "failing", r["pivot_fail"])
        if (name, row) in K.NEAR_RULE:
            assert r["pivot_min"] < 1e-9
            continue
        assert r["pivot_min"] >= 1e-9
        assert r["pivot_fail"] is None or r["pivot_fail"] == 0.0


def test_the_table_straddles_the_kernels_lds_capacity():
    """planted4096 | 4097 are either side of the capacity only as long as the kernel header says 4096."""
    import os
    import re
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gloc3d_amd", "csrc", "fgr_kernels.hpp")
    with open(hdr) as f:
        cap = int(re.search(r"constexpr uint32_t LDS_CAP = (\d+);", f.read()).group(1))
    assert cap == K.LDS_CAP and K.LDS_CAP in K.SIZES and K.LDS_CAP + 1 in K.SIZES


def test_parameters_reach_the_rule(oracle_mod):
    """The schedule: at anneal_every = 1 mu has reached delta^2 long before the last update; a ratio gate turns ok off; the
    stream id changes the samples."""
    P, Q, _, _ = K.pair_list("planted257", oracle_mod)
    assert not K.result("planted257", oracle_mod, min_inlier_ratio=0.9)["ok"]
    a, b = K.result("planted257", oracle_mod), R.fgr(P, Q, oracle_mod, stream_id=5, **K.PARAMS)
    assert (a["mult"] != b["mult"]).any() and a["n_tuples"] != 0 and b["ok"]
    one = K.result("planted257", oracle_mod, max_tuples=1)
    assert one["n_tuples"] == 1 and int(one["mult"].sum()) == 3
