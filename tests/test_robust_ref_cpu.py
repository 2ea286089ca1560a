"""CPU: the robust weighting's restatement (tests/robust_ref.py) against the library's host helpers bit for bit, its
properties on the exact form, the proof that every whole-alignment case of tests/robust_cases.py is stable, and the
reason for the feature: on the moved-object scene the robust refinements end nearer the truth than the plain ones."""
import numpy as np
import pytest

import gicp_ref as G
import gn_cases as GC
import p2l_ref as P
import robust_cases as RC
import robust_ref as RR
import vgicp_ref as V

MAX_ITERS = 30
# schedules that reach `scale` after 0, 1, 7 and more than MAX_ITERS updates, and none
SCHEDULES = [(0.0, 0.0), (1.0, 0.5), (1.5, 0.5), (100.0, 0.5), (1e6, 0.9), (2.0, 0.999)]
SETTLE = [0, 0, 1, 7, None, None]


def _blocks():
    for kind in (RR.NONE,) + RR.KINDS:
        for c in (0.25, 0.1, 3.0):
            for start, anneal in SCHEDULES:
                yield RR.block(kind, c, c * start, anneal)


def _s2_table(c):
    c2 = np.float64(c) * np.float64(c)
    return [0.0, 5e-324, float(np.nextafter(c2, 0.0)), float(c2), float(np.nextafter(c2, np.inf)), float(4.0 * c2), 1e300]


def test_the_schedules_settle_where_the_table_says():
    for (start, anneal), want in zip(SCHEDULES, SETTLE):
        rb = RR.block(RR.CAUCHY, 0.25, 0.25 * start, anneal)
        assert RR.settled(rb, MAX_ITERS) == want, (start, anneal)
        cs = [RR.scale(rb, k) for k in range(MAX_ITERS + 2)]
        assert all(a >= b >= rb["scale"] for a, b in zip(cs, cs[1:]))
        assert cs[0] == (rb["scale_start"] or rb["scale"])
        if want is not None:
            assert cs[want] == rb["scale"] and (want == 0 or cs[want - 1] > rb["scale"]) and cs[-1] == rb["scale"]
        else:
            assert cs[MAX_ITERS] > rb["scale"]


def test_the_host_helpers_equal_the_restatement_bit_for_bit(capi):
    n = 0
    for rb in _blocks():
        prm = capi.default_robust_params(**rb)
        assert (prm.scale, prm.scale_start, prm.anneal) == (rb["scale"], rb["scale_start"], rb["anneal"])     # (already float32)
        for k in (0, 1, 2, 6, 7, 8, MAX_ITERS, MAX_ITERS + 5, 1000):
            c = RR.scale(rb, k)
            if rb["kind"] != RR.NONE:
                assert capi.robust_scale(prm, k) == c, (rb, k)
            for s2 in _s2_table(c if rb["kind"] != RR.NONE else 1.0):
                want = float(RR.weight(rb["kind"], s2, c))
                got = capi.robust_weight(prm, k, s2)
                assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (rb, k, s2, got, want)
                n += 1
    print(f"{n} weights equal bit for bit")


@pytest.mark.parametrize("kind", RR.KINDS)
def test_weights_are_in_0_1_and_fall_with_the_residual(kind):
    c = 0.3
    s2 = np.concatenate([[0.0, 5e-324], np.geomspace(1e-12, 1e12, 4001), [1e300]])
    w = RR.weight(kind, s2, c)
    assert (w >= 0).all() and (w <= 1).all() and w[0] == 1.0 and (np.diff(w) <= 0).all() and w[-1] <= 1e-100
    # Huber and Tukey are continuous across t = 1: the kink's two float64 neighbours
    c2 = np.float64(c) * np.float64(c)
    lo, at, hi = RR.weight(kind, [np.nextafter(c2, 0.0), c2, np.nextafter(c2, np.inf)], c)
    if kind == RR.HUBER:
        assert lo == 1.0 and at == 1.0 and 1.0 - 1e-15 <= hi <= 1.0
    if kind == RR.TUKEY:
        assert 0.0 <= lo <= 1e-30 and at == 0.0 and hi == 0.0
    assert abs(lo - at) <= 1e-9 and abs(hi - at) <= 1e-9


def _exact_systems(oracle, kind):
    """The three weighted systems (the kind at robust_cases' scale for each method) and their plain twins on the exact
    form, a2_n257 against a0."""
    rb = {m: RC.robust(m, kind) for m in RC.METHODS}
    nn = GC.finite_nn(oracle)
    s, t = GC.cloud("a2_n257"), GC.cloud("a0")
    sn, tn = GC.normals("a2_n257", oracle), GC.normals("a0", oracle)
    T = GC.truth("a2", "a0") @ GC._se3(0.7, (0.08, -0.05, 0.02))
    vox = V.voxels(t, tn)
    return [(RR.p2l_system(s, t, tn, T, nn, rb["p2l"], rb["p2l"]["scale"], 1.0, exact=True), P.system(s, t, tn, T, nn, 1.0, exact=True)),
            (RR.gicp_system(s, sn, t, tn, T, nn, rb["gicp"], rb["gicp"]["scale"], 1.0, exact=True), G.system(s, sn, t, tn, T, nn, 1.0, exact=True)),
            (RR.vgicp_system(s, sn, vox, T, rb["vgicp"], rb["vgicp"]["scale"], exact=True), V.system(s, sn, vox, T, exact=True))]


def test_kind_none_equals_the_plain_restatements(oracle_mod):
    for got, want in _exact_systems(oracle_mod, RR.NONE):
        scale = max(np.abs(want[0]).max(), np.abs(want[1]).max(), want[2])
        assert np.abs(got[0] - want[0]).max() <= 1e-9 * scale and np.abs(got[1] - want[1]).max() <= 1e-9 * scale
        assert abs(got[2] - want[2]) <= 1e-9 * scale and got[3] == want[3] > 6 and got[4] == got[3]


@pytest.mark.parametrize("kind", RR.KINDS)
def test_a_weighted_system_keeps_the_sum_and_the_count(oracle_mod, kind):
    """... and its H is below the plain one (weights in [0, 1]): x^T H x for a few x."""
    rng = np.random.default_rng(5)
    for got, want in _exact_systems(oracle_mod, kind):
        assert got[3] == want[3] and abs(got[2] - want[2]) <= 1e-9 * want[2]
        assert 0.0 < got[4] < got[3]
        for _ in range(5):
            x = rng.normal(size=6)
            assert 0.0 <= x @ got[0] @ x <= (x @ want[0] @ x) * (1 + 1e-9)


def test_tukey_at_a_tiny_scale_is_degenerate_at_once(oracle_mod):
    nn = GC.finite_nn(oracle_mod)
    s, t, tn = GC.cloud("a2_n257"), GC.cloud("a0"), GC.normals("a0", oracle_mod)
    T = GC.truth("a2", "a0") @ GC._se3(0.7, (0.08, -0.05, 0.02))
    rb = RR.block(RR.TUKEY, 1e-6)
    H, g, s2, cnt, wsum = RR.p2l_system(s, t, tn, T, nn, rb, rb["scale"], exact=True)
    assert cnt >= 6 and not H.any() and not g.any() and wsum == 0.0 and s2 > 0
    ev = []
    r = RR.p2l_align(s, t, tn, nn, rb, init_T=T, max_iters=5, exact=True, events=ev)
    assert r["status"] == 2 and r["iters"] == 0 and ev == ["degenerate_at_0"] and (r["T"] == T).all() and r["weight"] == 0.0


def test_a_schedule_that_never_settles_never_converges(oracle_mod):
    """anneal so close to 1 that c never reaches scale within the cap: no status 1, however large the eps -- and the same
    job with no schedule converges at its first update."""
    nn = GC.finite_nn(oracle_mod)
    s, t, tn = GC.cloud("a2_n257"), GC.cloud("a0"), GC.normals("a0", oracle_mod)
    T = GC.truth("a2", "a0")
    kw = dict(init_T=T, max_iters=8, max_corr_dist=1.0, trans_eps=10.0, rot_eps=10.0, exact=True)
    slow = RR.p2l_align(s, t, tn, nn, RR.block(RR.CAUCHY, 0.1, 0.2, 0.999), **kw)
    assert RR.settled(RR.block(RR.CAUCHY, 0.1, 0.2, 0.999), 8) is None
    assert slow["status"] == 0 and slow["iters"] == 8
    assert RR.p2l_align(s, t, tn, nn, RR.block(RR.CAUCHY, 0.1), **kw)["status"] == 1
    # one that settles at update 3 stops there, not before
    r = RR.p2l_align(s, t, tn, nn, RR.block(RR.CAUCHY, 0.1, 0.8, 0.5), **kw)
    assert r["status"] == 1 and r["iters"] == 4


def test_every_case_of_the_gpu_table_is_stable(oracle_mod):
    """The case table tests/test_robust_gpu.py holds the device to: every case stable by the rule of tests/gn_cases.py."""
    refs = RC.references(oracle_mod)
    assert len(refs) == len(RC.CASES) == 27
    for c in RC.CASES:
        r = refs[c["name"]]
        print(f"{c['name']}: floor {r['floor'][0]:.1e} m {r['floor'][1]:.1e} rad, iters {r['ref']['iters']}, status {r['ref']['status']}, "
              f"mean weight {r['ref']['weight']:.4f}, {r['events']}")
        assert r["stable"], c["name"]
    for m in RC.METHODS:                                          # the schedule's two cases do what they are there for
        assert refs["a20_gnc_eps_" + m]["ref"]["status"] == 1 and refs["a20_gnc_eps_" + m]["ref"]["iters"] >= 4
        assert refs["a20_gnc_slow_" + m]["ref"]["status"] == 0 and refs["a20_gnc_slow_" + m]["ref"]["iters"] == 5


def test_the_moved_object_pulls_the_plain_refinement_not_the_robust_one(oracle_mod):
    """The reason for the feature, on the restatement: the translation error to the truth of the plain refinement is more
    than twice the robust one's, for Cauchy and Tukey, in all three methods."""
    refs = RC.references(oracle_mod)
    moved = RC.moved_mask(GC.cloud("a2"))
    assert 1000 < moved.sum() < 0.1 * len(moved)
    truth = RC.truth(RC.MOVED, "a0")
    for m in RC.METHODS:
        err = {k: P.pose_err(truth, refs["moved_%s_%s" % (k, m)]["ref"]["T"])[0] for k in ("none", "cauchy", "tukey")}
        print(f"{m}: translation error plain {err['none']:.4f} m, Cauchy {err['cauchy']:.4f} m, Tukey {err['tukey']:.4f} m")
        assert err["none"] > 2 * err["cauchy"] and err["none"] > 2 * err["tukey"], m
