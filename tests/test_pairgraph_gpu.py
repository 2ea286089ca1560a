"""GPU: the correspondence-graph global registration (gloc_reg_pair_graph, gloc_reg_fpfh_graph_batch_ids) against the numpy
restatement tests/pairgraph_ref.py on the case table tests/pairgraph_cases.py.

  Integers  degree, score, seeds, set sizes, per-seed inliers, the winner's rank, its inliers and ok are EQUAL to the
            restatement's on every case (no list has an entry on the compatibility threshold: the CPU file holds that).
  Poses     within 1e-4 m / 1e-4 rad of the restatement (the project's parity rule for poses that come out of an fp64
            Kabsch whose moments are reduced in another order and that come back in float32).
  Batch     the eight same-world known-answer pairs are located from resident scans; a batch of ten is its ten single
            calls bit for bit; a forced small workspace budget, and a target index on either scan, change no bit."""
import numpy as np
import pytest

import fpfh_cases
import gicp_ref
import pairgraph_cases as K
import pairgraph_ref as G
from util import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(capi, oracle_mod):
    store = capi.ScanStore()
    reg = capi.Registrar(store=store)
    yield dict(store=store, reg=reg, capi=capi)
    reg.close()
    store.close()


def _prm(capi, **over):
    return capi.default_fpfh_graph_params(**dict(K.PARAMS, **over))


def _check(g, r, name):
    e = gicp_ref.pose_err(r["T"], g["T"])
    print(name, "M", r["n_pairs"], "inliers", g["inliers"], r["inliers"], "rank", g["winner_rank"], r["winner_rank"], "ok", g["ok"], r["ok"],
          "pose off the restatement by", e)
    assert (g["degree"] == r["degree"]).all()
    assert (g["score"] == r["score"]).all()
    assert (g["seeds"] == r["seeds"]).all()
    assert (g["set_sizes"] == r["set_sizes"]).all()
    assert (g["seed_inliers"] == r["seed_inliers"]).all()
    assert g["winner_rank"] == r["winner_rank"] and g["inliers"] == r["inliers"] and g["ok"] == r["ok"]
    assert e[0] <= 1e-4 and e[1] <= 1e-4


@pytest.mark.parametrize("name", K.CASES)
def test_pair_graph_equals_the_restatement(env, oracle_mod, name):
    P, Q, _, _ = K.pair_list(name, oracle_mod)
    _check(env["reg"].pair_graph(P, Q, params=_prm(env["capi"])), K.result(name, oracle_mod), name)


@pytest.mark.parametrize("over", [dict(theta_num=1, theta_den=1), dict(n_seeds=1), dict(n_seeds=1024, min_inlier_ratio=0.9),
                                  dict(compat_thresh=0.25, inlier_thresh=0.3, theta_num=2, theta_den=3, n_seeds=17)],
                         ids=("theta1", "one_seed", "all_seeds", "tight"))
def test_parameters(env, oracle_mod, over):
    """Other parameters on the planted list of 257 (n_seeds beyond M: the ranks past M are empty) and on a known pair."""
    for name in ("planted257", "known:yaw90_3m"):
        r = K.result(name, oracle_mod, **over)
        assert r["edge"] == 0                                   # (no entry on this threshold either)
        P, Q, _, _ = K.pair_list(name, oracle_mod)
        _check(env["reg"].pair_graph(P, Q, params=_prm(env["capi"], **over)), r, name)


def test_outputs_are_optional(env, oracle_mod):
    """Every output may be NULL; an empty list leaves the identity."""
    import ctypes as C
    capi = env["capi"]
    P, Q, _, _ = K.pair_list("planted65", oracle_mod)
    prm = _prm(capi)
    T = np.empty(16, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    capi.check(capi.lib().gloc_reg_pair_graph(env["reg"]._h, ptr(P), ptr(Q), len(P), C.byref(prm), None, None, None, None, None, ptr(T), None, None, None))
    assert (bits(T.reshape(4, 4)) == bits(env["reg"].pair_graph(P, Q, params=prm)["T"])).all()
    capi.check(capi.lib().gloc_reg_pair_graph(env["reg"]._h, ptr(P), ptr(Q), len(P), C.byref(prm), None, None, None, None, None, None, None, None, None))
    g = env["reg"].pair_graph(P[:0], Q[:0], params=prm)
    assert (g["T"] == np.eye(4, dtype=np.float32)).all() and not g["ok"] and g["winner_rank"] == G.NONE and (g["seeds"] == G.NONE).all()


# ---- batch on resident scans ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def known(env, oracle_mod):
    """The known-answer pairs resident: name -> (source id, target id)."""
    ids = {}
    for name in K.KNOWN:
        src, tgt, _ = fpfh_cases.known_filtered(name)
        ids[name] = (env["store"].add(src), env["store"].add(tgt))
    return ids


@pytest.mark.parametrize("name", K.KNOWN)
def test_batch_equals_the_restatement(env, oracle_mod, known, name):
    r = K.result("known:" + name, oracle_mod)
    s, t = known[name]
    g = env["reg"].fpfh_graph_batch(s, [t], params=_prm(env["capi"]))
    e = gicp_ref.pose_err(r["T"], g["T"][0])
    print(name, "pairs", int(g["n_pairs"][0]), r["n_pairs"], "inliers", int(g["inliers"][0]), r["inliers"], "ok", bool(g["ok"][0]), r["ok"],
          "pose off the restatement by", e)
    assert int(g["n_pairs"][0]) == r["n_pairs"] and int(g["inliers"][0]) == r["inliers"] and bool(g["ok"][0]) == r["ok"]
    assert e[0] <= 1e-4 and e[1] <= 1e-4
    # ... and the host-list entry point on the same list gives the same bits
    P, Q, _, _ = K.pair_list("known:" + name, oracle_mod)
    assert (bits(env["reg"].pair_graph(P, Q, params=_prm(env["capi"]))["T"]) == bits(g["T"][0])).all()


def test_known_answer_pairs_are_located(env, oracle_mod, known):
    for name in K.SAME_WORLD:
        s, t = known[name]
        g = env["reg"].fpfh_graph_batch(s, [t], params=_prm(env["capi"]))
        f = env["reg"].fpfh_batch(s, [t], stream_ids=[0])
        truth = fpfh_cases.known_filtered(name)[2]
        err, err_f = fpfh_cases.pose_error(g["T"][0], truth), fpfh_cases.pose_error(f["T"][0], truth)
        print(name, "M", int(g["n_pairs"][0]), "graph: inliers %d, %.3f m %.3f deg" % ((int(g["inliers"][0]),) + err),
              "| RANSAC: inliers %d, %.3f m %.3f deg" % ((int(f["inliers"][0]),) + err_f))
        assert g["ok"][0] and err[0] <= K.OK_T and err[1] <= K.OK_R


def _same(a, b):
    return all((bits(a[k].astype(np.float32)) == bits(b[k].astype(np.float32))).all() for k in ("T", "inliers", "n_pairs", "ok"))


def test_batch_is_its_single_calls_whatever_the_budget(env, oracle_mod, known):
    reg, capi = env["reg"], env["capi"]
    s = known["yaw90_3m"][0]
    tg = [known[n][1] for n in K.KNOWN]                       # ten jobs: one true pair, the others whatever they match
    prm = _prm(capi)
    b1 = reg.fpfh_graph_batch(s, tg, params=prm)
    assert _same(b1, reg.fpfh_graph_batch(s, tg, params=prm))
    for c, t in enumerate(tg):
        one = reg.fpfh_graph_batch(s, [t], params=prm)
        assert (bits(one["T"][0]) == bits(b1["T"][c])).all() and one["inliers"][0] == b1["inliers"][c]
        assert one["n_pairs"][0] == b1["n_pairs"][c] and one["ok"][0] == b1["ok"][c]
    # a workspace budget that holds one job at a time, then three
    m = int(b1["n_pairs"].max())
    per_job = m * ((m + 63) // 64) * 8 + 8 * prm.n_seeds * m
    for jobs_in_flight in (1, 3):
        reg.set_option(capi.REG_OPT_PAIRGRAPH_BUDGET, jobs_in_flight * per_job)
        try:
            assert _same(b1, reg.fpfh_graph_batch(s, tg, params=prm))
        finally:
            reg.set_option(capi.REG_OPT_PAIRGRAPH_BUDGET, 0)
    assert b1["ok"][list(K.KNOWN).index("yaw90_3m")]


def test_target_index_changes_no_bit(env, oracle_mod, known):
    reg, store = env["reg"], env["store"]
    prm = _prm(env["capi"])
    s, t = known["yaw170_1m"]
    b = reg.fpfh_graph_batch(s, [t], params=prm)
    src, tgt, _ = fpfh_cases.known_filtered("yaw170_1m")
    s2, t2 = store.add(src), store.add(tgt)
    store.build_target_index(t2)
    k1 = reg.fpfh_graph_batch(s2, [t2], params=prm)
    store.build_target_index(s2)
    k2 = reg.fpfh_graph_batch(s2, [t2], params=prm)
    assert _same(b, k1) and _same(b, k2)
    store.release(s2)
    store.release(t2)


@pytest.mark.parametrize("src,tgt", [("empty", "a_vox"), ("a_vox", "empty"), ("n1", "a_vox"), ("zn", "a_vox"), ("n4", "n4")])
def test_fewer_than_three_pairs(env, oracle_mod, src, tgt):
    store = env["store"]
    s, t = store.add(fpfh_cases.cloud(src)), store.add(fpfh_cases.cloud(tgt))
    g = env["reg"].fpfh_graph_batch(s, [t, t], params=_prm(env["capi"]))
    r = G.register(fpfh_cases.cloud(src), fpfh_cases.cloud(tgt), oracle_mod, **K.PARAMS)
    assert (g["n_pairs"] == r["n_pairs"]).all() and (g["inliers"] == r["inliers"]).all() and (g["ok"] == r["ok"]).all()
    if r["n_pairs"] < 3:
        assert (g["T"] == np.eye(4, dtype=np.float32)).all() and not g["ok"].any()
    store.release(s)
    store.release(t)


def test_the_fpfh_stage_is_untouched(env, oracle_mod, known):
    """gloc_reg_fpfh_batch_ids before and after graph calls on the same handle: the same bits, and the restatement's counts."""
    reg = env["reg"]
    s, t = known["yaw45_2m"]
    a = reg.fpfh_batch(s, [t], stream_ids=[0])
    reg.fpfh_graph_batch(s, [t])
    b = reg.fpfh_batch(s, [t], stream_ids=[0])
    assert _same(a, b)
    ref = fpfh_cases.known_result("yaw45_2m", oracle_mod)
    assert int(a["n_pairs"][0]) == ref["n_pairs"] and int(a["inliers"][0]) == ref["inliers"]
