"""GPU: the correspondence-graph global registration (gloc_reg_pair_graph, gloc_reg_fpfh_graph_batch_ids) against the numpy
restatement tests/pairgraph_ref.py on the case table tests/pairgraph_cases.py.

  Integers  degree, score, seeds, set sizes, per-seed inliers, the winner's rank, its inliers and ok are EQUAL to the
            restatement's on every case (no list has an entry on the compatibility threshold: the CPU file holds that).
  Poses     within 1e-4 m / 1e-4 rad of the restatement (the project's parity rule for poses that come out of an fp64
            Kabsch whose moments are reduced in another order and that come back in float32).
  Batch     the eight same-world known-answer pairs are located from resident scans; a batch of ten is its ten single
            calls bit for bit; a forced small workspace budget, and a target index on either scan, change no bit.
  Widths    pg_score_kernel cuts a wave into 64 / lanes_per_row teams, lanes_per_row the power of two >= min(words, 64),
            and streams rows of more than 64 words 64 at a time.  K.CASES reach 1, 2, 4, 8 and 32 lanes; K.WIDE adds
            16 lanes (M = 513, 600: 9, 10 words; 1000, 1024: 16), 64 lanes (2049: 33 words; 4096: 64) and the streaming
            branch (4097, 4161: 65, 66 words), sparse (planted, density 0.14) and dense (all64: one word walked by 64
            teams; all2049; all4100 streaming); with them up to 5 chunks of ransac_score_kernel and 3 blocks of
            accum_kernel<1>.  The dense lists and the disjoint cliques are compared with closed forms, no restatement
            in between; hypothesis blocks of 16, 64 and 256 are crossed at n_seeds 16 | 17, 64 | 65, 256 | 257.
  Mixed     a batch of jobs of 0, 0 or 1, at most 4 and some hundred pairs shares the longest job's rows, words and
            lanes_per_row: it is its single calls bit for bit at any budget and in any order."""
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


# ---- row widths, closed forms, one handle, mixed batches ----------------------------------------------------------------
INTEGERS = ("degree", "score", "seeds", "set_sizes", "seed_inliers")


@pytest.mark.parametrize("name", K.WIDE)
def test_row_widths_equal_the_restatement(env, oracle_mod, name):
    P, Q, _, _ = K.pair_list(name, oracle_mod)
    _check(env["reg"].pair_graph(P, Q, params=_prm(env["capi"])), K.result(name, oracle_mod), name)


def _check_closed_form(g, x, truth, name):
    """The device against numbers written down without the restatement; the pose against the pure translation."""
    T = g["T"].astype(np.float64)
    off = float(np.linalg.norm(T[:3, 3] - truth[:3, 3])), float(np.arccos(np.clip((np.trace(T[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))
    print(name, "inliers", g["inliers"], x["inliers"], "rank", g["winner_rank"], "pose off the translation by", off)
    for k in INTEGERS:
        assert g[k].dtype == x[k].dtype and (g[k] == x[k]).all(), k
    assert g["winner_rank"] == x["winner_rank"] and g["inliers"] == x["inliers"] and g["ok"] == x["ok"]
    assert off[0] <= 1e-4 and off[1] <= 1e-4


@pytest.mark.parametrize("m", K.ALL_SIZES)
def test_dense_lists_are_their_closed_form(env, oracle_mod, m):
    P, Q, _, truth = K.pair_list("all%d" % m, oracle_mod)
    _check_closed_form(env["reg"].pair_graph(P, Q, params=_prm(env["capi"])), K.all_expected(m), truth, "all%d" % m)


@pytest.mark.parametrize("n_seeds", (64, 272))
def test_cliques_are_their_closed_form(env, oracle_mod, n_seeds):
    """64 seeds: all in the largest group.  272: every pair is a seed, every group is seen, the last two ranks are empty."""
    P, Q, _, truth = K.pair_list("cliques", oracle_mod)
    g = env["reg"].pair_graph(P, Q, params=_prm(env["capi"], n_seeds=n_seeds))
    _check_closed_form(g, K.cliques_expected(n_seeds), truth, "cliques")
    _check(g, K.result("cliques", oracle_mod, n_seeds=n_seeds), "cliques")


@pytest.mark.parametrize("n_seeds", (16, 17, 65, 256, 257))
def test_seed_count_boundaries(env, oracle_mod, n_seeds):
    """Either side of the hypothesis-block sizes of the scoring launch (16 up to 16 seeds, 64 up to 64, 256 beyond)."""
    r = K.result("planted1000", oracle_mod, n_seeds=n_seeds)
    assert r["edge"] == 0
    P, Q, _, _ = K.pair_list("planted1000", oracle_mod)
    _check(env["reg"].pair_graph(P, Q, params=_prm(env["capi"], n_seeds=n_seeds)), r, "planted1000")


@pytest.mark.parametrize("over", [dict(theta_num=1, theta_den=1), dict(compat_thresh=0.25, inlier_thresh=0.3, theta_num=2, theta_den=3, n_seeds=17)],
                         ids=("theta1", "tight"))
def test_parameters_on_streamed_rows(env, oracle_mod, over):
    r = K.result("planted4097", oracle_mod, **over)
    assert r["edge"] == 0
    P, Q, _, _ = K.pair_list("planted4097", oracle_mod)
    _check(env["reg"].pair_graph(P, Q, params=_prm(env["capi"], **over)), r, "planted4097")


def test_one_handle_any_order(capi, oracle_mod):
    """Long, short, dense, long again on one fresh handle, the seed count changing in between: every call is the
    restatement (rows or words a longer list left behind would show), and the same list twice gives the same bits."""
    reg = capi.Registrar()
    try:
        got = []
        for name, n_seeds in (("planted4161", 64), ("planted63", 64), ("all64", 16), ("planted4097", 64), ("planted3", 64), ("planted1000", 64),
                              ("planted4161", 64)):
            over = {} if n_seeds == 64 else dict(n_seeds=n_seeds)
            P, Q, _, _ = K.pair_list(name, oracle_mod)
            got.append(reg.pair_graph(P, Q, params=_prm(capi, **over)))
            _check(got[-1], K.result(name, oracle_mod, **over), name)
        a, b = got[0], got[-1]
        assert all((a[k] == b[k]).all() for k in INTEGERS) and (bits(a["T"]) == bits(b["T"])).all()
        assert (a["inliers"], a["winner_rank"], a["ok"]) == (b["inliers"], b["winner_rank"], b["ok"])
    finally:
        reg.close()


MIXED = ("empty", "true", "n1", "other", "n4", "true")


@pytest.mark.parametrize("order", [MIXED, MIXED[::-1], ("true", "other", "empty", "true", "n1", "n4")], ids=("as_listed", "reversed", "empty_opens_a_group"))
def test_mixed_batch_is_its_single_calls(env, oracle_mod, known, order):
    """One source against targets of no points, one point, four points and two whole scans: jobs of 0, at most 1, at most 4
    and some hundred pairs in one batch, at the default budget and at budgets of one and two jobs in flight (groups then
    start at jobs 1, 2, ... and at 2, 4: short and empty jobs open and close them)."""
    reg, capi, store = env["reg"], env["capi"], env["store"]
    s = known["yaw90_3m"][0]
    small = {n: store.add(fpfh_cases.cloud(n)) for n in ("empty", "n1", "n4")}
    ids = dict(small, true=known["yaw90_3m"][1], other=known["yaw45_2m"][1])
    tg = [ids[n] for n in order]
    prm = _prm(capi)
    try:
        singles = [reg.fpfh_graph_batch(s, [t], params=prm) for t in tg]
        m = max(int(one["n_pairs"][0]) for one in singles)
        per_job = m * ((m + 63) // 64) * 8 + 8 * prm.n_seeds * m
        for jobs_in_flight in (0, 1, 2):                     # (0: the default budget)
            reg.set_option(capi.REG_OPT_PAIRGRAPH_BUDGET, jobs_in_flight * per_job)
            try:
                b = reg.fpfh_graph_batch(s, tg, params=prm)
            finally:
                reg.set_option(capi.REG_OPT_PAIRGRAPH_BUDGET, 0)
            print(order, "in flight", jobs_in_flight, "pairs", b["n_pairs"].tolist(), "inliers", b["inliers"].tolist(), "ok", b["ok"].tolist())
            for c, one in enumerate(singles):
                assert (bits(one["T"][0]) == bits(b["T"][c])).all() and one["inliers"][0] == b["inliers"][c]
                assert one["n_pairs"][0] == b["n_pairs"][c] and one["ok"][0] == b["ok"][c]
            first, second = [c for c, n in enumerate(order) if n == "true"]
            assert (bits(b["T"][first]) == bits(b["T"][second])).all() and b["inliers"][first] == b["inliers"][second]
            assert b["n_pairs"][first] == b["n_pairs"][second] and b["ok"][first] == b["ok"][second]
            r = K.result("known:yaw90_3m", oracle_mod)
            e = gicp_ref.pose_err(r["T"], b["T"][first])
            assert int(b["n_pairs"][first]) == r["n_pairs"] and int(b["inliers"][first]) == r["inliers"] and bool(b["ok"][first]) == r["ok"]
            assert e[0] <= 1e-4 and e[1] <= 1e-4
            for c, n in enumerate(order):
                if n in ("empty", "n1"):
                    assert b["n_pairs"][c] <= 1 and (b["T"][c] == np.eye(4, dtype=np.float32)).all() and not b["ok"][c] and b["inliers"][c] == 0
                if n == "n4":
                    assert b["n_pairs"][c] <= 4
    finally:
        for t in small.values():
            store.release(t)
