"""GPU: Fast Global Registration (gloc_reg_fgr_pairs, gloc_reg_fpfh_fgr_batch_ids and its _radius / _keypoints forms) against
the numpy restatement tests/fgr_ref.py on the case table tests/fgr_cases.py.

  Integers  the multiplicities, n_tuples, status and ok are EQUAL to the restatement's on every case at every parameter
            row (no synthetic list has a tuple edge on the test's inequalities: the CPU file holds that).
  fp64      D^2 and the 27 sums of the last update formed agree to 1e-9 relative to the largest entry, as the _system tests
            of the Gauss-Newton refinements ask.
  Poses     within 1e-4 m / 1e-4 rad of the restatement: the project's tolerance for a pose against its fp64 restatement.
  Inliers   equal where the restatement flags no pair near the threshold, else within the flagged count; ok exact unless
            the flagged pairs could carry the count across what ok asks for (no case of the table).
  Batch     the ten known pairs against the restatement; exactly the committed set is located; a batch is its single calls
            bit for bit in either order, with tiny scans mixed in, with and without target indices and stream ids."""
import ctypes as C

import numpy as np
import pytest

import fgr_cases as K
import fgr_ref as R
import fpfh_cases
import fpfh_radius_cases as RK
import gicp_ref
import iss_cases as IK
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
    return capi.default_fgr_params(**dict(K.PARAMS, **over))


def _check(g, r, name):
    e = gicp_ref.pose_err(r["T"], g["T"])
    top = float(np.abs(r["system"]).max())
    sys_off = float(np.abs(g["system"] - r["system"]).max()) / top if top > 0 else float(np.abs(g["system"]).max())
    d2_off = abs(g["d2"] - r["d2"]) / r["d2"] if r["d2"] > 0 else abs(g["d2"])
    print(name, "M", r["n_pairs"], "tuples", g["n_tuples"], r["n_tuples"], "status", g["status"], r["status"], "inliers", g["inliers"], r["inliers"],
          "near", r["near"], "ok", g["ok"], r["ok"], "d2 off by", d2_off, "system off by", sys_off, "pose off the restatement by", e)
    assert g["mult"].dtype == r["mult"].dtype and (g["mult"] == r["mult"]).all()
    assert g["n_tuples"] == r["n_tuples"]
    assert d2_off <= 1e-9
    assert sys_off <= 1e-9
    assert e[0] <= 1e-4 and e[1] <= 1e-4
    assert g["status"] == r["status"]
    assert abs(g["inliers"] - r["inliers"]) <= r["near"]
    assert g["ok"] == r["ok"] or K.ok_hangs_on_flagged_pairs(r)


@pytest.mark.parametrize("row", list(K.ROWS))
@pytest.mark.parametrize("name", K.CASES)
def test_fgr_pairs_equals_the_restatement(env, oracle_mod, name, row):
    """default; max_iters 1, 4, 5 (across the first anneal step); no tuple test (every finite pair active: planted4096 | 4097
    are either side of what the kernel keeps in LDS); one tuple; anneal_every = 1."""
    over = K.ROWS[row]
    P, Q, _, _ = K.pair_list(name, oracle_mod)
    _check(env["reg"].fgr_pairs(P, Q, params=_prm(env["capi"], **over)), K.result(name, oracle_mod, **over), name + " " + row)


def test_scale_one_on_the_dense_list(env, oracle_mod):
    """tuple_scale = 1 on "all": whatever the restatement says (strict inequalities both ways: nothing passes)."""
    P, Q, _, _ = K.pair_list("all", oracle_mod)
    _check(env["reg"].fgr_pairs(P, Q, params=_prm(env["capi"], **K.SCALE1)), K.result("all", oracle_mod, **K.SCALE1), "all scale1")


def test_stream_id_reaches_the_samples(env, oracle_mod):
    P, Q, _, _ = K.pair_list("planted257", oracle_mod)
    _check(env["reg"].fgr_pairs(P, Q, params=_prm(env["capi"]), stream_id=5), R.fgr(P, Q, oracle_mod, stream_id=5, **K.PARAMS), "planted257 stream 5")


def test_more_active_pairs_than_lds_holds_with_the_test_on(env, oracle_mod):
    """4000 tuples on a dense list of 6000 (every sample passes; some 5200 distinct members): the tuple members themselves
    overflow the LDS copy and are streamed."""
    over = dict(max_tuples=4000, tuple_tries=5000, max_iters=8)
    P, Q, _, _ = K.pair_list("all6000", oracle_mod)
    r = R.fgr(P, Q, oracle_mod, **dict(K.PARAMS, **over))
    assert r["n_tuples"] == 4000 and int((r["mult"] > 0).sum()) > K.LDS_CAP and r["edge"] == 0
    _check(env["reg"].fgr_pairs(P, Q, params=_prm(env["capi"], **over)), r, "all6000 streamed")


def test_outputs_are_optional(env, oracle_mod):
    """Every output but the pose may be NULL; an empty list leaves the identity."""
    capi = env["capi"]
    P, Q, _, _ = K.pair_list("planted65", oracle_mod)
    prm = _prm(capi)
    T = np.empty(16, np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    capi.check(capi.lib().gloc_reg_fgr_pairs(env["reg"]._h, ptr(P), ptr(Q), len(P), 0, C.byref(prm), None, None, None, None, ptr(T), None, None, None))
    assert (bits(T.reshape(4, 4)) == bits(env["reg"].fgr_pairs(P, Q, params=prm)["T"])).all()
    for m in (0, 1, 2):
        g = env["reg"].fgr_pairs(P[:m], Q[:m], params=prm)
        assert (g["T"] == np.eye(4, dtype=np.float32)).all() and not g["ok"] and g["status"] == 2 and g["inliers"] == 0
        assert not g["mult"].any() and not g["system"].any() and g["d2"] == 0.0 and g["n_tuples"] == 0


# ---- batch on resident scans ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def known(env, oracle_mod):
    """The known-answer pairs resident: name -> (source id, target id)."""
    ids = {}
    for name in K.KNOWN:
        src, tgt, _ = fpfh_cases.known_filtered(name)
        ids[name] = (env["store"].add(src), env["store"].add(tgt))
    return ids


def _check_job(g, c, r, name):
    e = gicp_ref.pose_err(r["T"], g["T"][c])
    print(name, "pairs", int(g["n_pairs"][c]), r["n_pairs"], "inliers", int(g["inliers"][c]), r["inliers"], "near", r["near"], "ok", bool(g["ok"][c]),
          r["ok"], "pose off the restatement by", e)
    assert int(g["n_pairs"][c]) == r["n_pairs"] and abs(int(g["inliers"][c]) - r["inliers"]) <= r["near"]
    assert e[0] <= 1e-4 and e[1] <= 1e-4
    assert bool(g["ok"][c]) == r["ok"] or K.ok_hangs_on_flagged_pairs(r)


@pytest.mark.parametrize("name", K.KNOWN)
def test_batch_equals_the_restatement(env, oracle_mod, known, name):
    r = K.result("known:" + name, oracle_mod)
    s, t = known[name]
    g = env["reg"].fpfh_fgr_batch(s, [t], params=_prm(env["capi"]), stream_ids=[0])
    _check_job(g, 0, r, name)
    # ... and the host-list entry point on the same list gives the same bits
    P, Q, _, _ = K.pair_list("known:" + name, oracle_mod)
    one = env["reg"].fgr_pairs(P, Q, params=_prm(env["capi"]))
    assert (bits(one["T"]) == bits(g["T"][0])).all() and one["inliers"] == g["inliers"][0] and one["ok"] == g["ok"][0]


def test_exactly_the_committed_set_is_located(env, oracle_mod, known):
    located = []
    for name in K.SAME_WORLD:
        s, t = known[name]
        g = env["reg"].fpfh_fgr_batch(s, [t], params=_prm(env["capi"]), stream_ids=[0])
        err = fpfh_cases.pose_error(g["T"][0], fpfh_cases.known_filtered(name)[2])
        print(name, "M", int(g["n_pairs"][0]), "inliers", int(g["inliers"][0]), "ok", bool(g["ok"][0]), "%.3f m %.3f deg" % err)
        if g["ok"][0] and err[0] <= K.OK_T and err[1] <= K.OK_R:
            located.append(name)
    assert tuple(located) == K.LOCATED


def _same(a, b):
    return all((bits(a[k].astype(np.float32)) == bits(b[k].astype(np.float32))).all() for k in ("T", "inliers", "n_pairs", "ok"))


def _is_its_singles(reg, prm, s, tg, streams):
    """The batch (stream ids given, or None: 0 .. n - 1) against one call per job."""
    b = reg.fpfh_fgr_batch(s, tg, params=prm, stream_ids=streams)
    assert _same(b, reg.fpfh_fgr_batch(s, tg, params=prm, stream_ids=streams))
    for c, t in enumerate(tg):
        one = reg.fpfh_fgr_batch(s, [t], params=prm, stream_ids=[c if streams is None else streams[c]])
        assert (bits(one["T"][0]) == bits(b["T"][c])).all() and one["inliers"][0] == b["inliers"][c]
        assert one["n_pairs"][0] == b["n_pairs"][c] and one["ok"][0] == b["ok"][c]
    return b


@pytest.mark.parametrize("order", ("listed", "reversed"))
@pytest.mark.parametrize("streams", ([3, 0, 7, 1, 3, 2, 9, 4, 5, 6], None), ids=("stream_ids", "null_stream_ids"))
def test_batch_is_its_single_calls(env, oracle_mod, known, order, streams):
    reg = env["reg"]
    s = known["yaw90_3m"][0]
    tg = [known[n][1] for n in K.KNOWN]                       # ten jobs: one true pair, the others whatever they match
    if order == "reversed":
        tg, streams = tg[::-1], None if streams is None else streams[::-1]
    b = _is_its_singles(reg, _prm(env["capi"]), s, tg, streams)
    assert (b["n_pairs"] >= 3).all()


MIXED = ("empty", "true", "n1", "other", "n4", "true")


@pytest.mark.parametrize("order", [MIXED, MIXED[::-1]], ids=("as_listed", "reversed"))
def test_mixed_batch_is_its_single_calls(env, oracle_mod, known, order):
    """One source against targets of no points, one point, four points and two whole scans in one batch."""
    reg, store = env["reg"], env["store"]
    s = known["yaw90_3m"][0]
    small = {n: store.add(fpfh_cases.cloud(n)) for n in ("empty", "n1", "n4")}
    ids = dict(small, true=known["yaw90_3m"][1], other=known["yaw45_2m"][1])
    try:
        b = _is_its_singles(reg, _prm(env["capi"]), s, [ids[n] for n in order], [0] * len(order))
        first, second = [c for c, n in enumerate(order) if n == "true"]
        assert (bits(b["T"][first]) == bits(b["T"][second])).all() and b["inliers"][first] == b["inliers"][second]
        _check_job(b, first, K.result("known:yaw90_3m", oracle_mod), "yaw90_3m in a mixed batch")
        for c, n in enumerate(order):
            if n in ("empty", "n1"):
                assert b["n_pairs"][c] <= 1 and (b["T"][c] == np.eye(4, dtype=np.float32)).all() and not b["ok"][c] and b["inliers"][c] == 0
            if n == "n4":
                assert b["n_pairs"][c] <= 4
    finally:
        for t in small.values():
            store.release(t)


def test_target_index_changes_no_bit(env, oracle_mod, known):
    reg, store = env["reg"], env["store"]
    prm = _prm(env["capi"])
    s, t = known["yaw170_1m"]
    b = reg.fpfh_fgr_batch(s, [t], params=prm, stream_ids=[0])
    src, tgt, _ = fpfh_cases.known_filtered("yaw170_1m")
    s2, t2 = store.add(src), store.add(tgt)
    store.build_target_index(t2)
    k1 = reg.fpfh_fgr_batch(s2, [t2], params=prm, stream_ids=[0])
    store.build_target_index(s2)
    k2 = reg.fpfh_fgr_batch(s2, [t2], params=prm, stream_ids=[0])
    assert _same(b, k1) and _same(b, k2)
    store.release(s2)
    store.release(t2)


def _sup(capi, s):
    nr, fr, nmax, fmax, nmin = RK.SUPPORTS[s]
    return capi.default_fpfh_radius_params(normal_radius=nr, feature_radius=fr, normal_max_nn=nmax, feature_max_nn=fmax, normal_min_nn=nmin)


def _on_the_siblings_list(name, sibling, oracle_mod):
    """The restatement on the match list the graph stage's restatement reports for the same features (its "pairs")."""
    src, tgt, _ = fpfh_cases.known_filtered(name)
    pairs = sibling["pairs"]
    return R.fgr(src[pairs[:, 0]], tgt[pairs[:, 1]], oracle_mod, **K.PARAMS)


def test_radius_form(env, oracle_mod):
    reg, store, capi = env["reg"], env["store"], env["capi"]
    name, sup = "yaw90_0m", "S_B"
    src, tgt, _ = fpfh_cases.known_filtered(name)
    s, t = store.add(src), store.add(tgt)
    try:
        sib = RK.known_graph_result(name, sup, oracle_mod)
        g = reg.fpfh_fgr_batch(s, [t], params=_prm(capi), support=_sup(capi, sup), stream_ids=[0])
        gg = reg.fpfh_graph_batch(s, [t], support=_sup(capi, sup))
        assert int(gg["n_pairs"][0]) == sib["n_pairs"]
        _check_job(g, 0, _on_the_siblings_list(name, sib, oracle_mod), name + " " + sup)
    finally:
        store.release(s)
        store.release(t)


def test_keypoints_form(env, oracle_mod):
    reg, store, capi = env["reg"], env["store"], env["capi"]
    name, iss = "yaw90_0m", "dense"
    src, tgt, _ = fpfh_cases.known_filtered(name)
    s, t = store.add(src), store.add(tgt)
    try:
        sib = IK.known_result(name, None, iss, True, oracle_mod)
        kprm = capi.default_iss_params(**IK.ISS_SETS[iss])
        g = reg.fpfh_fgr_batch(s, [t], params=_prm(capi), keypoints=kprm, stream_ids=[0])
        gg = reg.fpfh_graph_batch(s, [t], keypoints=kprm)
        assert int(gg["n_pairs"][0]) == sib["n_pairs"]
        _check_job(g, 0, _on_the_siblings_list(name, sib, oracle_mod), name + " keypoints " + iss)
    finally:
        store.release(s)
        store.release(t)


@pytest.mark.parametrize("src,tgt", [("empty", "a_vox"), ("a_vox", "empty"), ("n1", "a_vox"), ("zn", "a_vox"), ("n4", "n4")])
def test_fewer_than_three_pairs(env, oracle_mod, src, tgt):
    store = env["store"]
    s, t = store.add(fpfh_cases.cloud(src)), store.add(fpfh_cases.cloud(tgt))
    g = env["reg"].fpfh_fgr_batch(s, [t, t], params=_prm(env["capi"]), stream_ids=[0, 0])
    r = R.register(fpfh_cases.cloud(src), fpfh_cases.cloud(tgt), oracle_mod, **K.PARAMS)
    assert (g["n_pairs"] == r["n_pairs"]).all() and (g["inliers"] == r["inliers"]).all() and (g["ok"] == r["ok"]).all()
    if r["n_pairs"] < 3:
        assert (g["T"] == np.eye(4, dtype=np.float32)).all() and not g["ok"].any() and (g["inliers"] == 0).all()
    store.release(s)
    store.release(t)


def test_the_other_stages_are_untouched(env, oracle_mod, known):
    """gloc_reg_fpfh_batch_ids and gloc_reg_fpfh_graph_batch_ids before and after FGR calls on one handle: the same bits."""
    reg = env["reg"]
    s, t = known["yaw45_2m"]
    a, ga = reg.fpfh_batch(s, [t], stream_ids=[0]), reg.fpfh_graph_batch(s, [t])
    reg.fpfh_fgr_batch(s, [t, known["yaw90_3m"][1]], params=_prm(env["capi"]))
    P, Q, _, _ = K.pair_list("planted257", oracle_mod)
    reg.fgr_pairs(P, Q, params=_prm(env["capi"]))
    b, gb = reg.fpfh_batch(s, [t], stream_ids=[0]), reg.fpfh_graph_batch(s, [t])
    assert _same(a, b) and _same(ga, gb)
    ref = fpfh_cases.known_result("yaw45_2m", oracle_mod)
    assert int(a["n_pairs"][0]) == ref["n_pairs"] and int(a["inliers"][0]) == ref["inliers"]
