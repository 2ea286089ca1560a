"""GPU: the FPFH feature-based global registration (gloc_scan_store_build_fpfh / _spfh, gloc_reg_fpfh_match,
gloc_reg_fpfh_batch_ids) against the float64 restatement tests/fpfh_ref.py on the case table tests/fpfh_cases.py.

  SPFH     integer counts: equal to the restatement for every point that is not edge-flagged.
  FPFH     |device - restatement| <= 10 x the restatement's forward-versus-reversed difference + one float32 rounding of the
           stored value (2^-24 relative); zero rows in one are zero rows in the other; points with an edge-flagged list
           entry are left out (their neighbours' counts may legitimately differ), which the CPU file's 1 % cap bounds.
  Matcher  bit-defined: indices and d2 bits equal the float32 statement.
  Batch    pair count, inliers and ok equal the restatement's; the pose within 1e-4 m / 1e-4 rad (the project's parity
           rule for RANSAC poses: the refit's fp64 moments are reduced in another order, the pose comes back in float32)."""
import numpy as np
import pytest

import fpfh_cases as K
import fpfh_ref as F
import gicp_ref
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
    return capi.default_fpfh_params(**dict({k: v for k, v in K.PARAMS.items()}, **over))


# ---- features ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.CLOUDS)
def test_spfh_and_fpfh_equal_the_restatement(env, oracle_mod, name):
    store = env["store"]
    xyz = K.cloud(name)
    ref = K.features(name, oracle_mod)
    sid = store.add(xyz)
    before = store.bytes()[0]
    store.build_fpfh(sid, K.PARAMS["normal_k"], K.PARAMS["feature_k"])
    assert store.bytes()[0] == before + (12 + 132) * len(xyz)
    store.build_fpfh(sid, K.PARAMS["normal_k"], K.PARAMS["feature_k"])          # at most once
    assert store.bytes()[0] == before + (12 + 132) * len(xyz)
    feat = store.fpfh(sid)
    counts, used = store.spfh(sid, K.PARAMS["feature_k"])
    n = len(xyz)
    if n == 0:
        assert feat.shape == (0, 33)
        store.release(sid)
        return
    assert (bits(store.normals(sid)) == bits(ref["nrm"])).all()             # (the restatement starts from the same normals)
    # SPFH: exact off the edge flags
    chk = ~ref["flagged"]
    assert (used[chk] == ref["used"][chk]).all()
    assert (counts[chk] == ref["counts"][chk]).all()
    print(name, "points", n, "edge-flagged", int(ref["flagged"].sum()), "SPFH rows differing among the flagged", int((counts != ref["counts"]).any(1).sum()))
    # FPFH: left out -- every point with an edge-flagged list entry
    idx = ref["idx"]
    inside = idx < n
    out = (ref["flagged"][np.where(inside, idx, 0)] & inside).any(1) | ref["flagged"]
    rev = F.fpfh(ref["counts"], ref["used"], ref["idx"], ref["d2"], order="reversed")
    floor = np.abs(rev - ref["feat64"])
    tol = 10.0 * floor + np.abs(ref["feat64"]) * 2.0 ** -24
    err = np.abs(feat.astype(np.float64) - ref["feat64"])
    zero_dev, zero_ref = ~(feat != 0).any(1), ~(ref["feat64"] != 0).any(1)
    print(name, "left out", int(out.sum()), "floor max", floor[~out].max(initial=0.0), "device error max", err[~out].max(initial=0.0),
          "in units of the tolerance", (err[~out] / np.maximum(tol[~out], 1e-300)).max(initial=0.0), "zero rows", int(zero_ref.sum()))
    assert (zero_dev[~out] == zero_ref[~out]).all()
    assert (err[~out] <= tol[~out]).all()
    after = store.bytes()[0]
    store.release(sid)
    assert store.bytes()[0] <= after - (12 + 132) * n                        # features and normals go with the scan


def test_features_follow_the_target_index(env, oracle_mod):
    """The kd re-sort moves the rows with the points: the reported features are the same bits."""
    store = env["store"]
    sid = store.add(K.cloud("a_odd"))
    store.build_fpfh(sid)
    f0 = store.fpfh(sid)
    store.build_target_index(sid)
    assert (bits(store.fpfh(sid)) == bits(f0)).all()
    sid2 = store.add(K.cloud("a_odd"))
    store.build_target_index(sid2)
    store.build_fpfh(sid2)
    assert (bits(store.fpfh(sid2)) == bits(f0)).all()
    live = store.bytes()[0]
    store.build_fpfh(sid2, 10, 8)                                             # another feature_k: rebuilt in the same allocation
    f8 = store.fpfh(sid2)
    assert store.bytes()[0] == live and (f8 != f0).any()
    assert np.allclose(f8, F.features(K.cloud("a_odd"), 10, 8, oracle_mod)["feat"], rtol=1e-6, atol=1e-5)
    store.release(sid)
    store.release(sid2)


# ---- matcher ----------------------------------------------------------------------------------------------------------
def _rows(rng, n):
    """Feature-like rows: three sub-histograms of sum 100 with a few occupied bins."""
    x = rng.random((n, 3, 11)) ** 4
    x = 100.0 * x / x.sum(2, keepdims=True)
    return np.ascontiguousarray(x.reshape(n, 33), np.float32)


def _check_match(env, a, b):
    for mutual in (False, True):
        gi, gd = env["reg"].fpfh_match(a, b, mutual=mutual)
        ri, rd = F.match(a, b, mutual=mutual)
        assert (gi == ri).all(), (mutual, np.flatnonzero(gi != ri)[:5])
        assert (bits(gd) == bits(rd)).all()


@pytest.mark.parametrize("n_src", (1, 63, 64, 65, 257))
def test_matcher_shapes(env, n_src):
    tile = env["capi"].FPFH_MATCH_TILE
    rng = np.random.default_rng(100 + n_src)
    a = _rows(rng, n_src)
    for n_tgt in (1, tile - 1, tile, tile + 1, 3 * tile + 5):
        _check_match(env, a, _rows(rng, n_tgt))


def test_matcher_content(env):
    tile = env["capi"].FPFH_MATCH_TILE
    rng = np.random.default_rng(7)
    a, b = _rows(rng, 300), _rows(rng, 2 * tile + 9)
    b[tile + 3] = b[5]                                        # duplicated target rows, across tiles: the lower index wins
    b[tile - 1] = b[tile]
    a[10] = b[5]
    a[11] = b[tile]
    b[::7] = 0.0                                              # zero rows on either side are skipped
    a[::5] = 0.0
    _check_match(env, a, b)
    gi, gd = env["reg"].fpfh_match(a, b, mutual=False)
    assert (gi[::5] == F.NONE).all() and np.isinf(gd[::5]).all() and not np.isin(gi, np.arange(0, len(b), 7)).any()
    if 10 % 5 and 5 % 7:
        assert gi[10] == 5 and gd[10] == 0
    # many exact ties: rows drawn from a handful of prototypes
    protos = _rows(rng, 6)
    _check_match(env, protos[rng.integers(0, 6, 257)], protos[rng.integers(0, 6, 3 * tile + 5)])
    # all rows zero: every output is "none"
    z = np.zeros((65, 33), np.float32)
    for x, y in ((z, b), (a, np.zeros((tile + 1, 33), np.float32)), (z, z)):
        for mutual in (False, True):
            gi, gd = env["reg"].fpfh_match(x, y, mutual=mutual)
            assert (gi == F.NONE).all() and np.isinf(gd).all()
    gi, _ = env["reg"].fpfh_match(a, np.zeros((0, 33), np.float32))
    assert (gi == F.NONE).all()


def test_matcher_on_computed_features(env, oracle_mod):
    """... and on real features, where near-ties are common (planar neighbourhoods give equal rows)."""
    fa, fb = K.features("a_vox", oracle_mod)["feat"], K.features("a_odd", oracle_mod)["feat"]
    _check_match(env, fa, fb)


# ---- batch ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def known(env, oracle_mod):
    """The known-answer pairs resident: name -> (source id, target id)."""
    ids = {}
    for name in K.KNOWN:
        src, tgt, _ = K.known_filtered(name)
        ids[name] = (env["store"].add(src), env["store"].add(tgt))
    return ids


@pytest.mark.parametrize("name", tuple(K.KNOWN))
def test_batch_equals_the_restatement(env, oracle_mod, known, name):
    ref = K.known_result(name, oracle_mod)
    s, t = known[name]
    g = env["reg"].fpfh_batch(s, [t], stream_ids=[0], params=_prm(env["capi"]))
    e = gicp_ref.pose_err(ref["T"], g["T"][0])
    print(name, "pairs", int(g["n_pairs"][0]), ref["n_pairs"], "inliers", int(g["inliers"][0]), ref["inliers"], "ok", bool(g["ok"][0]), ref["ok"],
          "pose off the restatement by", e)
    assert int(g["n_pairs"][0]) == ref["n_pairs"]
    assert int(g["inliers"][0]) == ref["inliers"]
    assert bool(g["ok"][0]) == ref["ok"]
    assert e[0] <= 1e-4 and e[1] <= 1e-4


def test_batch_is_its_single_calls_and_repeatable(env, oracle_mod, known):
    reg, store = env["reg"], env["store"]
    s = known["yaw90_3m"][0]
    tg = [known[n][1] for n in ("yaw90_3m", "yaw0_1m", "yaw170_1m", "other_ab")] + [known["yaw90_3m"][1]]
    streams = [3, 0, 7, 1, 3]
    prm = _prm(env["capi"])
    b1 = reg.fpfh_batch(s, tg, stream_ids=streams, params=prm)
    b2 = reg.fpfh_batch(s, tg, stream_ids=streams, params=prm)
    for k in ("T", "inliers", "n_pairs", "ok"):
        assert (bits(b1[k].astype(np.float32)) == bits(b2[k].astype(np.float32))).all()
    for c, (t, sid) in enumerate(zip(tg, streams)):
        one = reg.fpfh_batch(s, [t], stream_ids=[sid], params=prm)
        assert (bits(one["T"][0]) == bits(b1["T"][c])).all() and one["inliers"][0] == b1["inliers"][c] and one["n_pairs"][0] == b1["n_pairs"][c]
        assert one["ok"][0] == b1["ok"][c]
    assert (bits(b1["T"][0]) == bits(b1["T"][4])).all()
    # the default stream ids are 0 .. n - 1
    d = reg.fpfh_batch(s, tg[:2], params=prm)
    e = reg.fpfh_batch(s, tg[:2], stream_ids=[0, 1], params=prm)
    assert (bits(d["T"]) == bits(e["T"])).all()
    # a target index on the target, then on the source: the same bits
    src, tgt, _ = K.known_filtered("yaw90_3m")
    s2, t2 = store.add(src), store.add(tgt)
    store.build_target_index(t2)
    k1 = reg.fpfh_batch(s2, [t2], stream_ids=[3], params=prm)
    store.build_target_index(s2)
    k2 = reg.fpfh_batch(s2, [t2], stream_ids=[3], params=prm)
    for k in (k1, k2):
        assert (bits(k["T"][0]) == bits(b1["T"][0])).all() and k["inliers"][0] == b1["inliers"][0] and k["n_pairs"][0] == b1["n_pairs"][0]
    # not mutual, every hypothesis scored: still the restatement's counts
    prm2 = _prm(env["capi"], mutual=0, ransac_confidence=0.0, ransac_iters=600, min_inlier_ratio=0.2)
    g = reg.fpfh_batch(s, [tg[0]], stream_ids=[5], params=prm2)
    r = F.register(src, tgt, oracle_mod, stream_id=5, **dict(K.PARAMS, mutual=0, ransac_confidence=0.0, ransac_iters=600, min_inlier_ratio=0.2))
    assert int(g["n_pairs"][0]) == r["n_pairs"] and int(g["inliers"][0]) == r["inliers"] and bool(g["ok"][0]) == r["ok"]
    assert max(gicp_ref.pose_err(r["T"], g["T"][0])) <= 1e-4


@pytest.mark.parametrize("src,tgt", [("empty", "a_vox"), ("a_vox", "empty"), ("n1", "a_vox"), ("zn", "a_vox"), ("a_vox", "zn"), ("n4", "n4")])
def test_fewer_than_three_pairs(env, oracle_mod, src, tgt):
    store = env["store"]
    s, t = store.add(K.cloud(src)), store.add(K.cloud(tgt))
    g = env["reg"].fpfh_batch(s, [t, t], params=_prm(env["capi"]))
    r = F.register(K.cloud(src), K.cloud(tgt), oracle_mod, **K.PARAMS)
    assert r["n_pairs"] < 3 or (src, tgt) == ("n4", "n4")
    assert (g["n_pairs"] == r["n_pairs"]).all()
    if r["n_pairs"] < 3:
        assert (g["T"] == np.eye(4, dtype=np.float32)).all() and not g["ok"].any() and (g["inliers"] == 0).all()
    else:
        assert (g["inliers"] == r["inliers"]).all() and (g["ok"] == r["ok"]).all()
    store.release(s)
    store.release(t)


# ---- known answers ----------------------------------------------------------------------------------------------------
def test_known_answer_cases_are_located(env, oracle_mod, known):
    names = K.known_answer_cases(oracle_mod)
    assert len(names) >= 3
    for name in names:
        s, t = known[name]
        g = env["reg"].fpfh_batch(s, [t], stream_ids=[0], params=_prm(env["capi"]))
        err = K.pose_error(g["T"][0], K.known_filtered(name)[2])
        print(name, "device pose off ground truth by %.3f m, %.3f deg" % err, "inliers", int(g["inliers"][0]), "of", int(g["n_pairs"][0]))
        assert g["ok"][0] and err[0] <= K.OK_T and err[1] <= K.OK_R


def test_the_170_degree_start_refines(env, oracle_mod, known):
    """The located pose is a start generalized ICP can use: ten passes from the device's pose end within 10 x the error the
    restatement's pose reaches through the generalized ICP restatement."""
    name = "yaw170_1m"
    assert name in K.known_answer_cases(oracle_mod)
    src, tgt, truth = K.known_filtered(name)
    s, t = known[name]
    capi = env["capi"]
    g = env["reg"].fpfh_batch(s, [t], stream_ids=[0], params=_prm(capi))
    T, _, _, status = env["reg"].gicp_batch(s, [t], init_T=g["T"], params=capi.default_gicp_params(max_iters=10))
    ns, nt = F.normals(src, 10, oracle_mod), F.normals(tgt, 10, oracle_mod)
    nn = lambda p, q: oracle_mod.nn3(p, q, grid=True)  # noqa: E731
    r = gicp_ref.align(src, ns, tgt, nt, nn, init_T=K.known_result(name, oracle_mod)["T"].astype(np.float32), max_iters=10)
    e_ref, e_dev = gicp_ref.pose_err(truth, r["T"]), gicp_ref.pose_err(truth, T[0])
    print("restatement through gicp_ref: %.4g m %.4g rad; device through gicp_batch: %.4g m %.4g rad" % (e_ref + e_dev))
    assert e_dev[0] <= 10.0 * e_ref[0] and e_dev[1] <= 10.0 * e_ref[1]
