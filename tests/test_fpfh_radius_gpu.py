"""GPU: the radius-support FPFH (gloc_scan_store_radius_neighbors / _build_normals_radius / _build_fpfh_radius / _spfh_radius,
gloc_reg_fpfh_batch_ids_radius, gloc_reg_fpfh_graph_batch_ids_radius) against tests/fpfh_radius_ref.py on the case table
tests/fpfh_radius_cases.py.

  Lists    bit-defined: indices, d2 bits and counts equal the float32 brute force, with and without a target index, and
           whatever the store's workspace held before.
  Normals  bit-equal to the checker's normals on those lists, zero rows (fewer than normal_min_nn entries) included.
  SPFH     integer counts: equal for every point that is not edge-flagged (none is; the CPU file holds the cap).
  FPFH     test_fpfh_gpu.py's rule: |device - restatement| <= 10 x the restatement's forward-versus-reversed difference + one
           float32 rounding of the stored value; zero rows coincide.
  Batch    pair count, inliers and ok equal the restatement's, the pose within 1e-4 m / 1e-4 rad (the project's bound)."""
import ctypes as C

import numpy as np
import pytest

import fpfh_cases as K
import fpfh_radius_cases as RK
import fpfh_radius_ref as R
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


def _sup(capi, s):
    nr, fr, nmax, fmax, nmin = RK.SUPPORTS[s] if isinstance(s, str) else s
    return capi.default_fpfh_radius_params(normal_radius=nr, feature_radius=fr, normal_max_nn=nmax, feature_max_nn=fmax, normal_min_nn=nmin)


def _lists_equal(got, ref):
    return (got[0] == ref[0]).all() and (bits(got[1]) == bits(ref[1])).all() and (got[2] == ref[2]).all()


# ---- the search ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,r,max_nn", RK.LISTS)
def test_radius_neighbors_equal_the_restatement(env, name, r, max_nn):
    store = env["store"]
    ref = RK.lists(name, r, max_nn)
    sid = store.add(RK.cloud(name))
    got = store.radius_neighbors(sid, r, max_nn)
    bad = np.flatnonzero((got[0] != ref[0]).any(1) | (got[2] != ref[2]))
    print(name, r, max_nn, "points", len(ref[2]), "count max", int(ref[2].max(initial=0)), "truncated", int((ref[2] > max_nn).sum()), "rows off", bad[:5])
    assert got[0].shape == ref[0].shape and _lists_equal(got, ref)
    store.build_target_index(sid)                                           # the kd order cuts other chunks: the same lists
    assert _lists_equal(store.radius_neighbors(sid, r, max_nn), ref)
    store.release(sid)


def test_one_store_through_big_small_lattice_big(capi):
    """The workspace of a store is grown on demand and reused: a search after a wider, a narrower or a larger one is the
    search of a fresh store."""
    store = capi.ScanStore()
    seq = [("a", 1.0, 100), ("n4", 2.5, 128), ("lattice", 2.0, 16), ("a", 1.0, 100), ("uniform", 1.5, 128), ("a_odd", 0.5, 30)]
    ids = {}
    for name, r, max_nn in seq:
        if name not in ids:
            ids[name] = store.add(RK.cloud(name))
        assert _lists_equal(store.radius_neighbors(ids[name], r, max_nn), RK.lists(name, r, max_nn)), name
    store.close()


# ---- normals and features -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sup", RK.FEATURES)
def test_normals_spfh_and_fpfh_equal_the_restatement(env, oracle_mod, name, sup):
    store, capi = env["store"], env["capi"]
    xyz = RK.cloud(name)
    n = len(xyz)
    ref = RK.features(name, sup, oracle_mod)
    nr, fr, nmax, fmax, nmin = RK.SUPPORTS[sup]
    prm = _sup(capi, sup)
    sid = store.add(xyz)
    before = store.bytes()[0]
    store.build_normals_radius(sid, nr, nmax, nmin)
    assert store.bytes()[0] == before + 12 * n
    nrm = store.normals(sid)
    assert (bits(nrm) == bits(ref["nrm"])).all()
    store.build_fpfh_radius(sid, prm)
    assert store.bytes()[0] == before + (12 + 132) * n
    store.build_fpfh_radius(sid, prm)                                      # at most once
    assert store.bytes()[0] == before + (12 + 132) * n
    assert (bits(store.normals(sid)) == bits(ref["nrm"])).all()             # (the features kept the normals they found)
    feat = store.fpfh(sid)
    counts, used = store.spfh_radius(sid, fr, fmax)
    if n == 0:
        assert feat.shape == (0, 33)
        store.release(sid)
        return
    chk = ~ref["flagged"]
    assert (used[chk] == ref["used"][chk]).all()
    assert (counts[chk] == ref["counts"][chk]).all()
    idx = ref["idx"]
    inside = idx < n
    out = (ref["flagged"][np.where(inside, idx, 0)] & inside).any(1) | ref["flagged"]
    rev = F.fpfh(ref["counts"], ref["used"], ref["idx"], ref["d2"], order="reversed")
    floor = np.abs(rev - ref["feat64"])
    tol = 10.0 * floor + np.abs(ref["feat64"]) * 2.0 ** -24
    err = np.abs(feat.astype(np.float64) - ref["feat64"])
    zero_dev, zero_ref = ~(feat != 0).any(1), ~(ref["feat64"] != 0).any(1)
    print(name, sup, "points", n, "left out", int(out.sum()), "used max", int(ref["used"].max()), "floor max", floor[~out].max(initial=0.0),
          "device error max", err[~out].max(initial=0.0), "in units of the tolerance", (err[~out] / np.maximum(tol[~out], 1e-300)).max(initial=0.0),
          "zero rows", int(zero_ref.sum()))
    assert (zero_dev[~out] == zero_ref[~out]).all()
    assert (err[~out] <= tol[~out]).all()
    after = store.bytes()[0]
    store.release(sid)
    assert store.bytes()[0] <= after - (12 + 132) * n


# ---- one set per scan, tagged with its support --------------------------------------------------------------------------
def test_k_then_radius_then_k_each_equals_a_fresh_scan(env, oracle_mod):
    store, capi = env["store"], env["capi"]
    xyz = RK.cloud("a_vox")
    fresh_k, fresh_r = store.add(xyz), store.add(xyz)
    store.build_fpfh(fresh_k, 10, 16)
    store.build_fpfh_radius(fresh_r, _sup(capi, "S_B"))
    fk, nk, fr, nr = store.fpfh(fresh_k), store.normals(fresh_k), store.fpfh(fresh_r), store.normals(fresh_r)
    assert (fk != fr).any() and (bits(nk) != bits(nr)).any()
    sid = store.add(xyz)
    live = None
    for step in ("k", "radius", "k", "radius", "other radius"):
        if step == "k":
            store.build_fpfh(sid, 10, 16)
            assert (bits(store.fpfh(sid)) == bits(fk)).all() and (bits(store.normals(sid)) == bits(nk)).all()
        elif step == "radius":
            store.build_fpfh_radius(sid, _sup(capi, "S_B"))
            assert (bits(store.fpfh(sid)) == bits(fr)).all() and (bits(store.normals(sid)) == bits(nr)).all()
        else:                                                               # the same normals, another feature support
            store.build_fpfh_radius(sid, _sup(capi, (0.75, 1.0, 32, 48, 5)))
            assert (bits(store.normals(sid)) == bits(nr)).all() and (bits(store.fpfh(sid)) != bits(fr)).any()
            ref = R.features(xyz, (0.75, 1.0, 32, 48, 5), oracle_mod)
            assert np.allclose(store.fpfh(sid), ref["feat"], rtol=1e-6, atol=1e-5)
        live = live or store.bytes()[0]
        assert store.bytes()[0] == live                                     # rebuilt in the same two allocations
    # radius normals alone drop the k features' validity: the k request after them rebuilds both
    store.build_normals_radius(sid, 0.75, 32, 5)
    store.build_fpfh(sid, 10, 16)
    assert (bits(store.fpfh(sid)) == bits(fk)).all()
    for s in (fresh_k, fresh_r, sid):
        store.release(s)


def test_normals_alone_k_radius_k_radius_each_equal_a_fresh_scan(env):
    """The normals-only transitions: k -> radius -> k -> the radius with another min_nn on one scan.  After each step the
    normals are, bit for bit, those of a fresh scan built directly from that support (which the tests above tie to the
    restatement), in the allocation the first step made; the features asked for afterwards are the fresh k scan's.  An
    empty scan takes the same calls and allocates nothing."""
    store = env["store"]
    xyz = RK.cloud("a_vox")
    nr, _, nmax, _, nmin = RK.S_A
    steps = [("k", 10), ("radius", nmin), ("k", 10), ("radius", nmin + 3)]

    def build(s, step):
        if step[0] == "k":
            store.build_normals(s, step[1])
        else:
            store.build_normals_radius(s, nr, nmax, step[1])

    fresh = {}
    for step in steps[1:]:
        fresh[step] = store.add(xyz)
        build(fresh[step], step)
    want = {step: store.normals(f) for step, f in fresh.items()}
    differ = [(bits(want[a]) != bits(want[b])).any() for a, b in ((steps[0], steps[1]), (steps[0], steps[3]), (steps[1], steps[3]))]
    print("points", len(xyz), "the three supports give three sets of normals", differ)
    assert all(differ)
    store.build_fpfh(fresh[steps[0]], 10, 16)
    fk = store.fpfh(fresh[steps[0]])
    sid, empty = store.add(xyz), store.add(RK.cloud("empty"))
    before = store.bytes()[0]
    for step in steps:
        build(sid, step)
        build(empty, step)
        assert store.bytes()[0] == before + 12 * len(xyz)
        assert (bits(store.normals(sid)) == bits(want[step])).all(), step
        assert store.normals(empty).shape == (0, 3)
    store.build_fpfh(sid, 10, 16)
    store.build_fpfh(empty, 10, 16)
    assert store.bytes()[0] == before + (12 + 132) * len(xyz)
    assert (bits(store.fpfh(sid)) == bits(fk)).all() and (bits(store.normals(sid)) == bits(want[steps[0]])).all()
    assert store.fpfh(empty).shape == (0, 33)
    for s in [sid, empty] + list(fresh.values()):
        store.release(s)


def test_features_follow_the_target_index_with_their_tags(env):
    store, capi = env["store"], env["capi"]
    prm = _sup(capi, "S_RAW")
    sid = store.add(RK.cloud("a_odd"))
    store.build_fpfh_radius(sid, prm)
    f0, n0 = store.fpfh(sid), store.normals(sid)
    live = store.bytes()[0]
    store.build_target_index(sid)
    assert (bits(store.fpfh(sid)) == bits(f0)).all() and (bits(store.normals(sid)) == bits(n0)).all()
    store.build_fpfh_radius(sid, prm)                                      # the tags came along: still a no-op
    assert store.bytes()[0] == live and (bits(store.fpfh(sid)) == bits(f0)).all()
    sid2 = store.add(RK.cloud("a_odd"))
    store.build_target_index(sid2)
    store.build_fpfh_radius(sid2, prm)
    assert (bits(store.fpfh(sid2)) == bits(f0)).all()
    store.release(sid)
    store.release(sid2)


def test_refinements_use_the_radius_normals(env, oracle_mod):
    """p2l / gicp on scans that carry radius normals run on them: the normals are not rebuilt, and the generalized ICP
    system is the restatement's on THOSE normals (10 x its own order / inverse floor, test_gicp_gpu.py's rule), which the
    system on k-NN normals is not."""
    store, reg, capi = env["store"], env["reg"], env["capi"]
    src, tgt, truth = K.known_filtered("yaw0_1m")
    nr, _, nmax, _, nmin = RK.S_A
    s, t, sk, tk = store.add(src), store.add(tgt), store.add(src), store.add(tgt)
    store.build_normals_radius(s, nr, nmax, nmin)
    store.build_normals_radius(t, nr, nmax, nmin)
    ns, nt = store.normals(s), store.normals(t)
    T = np.asarray(truth, np.float32)
    H, g, s2, cnt = reg.gicp_system(s, t, T)
    Hk, gk, _, _ = reg.gicp_system(sk, tk, T)                               # (k = 10 normals built by the call)
    assert (bits(store.normals(s)) == bits(ns)).all() and (bits(store.normals(t)) == bits(nt)).all()
    rs = [R.radius_lists(x, nr, nmax) for x in (src, tgt)]
    ref_ns, ref_nt = (R.normals(x, l[0], l[2], nmax, nmin, oracle_mod) for x, l in zip((src, tgt), rs))
    assert (bits(ns) == bits(ref_ns)).all() and (bits(nt) == bits(ref_nt)).all()
    nn = lambda p, q: oracle_mod.nn3(p, q, grid=True)  # noqa: E731
    prm = capi.default_gicp_params()
    p, q, a, b = gicp_ref.pairs(src, ns, tgt, nt, T, nn, prm.max_corr_dist)
    Rm = gicp_ref.rotation(T)
    ref = gicp_ref.system_of_pairs(p, q, a, b, Rm, prm.plane_eps)
    rev = gicp_ref.system_of_pairs(p, q, a, b, Rm, prm.plane_eps, order="reversed")
    adj = gicp_ref.system_of_pairs(p, q, a, b, Rm, prm.plane_eps, how="adj")
    scale = max(np.abs(ref[0]).max(), np.abs(ref[1]).max(), ref[2])
    rel = lambda x, y: max(np.abs(x[0] - y[0]).max(), np.abs(x[1] - y[1]).max(), abs(x[2] - y[2])) / scale  # noqa: E731
    tol = 10 * max(rel(ref, rev), rel(ref, adj))
    err, err_k = rel((H, g, s2), ref), max(np.abs(Hk - ref[0]).max(), np.abs(gk - ref[1]).max()) / scale
    print("pairs", cnt, ref[3], "tolerance %.3e, device on the radius normals %.3e, on k-NN normals %.3e" % (tol, err, err_k))
    assert cnt == ref[3] and err <= tol and err_k > 100 * tol
    out = reg.p2l_batch(s, [t], init_T=T[None])
    assert np.isfinite(np.asarray(out[0])).all()
    assert (bits(store.normals(s)) == bits(ns)).all() and (bits(store.normals(t)) == bits(nt)).all()
    for x in (s, t, sk, tk):
        store.release(x)


def test_a_rebuild_under_a_pinned_batch_is_refused(env):
    store, reg, capi = env["store"], env["reg"], env["capi"]
    s, t = store.add(RK.cloud("a_vox")), store.add(RK.cloud("a_vox"))
    store.build_fpfh_radius(s, _sup(capi, "S_B"))
    store.build_fpfh(t, 10, 16)
    fs, ft = store.fpfh(s), store.fpfh(t)
    reg.batch_multi_begin([s], [[t]], params=capi.default_reg_params(ransac_iters=0, icp_iters=2))
    try:
        for call in (lambda: store.build_fpfh_radius(s, _sup(capi, "S_A")), lambda: store.build_fpfh(s, 10, 16),
                     lambda: store.build_fpfh_radius(t, _sup(capi, "S_B")), lambda: store.build_normals_radius(t, 1.0, 30, 5),
                     lambda: store.build_normals(s, 10)):
            with pytest.raises(capi.GlocError) as e:
                call()
            assert e.value.code == 5
        store.build_fpfh_radius(s, _sup(capi, "S_B"))                       # the support it has: a no-op, pinned or not
        store.build_fpfh(t, 10, 16)
    finally:
        reg.batch_multi_end()
    assert (bits(store.fpfh(s)) == bits(fs)).all() and (bits(store.fpfh(t)) == bits(ft)).all()
    store.build_fpfh_radius(s, _sup(capi, "S_A"))                           # ... and free again afterwards
    store.release(s)
    store.release(t)


# ---- the batch entries --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def known(env):
    ids = {}
    for name in K.KNOWN:
        src, tgt, _ = K.known_filtered(name)
        ids[name] = (env["store"].add(src), env["store"].add(tgt))
    return ids


def _same(a, b):
    return all((bits(a[k].astype(np.float32)) == bits(b[k].astype(np.float32))).all() for k in ("T", "inliers", "n_pairs", "ok"))


@pytest.mark.parametrize("sup", RK.KNOWN_SUPPORTS)
def test_batches_equal_the_restatement(env, oracle_mod, known, sup):
    reg, capi = env["reg"], env["capi"]
    prm, gprm, support = capi.default_fpfh_params(**K.PARAMS), capi.default_fpfh_graph_params(), _sup(capi, sup)
    for name in K.KNOWN:
        s, t = known[name]
        ref, gref = RK.known_result(name, sup, oracle_mod), RK.known_graph_result(name, sup, oracle_mod)
        g = reg.fpfh_batch(s, [t], stream_ids=[0], params=prm, support=support)
        gg = reg.fpfh_graph_batch(s, [t], params=gprm, support=support)
        e, eg = gicp_ref.pose_err(ref["T"], g["T"][0]), gicp_ref.pose_err(gref["T"], gg["T"][0])
        print(sup, name, "pairs", int(g["n_pairs"][0]), ref["n_pairs"], "RANSAC inliers", int(g["inliers"][0]), ref["inliers"], "off by", e,
              "| graph inliers", int(gg["inliers"][0]), gref["inliers"], "off by", eg)
        assert int(g["n_pairs"][0]) == ref["n_pairs"] and int(g["inliers"][0]) == ref["inliers"] and bool(g["ok"][0]) == ref["ok"]
        assert e[0] <= 1e-4 and e[1] <= 1e-4
        assert int(gg["n_pairs"][0]) == gref["n_pairs"] and int(gg["inliers"][0]) == gref["inliers"] and bool(gg["ok"][0]) == gref["ok"]
        assert eg[0] <= 1e-4 and eg[1] <= 1e-4
    located = RK.known_answer_cases(sup, oracle_mod)
    assert located and "yaw90_0m" in located and "yaw180_0m" in located
    for name in located:                                                    # held to the cases the restatement locates
        s, t = known[name]
        g = reg.fpfh_batch(s, [t], stream_ids=[0], params=prm, support=support)
        err = K.pose_error(g["T"][0], K.known_filtered(name)[2])
        assert g["ok"][0] and err[0] <= K.OK_T and err[1] <= K.OK_R


@pytest.mark.parametrize("sup", RK.KNOWN_SUPPORTS)
def test_a_batch_is_its_single_calls(env, known, sup):
    reg, capi = env["reg"], env["capi"]
    prm, gprm, support = capi.default_fpfh_params(**K.PARAMS), capi.default_fpfh_graph_params(), _sup(capi, sup)
    s = known["yaw90_3m"][0]
    tg = [known[n][1] for n in K.KNOWN]
    streams = [3, 0, 7, 1, 3, 2, 9, 4, 5, 6]
    b = reg.fpfh_batch(s, tg, stream_ids=streams, params=prm, support=support)
    gb = reg.fpfh_graph_batch(s, tg, params=gprm, support=support)
    assert _same(b, reg.fpfh_batch(s, tg, stream_ids=streams, params=prm, support=support))
    for c, (t, sid) in enumerate(zip(tg, streams)):
        one = reg.fpfh_batch(s, [t], stream_ids=[sid], params=prm, support=support)
        gone = reg.fpfh_graph_batch(s, [t], params=gprm, support=support)
        for full, single in ((b, one), (gb, gone)):
            assert (bits(single["T"][0]) == bits(full["T"][c])).all() and single["inliers"][0] == full["inliers"][c]
            assert single["n_pairs"][0] == full["n_pairs"][c] and single["ok"][0] == full["ok"][c]
    assert b["ok"][list(K.KNOWN).index("yaw90_3m")]


def test_support_none_makes_todays_calls(env, known):
    """fpfh_batch / fpfh_graph_batch without a support: the bits of gloc_reg_fpfh_batch_ids / _graph_batch_ids called
    directly, before and after radius calls on the same scans (which rebuild their features in between)."""
    reg, capi = env["reg"], env["capi"]
    L = capi.lib()
    s, t = known["yaw45_2m"]
    prm, gprm = capi.default_fpfh_params(**K.PARAMS), capi.default_fpfh_graph_params()
    ids, sid = np.array([t], np.uint32), np.array([0], np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def direct(graph):
        T, inl, npairs, ok = np.empty((1, 4, 4), np.float32), np.empty(1, np.uint32), np.empty(1, np.uint32), np.empty(1, np.int32)
        if graph:
            rc = L.gloc_reg_fpfh_graph_batch_ids(reg._h, s, vp(ids), 1, C.byref(gprm), vp(T), vp(inl), vp(npairs), vp(ok))
        else:
            rc = L.gloc_reg_fpfh_batch_ids(reg._h, s, vp(ids), 1, vp(sid), C.byref(prm), vp(T), vp(inl), vp(npairs), vp(ok))
        assert rc == 0
        return dict(T=T, inliers=inl, n_pairs=npairs, ok=ok.astype(bool))

    d, dg = direct(False), direct(True)
    assert _same(d, reg.fpfh_batch(s, [t], stream_ids=[0], params=prm)) and _same(dg, reg.fpfh_graph_batch(s, [t], params=gprm))
    r = reg.fpfh_batch(s, [t], stream_ids=[0], params=prm, support=_sup(capi, "S_B"))
    assert not _same(d, r)
    assert _same(d, reg.fpfh_batch(s, [t], stream_ids=[0], params=prm, support=None))
    assert _same(dg, reg.fpfh_graph_batch(s, [t], params=gprm, support=None))


@pytest.mark.parametrize("src,tgt", [("empty", "a_vox"), ("a_vox", "empty"), ("n1", "a_vox"), ("zn", "a_vox"), ("n64", "n64")])
def test_fewer_than_three_pairs(env, src, tgt):
    store, capi = env["store"], env["capi"]
    s, t = store.add(RK.cloud(src)), store.add(RK.cloud(tgt))
    for g in (env["reg"].fpfh_batch(s, [t, t], support=_sup(capi, "S_A")), env["reg"].fpfh_graph_batch(s, [t, t], support=_sup(capi, "S_A"))):
        assert (g["n_pairs"] == 0).all() and (g["T"] == np.eye(4, dtype=np.float32)).all() and not g["ok"].any() and (g["inliers"] == 0).all()
    store.release(s)
    store.release(t)
