"""GPU: the ISS keypoints (gloc_scan_store_iss_saliency / _build_keypoints / _keypoints / _keypoint_fpfh) and the
keypoint-restricted FPFH registrations (gloc_reg_fpfh_batch_ids_keypoints, gloc_reg_fpfh_graph_batch_ids_keypoints) against
tests/iss_ref.py on the case table tests/iss_cases.py.

  Saliency   bit-defined: the fp64 eigenvalues and the fp32 saliency equal the restatement's on every point of every case
             (the precedent: the normals through the same Jacobi are bit-equal).
  Keypoints  the index lists equal the restatement's, with and without a target index, before and after building one.
  Batch      pair count, inliers and ok equal the restatement's, the pose within 1e-4 m / 1e-4 rad -- the bound
             test_fpfh_radius_gpu.py holds the same RANSAC and graph stages to."""
import ctypes as C

import numpy as np
import pytest

import fpfh_cases as K
import fpfh_radius_cases as RK
import fpfh_ref as F
import gicp_ref
import iss_cases as IK
import iss_ref as I
from util import bits

pytestmark = pytest.mark.gpu
STATE = 5               # GLOC_ERR_STATE (include/gloc3d.h)


@pytest.fixture(scope="module")
def env(capi, oracle_mod):
    store = capi.ScanStore()
    reg = capi.Registrar(store=store)
    yield dict(store=store, reg=reg, capi=capi)
    reg.close()
    store.close()


def _iss(capi, prm):
    return capi.default_iss_params(**prm)


def _sup(capi, s):
    if s is None:
        return None
    nr, fr, nmax, fmax, nmin = RK.SUPPORTS[s]
    return capi.default_fpfh_radius_params(normal_radius=nr, feature_radius=fr, normal_max_nn=nmax, feature_max_nn=fmax, normal_min_nn=nmin)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- I1 - I3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(IK.CASES))
def test_saliency_equals_the_restatement(env, oracle_mod, name):
    store, capi = env["store"], env["capi"]
    prm, ref = IK.CASES[name][0], IK.saliency(name, oracle_mod)
    sid = store.add(IK.cloud(name))
    sal, eig = store.iss_saliency(sid, _iss(capi, prm))
    off = np.flatnonzero((bits(sal) != bits(ref["sal"])) | (_bits64(eig) != _bits64(ref["eig"])).any(1))
    print(name, "points", len(sal), "salient", int((ref["sal"] > 0).sum()), "points off", off[:5])
    assert sal.shape == ref["sal"].shape and eig.shape == ref["eig"].shape and len(off) == 0
    store.build_target_index(sid)                                           # other chunks, the same lists, the same sums
    sal2, eig2 = store.iss_saliency(sid, _iss(capi, prm))
    assert (bits(sal2) == bits(sal)).all() and (_bits64(eig2) == _bits64(eig)).all()
    store.release(sid)


@pytest.mark.parametrize("name", list(IK.CASES))
def test_keypoints_equal_the_restatement(env, oracle_mod, name):
    store, capi = env["store"], env["capi"]
    prm, ref = IK.CASES[name][0], IK.saliency(name, oracle_mod)
    x = IK.cloud(name)
    sid = store.add(x)
    before = store.bytes()[0]
    store.build_keypoints(sid, _iss(capi, prm))
    kp = store.keypoints(sid)
    print(name, "points", len(x), "K", len(kp), "restatement", len(ref["kp"]))
    assert kp.dtype == np.uint32 and len(kp) == len(ref["kp"]) and (kp == ref["kp"]).all()
    assert store.bytes()[0] == before + 4 * len(kp)                        # (no features: no table of rows)
    store.build_target_index(sid)                                           # upload-order indices: the re-sort does not touch them
    assert (store.keypoints(sid) == ref["kp"]).all()
    store.build_keypoints(sid, _iss(capi, prm))                             # the tag came along: a no-op
    assert (store.keypoints(sid) == ref["kp"]).all() and store.bytes()[0] == before + 4 * len(kp)
    sid2 = store.add(x)                                                     # ... and built on the kd order from the start
    store.build_target_index(sid2)
    store.build_keypoints(sid2, _iss(capi, prm))
    assert (store.keypoints(sid2) == ref["kp"]).all()
    store.release(sid)
    store.release(sid2)
    assert store.bytes()[0] <= before


# ---- one keypoint set per scan, tagged; the table of rows follows the features ----------------------------------------------
def test_tags_rebuilds_and_the_gathered_table(env, oracle_mod):
    store, capi = env["store"], env["capi"]
    x = K.known_filtered("yaw0_1m")[0]
    n = len(x)
    kd, kn = I.keypoints(x, IK.ISS_SETS["default"], oracle_mod), I.keypoints(x, IK.ISS_SETS["dense"], oracle_mod)
    assert len(kd) >= 3 and len(kn) > len(kd)
    d, dense = _iss(capi, IK.ISS_SETS["default"]), _iss(capi, IK.ISS_SETS["dense"])
    sid = store.add(x)
    base = store.bytes()[0]
    for call in (lambda: store.keypoints(sid), lambda: store.keypoint_fpfh(sid)):   # no keypoints yet
        with pytest.raises(capi.GlocError) as e:
            call()
        assert e.value.code == STATE
    store.build_keypoints(sid, d)
    assert (store.keypoints(sid) == kd).all() and store.bytes()[0] == base + 4 * len(kd)
    with pytest.raises(capi.GlocError) as e:                                # keypoints, but no features to gather from
        store.keypoint_fpfh(sid)
    assert e.value.code == STATE
    store.build_fpfh(sid, 10, 16)
    fk = store.fpfh(sid)
    assert store.bytes()[0] == base + 4 * len(kd) + (12 + 132) * n
    assert (bits(store.keypoint_fpfh(sid)) == bits(fk[kd])).all()           # gathered on request ...
    full = base + (4 + 132) * len(kd) + (12 + 132) * n
    assert store.bytes()[0] == full
    store.build_keypoints(sid, d)                                           # the same again: a no-op
    assert store.bytes()[0] == full and (store.keypoints(sid) == kd).all()
    store.build_keypoints(sid, dense)                                       # other parameters: rebuilt, the table with them
    assert (store.keypoints(sid) == kn).all()
    assert store.bytes()[0] == base + (4 + 132) * len(kn) + (12 + 132) * n
    assert (bits(store.keypoint_fpfh(sid)) == bits(fk[kn])).all()
    store.build_fpfh_radius(sid, _sup(capi, "S_B"))                         # features rebuilt under the keypoints: the table goes
    fr = store.fpfh(sid)
    assert (bits(fr) != bits(fk)).any()
    assert store.bytes()[0] == base + 4 * len(kn) + (12 + 132) * n and (store.keypoints(sid) == kn).all()
    assert (bits(store.keypoint_fpfh(sid)) == bits(fr[kn])).all()           # ... and comes back from the new features
    assert store.bytes()[0] == base + (4 + 132) * len(kn) + (12 + 132) * n
    store.build_normals(sid, 10)                                            # normals of another support: features invalid, table gone
    assert store.bytes()[0] == base + 4 * len(kn) + (12 + 132) * n
    with pytest.raises(capi.GlocError) as e:
        store.keypoint_fpfh(sid)
    assert e.value.code == STATE
    store.build_fpfh(sid, 10, 16)
    assert (bits(store.keypoint_fpfh(sid)) == bits(fk[kn])).all()
    store.build_target_index(sid)                                           # the re-sort moves the features, not the table
    assert (store.keypoints(sid) == kn).all() and (bits(store.keypoint_fpfh(sid)) == bits(fk[kn])).all()
    assert (bits(store.fpfh(sid)) == bits(fk)).all()
    store.release(sid)
    assert store.bytes()[0] <= base                                         # (the list and the table went with the scan)


def test_a_rebuild_under_a_pinned_batch_is_refused(env, oracle_mod):
    store, reg, capi = env["store"], env["reg"], env["capi"]
    x = K.known_filtered("yaw0_1m")[0]
    d, dense = _iss(capi, IK.ISS_SETS["default"]), _iss(capi, IK.ISS_SETS["dense"])
    s, t = store.add(x), store.add(x)
    store.build_fpfh(s, 10, 16)
    store.build_keypoints(s, d)
    kp, rows = store.keypoints(s), store.keypoint_fpfh(s)
    reg.batch_multi_begin([s], [[t]], params=capi.default_reg_params(ransac_iters=0, icp_iters=2))
    try:
        with pytest.raises(capi.GlocError) as e:
            store.build_keypoints(s, dense)
        assert e.value.code == STATE
        store.build_keypoints(s, d)                                         # the parameters it has: a no-op, pinned or not
        store.build_keypoints(t, dense)                                     # a scan without keypoints gets them: nothing is replaced
    finally:
        reg.batch_multi_end()
    assert (store.keypoints(s) == kp).all() and (bits(store.keypoint_fpfh(s)) == bits(rows)).all()
    store.build_keypoints(s, dense)                                         # ... and free again afterwards
    assert (store.keypoints(s) == store.keypoints(t)).all()
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


@pytest.mark.parametrize("sup,iss", [(None, "default"), (None, "dense"), ("S_B", "default"), ("S_B", "dense")])
def test_batches_equal_the_restatement(env, oracle_mod, known, sup, iss):
    reg, store, capi = env["reg"], env["store"], env["capi"]
    prm, gprm, support, kprm = capi.default_fpfh_params(**K.PARAMS), capi.default_fpfh_graph_params(), _sup(capi, sup), _iss(capi, IK.ISS_SETS[iss])
    for name in K.KNOWN:
        s, t = known[name]
        ref, gref = IK.known_result(name, sup, iss, False, oracle_mod), IK.known_result(name, sup, iss, True, oracle_mod)
        g = reg.fpfh_batch(s, [t], stream_ids=[0], params=prm, support=support, keypoints=kprm)
        gg = reg.fpfh_graph_batch(s, [t], params=gprm, support=support, keypoints=kprm)
        ks, kt = IK.known_keypoints(name, iss, oracle_mod)
        assert (store.keypoints(s) == ks).all() and (store.keypoints(t) == kt).all()   # built by the call
        e, eg = gicp_ref.pose_err(ref["T"], g["T"][0]), gicp_ref.pose_err(gref["T"], gg["T"][0])
        print(sup, iss, name, "K", len(ks), len(kt), "pairs", int(g["n_pairs"][0]), ref["n_pairs"], "RANSAC inliers", int(g["inliers"][0]),
              ref["inliers"], "off by", e, "| graph inliers", int(gg["inliers"][0]), gref["inliers"], "off by", eg)
        assert int(g["n_pairs"][0]) == ref["n_pairs"] and int(g["inliers"][0]) == ref["inliers"] and bool(g["ok"][0]) == ref["ok"]
        assert e[0] <= 1e-4 and e[1] <= 1e-4
        assert int(gg["n_pairs"][0]) == gref["n_pairs"] and int(gg["inliers"][0]) == gref["inliers"] and bool(gg["ok"][0]) == gref["ok"]
        assert eg[0] <= 1e-4 and eg[1] <= 1e-4


@pytest.mark.parametrize("sup", [None, "S_B"])
def test_the_full_table_matcher_on_zeroed_rows_keeps_the_same_pairs(env, oracle_mod, known, sup):
    """I4 both ways on the device: gloc_reg_fpfh_match on the full tables with the non-keypoint rows zeroed, and on the
    gathered tables in rank space with the ranks turned into indices through the keypoint lists -- the same kept pairs, as
    many as the keypoint batch reports, and the restatement's."""
    reg, store, capi = env["reg"], env["store"], env["capi"]
    prm, kprm, support = capi.default_fpfh_params(**K.PARAMS), _iss(capi, IK.ISS_SETS["dense"]), _sup(capi, sup)
    for name in ("yaw90_0m", "yaw45_2m", "other_ab"):
        s, t = known[name]
        g = reg.fpfh_batch(s, [t], stream_ids=[0], params=prm, support=support, keypoints=kprm)
        ks, kt = store.keypoints(s), store.keypoints(t)
        fs, ft = store.fpfh(s), store.fpfh(t)
        full, _ = reg.fpfh_match(I.restrict(fs, ks), I.restrict(ft, kt), mutual=True)
        rank, _ = reg.fpfh_match(store.keypoint_fpfh(s), store.keypoint_fpfh(t), mutual=True)
        via = np.full(len(fs), F.NONE, np.uint32)
        kept = rank != F.NONE
        via[ks[kept]] = kt[rank[kept]]
        ref = IK.known_result(name, sup, "dense", False, oracle_mod)
        print(sup, name, "kept pairs", int((full != F.NONE).sum()), "in rank space", int(kept.sum()), "batch", int(g["n_pairs"][0]))
        assert (full == via).all() and int((full != F.NONE).sum()) == int(g["n_pairs"][0]) == ref["n_pairs"]
        keep = np.flatnonzero(full != F.NONE)
        assert (np.stack([keep, full[keep]], 1) == ref["pairs"]).all()


@pytest.mark.parametrize("sup,iss", [(None, "dense"), ("S_B", "default")])
def test_a_batch_is_its_single_calls(env, known, sup, iss):
    reg, capi = env["reg"], env["capi"]
    prm, gprm, support, kprm = capi.default_fpfh_params(**K.PARAMS), capi.default_fpfh_graph_params(), _sup(capi, sup), _iss(capi, IK.ISS_SETS[iss])
    s = known["yaw90_0m"][0]
    tg = [known[n][1] for n in K.KNOWN]
    streams = [3, 0, 7, 1, 3, 2, 9, 4, 5, 6]
    b = reg.fpfh_batch(s, tg, stream_ids=streams, params=prm, support=support, keypoints=kprm)
    gb = reg.fpfh_graph_batch(s, tg, params=gprm, support=support, keypoints=kprm)
    assert _same(b, reg.fpfh_batch(s, tg, stream_ids=streams, params=prm, support=support, keypoints=kprm))
    for c, (t, sid) in enumerate(zip(tg, streams)):
        one = reg.fpfh_batch(s, [t], stream_ids=[sid], params=prm, support=support, keypoints=kprm)
        gone = reg.fpfh_graph_batch(s, [t], params=gprm, support=support, keypoints=kprm)
        for full, single in ((b, one), (gb, gone)):
            assert (bits(single["T"][0]) == bits(full["T"][c])).all() and single["inliers"][0] == full["inliers"][c]
            assert single["n_pairs"][0] == full["n_pairs"][c] and single["ok"][0] == full["ok"][c]
    assert b["ok"][list(K.KNOWN).index("yaw90_0m")] and (b["n_pairs"] >= 3).all()


def test_a_target_index_does_not_change_the_result(env, known):
    reg, store, capi = env["reg"], env["store"], env["capi"]
    prm, gprm, kprm = capi.default_fpfh_params(**K.PARAMS), capi.default_fpfh_graph_params(), _iss(capi, IK.ISS_SETS["dense"])
    src, tgt, _ = K.known_filtered("yaw180_0m")
    s, t = known["yaw180_0m"]
    s2, t2 = store.add(src), store.add(tgt)
    store.build_target_index(t2)
    store.build_target_index(s2)
    assert _same(reg.fpfh_batch(s, [t], stream_ids=[0], params=prm, keypoints=kprm), reg.fpfh_batch(s2, [t2], stream_ids=[0], params=prm, keypoints=kprm))
    assert _same(reg.fpfh_graph_batch(s, [t], params=gprm, keypoints=kprm), reg.fpfh_graph_batch(s2, [t2], params=gprm, keypoints=kprm))
    store.release(s2)
    store.release(t2)


def test_keypoints_none_makes_todays_calls(env, known):
    """fpfh_batch / fpfh_graph_batch without keypoints: the bytes of the existing entries called directly, at both kinds of
    support, before and after keypoint calls on the same scans."""
    reg, capi = env["reg"], env["capi"]
    L = capi.lib()
    s, t = known["yaw45_2m"]
    prm, gprm, sup = capi.default_fpfh_params(**K.PARAMS), capi.default_fpfh_graph_params(), _sup(capi, "S_B")
    kprm = _iss(capi, IK.ISS_SETS["dense"])
    ids, sid = np.array([t], np.uint32), np.array([0], np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def direct(graph, radius):
        T, inl, npairs, ok = np.empty((1, 4, 4), np.float32), np.empty(1, np.uint32), np.empty(1, np.uint32), np.empty(1, np.int32)
        if graph and radius:
            rc = L.gloc_reg_fpfh_graph_batch_ids_radius(reg._h, s, vp(ids), 1, C.byref(gprm), C.byref(sup), vp(T), vp(inl), vp(npairs), vp(ok))
        elif graph:
            rc = L.gloc_reg_fpfh_graph_batch_ids(reg._h, s, vp(ids), 1, C.byref(gprm), vp(T), vp(inl), vp(npairs), vp(ok))
        elif radius:
            rc = L.gloc_reg_fpfh_batch_ids_radius(reg._h, s, vp(ids), 1, vp(sid), C.byref(prm), C.byref(sup), vp(T), vp(inl), vp(npairs), vp(ok))
        else:
            rc = L.gloc_reg_fpfh_batch_ids(reg._h, s, vp(ids), 1, vp(sid), C.byref(prm), vp(T), vp(inl), vp(npairs), vp(ok))
        assert rc == 0
        return dict(T=T, inliers=inl, n_pairs=npairs, ok=ok.astype(bool))

    def through_capi(graph, radius, keypoints):
        if graph:
            return reg.fpfh_graph_batch(s, [t], params=gprm, support=sup if radius else None, keypoints=keypoints)
        return reg.fpfh_batch(s, [t], stream_ids=[0], params=prm, support=sup if radius else None, keypoints=keypoints)

    for radius in (False, True):
        want = [direct(False, radius), direct(True, radius)]
        for graph in (False, True):
            assert _same(want[graph], through_capi(graph, radius, None))
            k = through_capi(graph, radius, kprm)
            assert not _same(want[graph], k) and k["n_pairs"][0] < want[graph]["n_pairs"][0]
            assert _same(want[graph], through_capi(graph, radius, None)) and _same(want[graph], direct(graph, radius))


@pytest.mark.parametrize("src,tgt", [("empty", "uniform"), ("uniform", "empty"), ("n1", "uniform"), ("plane", "uniform"), ("uniform", "plane"),
                                     ("n4", "n4")])
def test_fewer_than_three_keypoints(env, src, tgt):
    """K_src < 3, or no target keypoint: the identity, ok = 0, no pairs, no inliers -- from both entries, two jobs each."""
    store, reg, capi = env["store"], env["reg"], env["capi"]
    s, t = store.add(IK.cloud(src)), store.add(IK.cloud(tgt))
    kprm = _iss(capi, IK.D)
    for g in (reg.fpfh_batch(s, [t, t], keypoints=kprm), reg.fpfh_graph_batch(s, [t, t], keypoints=kprm)):
        assert (g["n_pairs"] == 0).all() and (g["T"] == np.eye(4, dtype=np.float32)).all() and not g["ok"].any() and (g["inliers"] == 0).all()
    store.release(s)
    store.release(t)
