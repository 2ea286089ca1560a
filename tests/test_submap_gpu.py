"""GPU: local submaps (gloc_scan_store_add_submap[s]) against the numpy restatement tests/submap_ref.py -- BITWISE: the point
count, the order and the fp32 bits of every coordinate --, the batch call against the single call, the errors, the result
as an ordinary resident scan, and the detector's build_submaps()."""
import ctypes as C

import numpy as np
import pytest

import submap_cases as cases
import submap_ref as ref
from util import bits

pytestmark = pytest.mark.gpu
EYE = np.eye(4, dtype=np.float32)
INFO_KEYS = ("points_in", "points_used", "cells", "kept")


@pytest.fixture(scope="module")
def env(capi):
    """Three casts of about 3 000 points from poses that differ in yaw, pitch and translation, resident in one store."""
    from gloc3d_amd import synth
    world = synth.make_world(7)
    poses = [synth.se3(0.0, (0.0, 0.0, 0.0)), synth.se3(7.0, (0.9, -0.3, 0.05), pitch_deg=1.5),
             synth.se3(-11.0, (-0.7, 0.6, -0.04), pitch_deg=-2.0, roll_deg=1.0)]
    scans = [np.ascontiguousarray(synth.lidar_scan(world, P, seed=40 + i, n_beams=16, n_az=200)[:, :3]) for i, P in enumerate(poses)]
    T = cases.member_poses(poses, 0, [0, 1, 2])
    store = capi.ScanStore()
    ids = [store.add(s) for s in scans]
    reg = capi.Registrar(store=store)
    yield dict(store=store, reg=reg, scans=scans, ids=ids, T=T)
    reg.close()
    store.close()


def check(capi, store, members, prm_kw=None, ids=None):
    """One submap on the device against the restatement: members = [(points, T)]; `ids`: the resident scans to use instead of
    uploading the points.  Returns the restatement's points."""
    kw = dict(prm_kw or {})
    own = ids is None
    ids = [store.add(p) for p, _ in members] if own else ids
    want, winfo = ref.submap(members, **kw)
    assert winfo["kept"] > 0
    sid, info = store.add_submap(ids, np.stack([T for _, T in members]), capi.default_submap_params(**kw), want_info=True)
    got = store.download(sid)
    assert store.points(sid) == got.shape[0] == want.shape[0]
    assert (bits(got) == bits(want)).all()
    assert {k: info[k] for k in INFO_KEYS} == {k: winfo[k] for k in INFO_KEYS}
    store.release(sid)
    if own:
        for i in ids:
            store.release(i)
    return want


@pytest.mark.parametrize("leaf", [0.2, 0.5])
def test_three_members(capi, env, leaf):
    members = list(zip(env["scans"], env["T"]))
    assert all(2500 < len(s) < 3300 for s in env["scans"])            # several 256-thread blocks per member, 1024-wide scan blocks
    want = check(capi, env["store"], members, dict(leaf=leaf), ids=env["ids"])
    assert want.shape[0] > 1100


def edge_cases():
    rng = np.random.default_rng(3)
    face = np.arange(-12, 13, dtype=np.float32) * np.float32(0.2)      # fp32 multiples of the leaf: on cell faces, or one ulp off
    grid = np.stack(np.meshgrid(face, face[::3], face[::5], indexing="ij"), -1).reshape(-1, 3)
    neg = (rng.uniform(-40.0, -0.01, (3000, 3))).astype(np.float32)
    zeros = np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, -0.0, 0.1], [-0.0, 0.1, -0.1], [-0.1, 0.0, -0.0], [1e-30, -1e-30, 0.0],
                      [-1e-45, 1e-45, -0.0]], np.float32)
    bad = (rng.standard_normal((1200, 3)) * 8).astype(np.float32)
    bad[::7, 0] = np.nan
    bad[3::11, 1] = np.inf
    bad[5::13, 2] = -np.inf
    far = np.concatenate([rng.uniform(-5, 5, (150, 3)).astype(np.float32),
                          np.array([[3e5, 0.0, 0.0], [0.0, -3e5, 0.5], [1.0, 1.0, 3e5], [-3e5, -3e5, -3e5]], np.float32)])
    good = rng.uniform(-6.0, 6.0, (700, 3)).astype(np.float32)
    return {"signed_zeros": [(zeros, EYE)], "cell_faces": [(grid, EYE)], "cell_faces_half": [(grid * np.float32(2.5), EYE)],
            "negative": [(neg, EYE)], "non_finite_rows": [(bad, EYE)], "beyond_key_range": [(far, EYE)],
            "one_point": [(np.array([[-1.25, 3.5, 0.75]], np.float32), EYE)],
            "all_skipped_beside_good": [(np.full((300, 3), np.nan, np.float32), EYE), (good, EYE)]}


@pytest.mark.parametrize("case", sorted(edge_cases()))
def test_one_member_identity_is_the_voxel_grid_filter(capi, env, case):
    members = edge_cases()[case]
    kw = dict(leaf=0.5) if case == "cell_faces_half" else dict(leaf=0.2)
    want = check(capi, env["store"], members, kw)
    if case in ("signed_zeros", "cell_faces", "cell_faces_half", "negative", "one_point"):   # nothing is skipped there
        assert ref.submap(members, **kw)[1]["points_used"] == sum(len(p) for p, _ in members)
    if case == "beyond_key_range":
        assert ref.submap(members, **kw)[1]["points_used"] == 150 and np.abs(want).max() < 6


def test_a_long_run_across_blocks_and_members(capi, env):
    rng = np.random.default_rng(11)
    cell = (np.array([1.2, -0.8, 0.4]) + rng.uniform(0.005, 0.195, (2500, 3))).astype(np.float32)    # all inside one 0.2 m cell
    scatter = rng.uniform(-9.0, 9.0, (1500, 3)).astype(np.float32)
    parts = [np.concatenate([scatter[:500], cell[:900]]), np.concatenate([cell[900:1700], scatter[500:1000]]),
             np.concatenate([scatter[1000:1200], cell[1700:], scatter[1200:]])]
    members = [(p, EYE) for p in parts]
    _, info = ref.submap(members, leaf=0.2)
    k = np.floor(cell * (np.float32(1.0) / np.float32(0.2))).astype(np.int64)
    assert (k == k[0]).all() and info["points_used"] - info["cells"] >= 2499                          # one run of >= 2 500 points
    check(capi, env["store"], members, dict(leaf=0.2))
    check(capi, env["store"], members, dict(leaf=0.2, min_scans=3, min_points=2000))                    # only that run stays


@pytest.mark.parametrize("kw", [dict(min_scans=2), dict(min_scans=3), dict(min_points=3), dict(max_range=20.0),
                                dict(min_scans=2, min_points=3, max_range=20.0)], ids=lambda kw: "-".join(f"{k}{v:g}" for k, v in kw.items()))
def test_filters(capi, env, kw):
    members = list(zip(env["scans"], env["T"]))
    full = ref.submap(members, leaf=0.2)[1]
    want = check(capi, env["store"], members, dict(leaf=0.2, **kw), ids=env["ids"])
    assert 0 < want.shape[0] < full["kept"]


def test_batch_equals_singles(capi, env):
    store, ids, scans, T = env["store"], env["ids"], env["scans"], env["T"]
    rng = np.random.default_rng(21)
    extra = store.add(rng.uniform(-10.0, 10.0, (2100, 3)).astype(np.float32))
    extra2 = store.add(rng.uniform(-8.0, 8.0, (1900, 3)).astype(np.float32))
    pts = {ids[0]: scans[0], ids[1]: scans[1], ids[2]: scans[2], extra: store.download(extra), extra2: store.download(extra2)}
    shift = np.eye(4, dtype=np.float32)
    shift[:3, 3] = (0.31, -0.17, 0.05)
    submaps = [([extra], EYE[None]),                                                    # `extra` is a member of three of them
               ([extra2], shift[None]),                                                 # 2 100 + 1 900 points: one group at 5 000
               ([ids[0], ids[1], ids[2], extra], np.stack([T[0], T[1], T[2], shift])),  # about 11 200 points: over that budget
               ([ids[2], ids[0]], np.stack([T[2], T[0]])),
               ([extra, ids[1], extra2], np.stack([EYE, T[1], shift]))]
    want = [ref.submap([(pts[i], t) for i, t in zip(m, Ts)], leaf=0.2) for m, Ts in submaps]
    singles = [store.download(s) for s in [store.add_submap(m, Ts) for m, Ts in submaps]]
    n0 = len(store)
    for group_points in (0, 5000):              # one group; four groups, the first of two submaps
        new, info = store.add_submaps(submaps, capi.default_submap_params(group_points=group_points), want_info=True)
        assert len(set(new)) == 5 and len(store) == n0 + 5
        for s in range(5):
            got = store.download(new[s])
            assert got.shape == singles[s].shape == want[s][0].shape
            assert (bits(got) == bits(singles[s])).all() and (bits(got) == bits(want[s][0])).all()
            assert {k: info[s][k] for k in INFO_KEYS} == {k: want[s][1][k] for k in INFO_KEYS}
        for s in new:
            store.release(s)
    via_reg = env["reg"].scan_add_submaps(submaps)                                      # the handle's shim: the same store
    assert all((bits(store.download(a)) == bits(b)).all() for a, b in zip(via_reg, singles))


def test_a_members_target_index_does_not_matter(capi, env):
    store = env["store"]
    a = store.add(env["scans"][1])                                   # (a fresh copy: env's scans stay in curve order)
    members, T = [env["ids"][0], a], np.stack([env["T"][0], env["T"][1]])
    before = store.download(store.add_submap(members, T))
    assert not store.debug_index(a)["kd"]
    store.build_target_index(a)
    assert store.debug_index(a)["kd"]
    after = store.download(store.add_submap(members, T))
    assert before.shape == after.shape and (bits(before) == bits(after)).all()
    assert (bits(before) == bits(ref.submap([(env["scans"][0], T[0]), (env["scans"][1], T[1])], leaf=0.2)[0])).all()


def test_the_result_is_an_ordinary_scan(capi, env):
    store, reg, ids = env["store"], env["reg"], env["ids"]
    want, _ = ref.submap(list(zip(env["scans"], env["T"])), leaf=0.2)
    sid = store.add_submap(ids, env["T"])
    assert store.points(sid) == len(want) and (bits(store.download(sid)) == bits(want)).all()
    store.release(sid)
    again = store.add_submap(ids, env["T"])
    assert again == sid                                              # the released id is handed out again
    up = store.add(want)
    q = store.add(cases.trajectory()[2][0][::6])
    prm = capi.default_reg_params(ransac_iters=1000, icp_iters=10)
    for build_index in (False, True):
        if build_index:
            store.build_target_index(again)
            store.build_target_index(up)
        a, b = reg.batch_ids(q, [again], params=prm), reg.batch_ids(q, [up], params=prm)
        assert (bits(a["T"]) == bits(b["T"])).all() and (bits(a["rmse"]) == bits(b["rmse"])).all()
        assert (a["inliers"] == b["inliers"]).all() and (a["ok"] == b["ok"]).all()
    store.build_normals(again, 10)
    nrm = store.normals(again)
    assert nrm.shape == want.shape and np.isfinite(nrm).all() and (np.abs(nrm).sum(axis=1) > 0).mean() > 0.9


def test_errors_leave_the_store_as_it_was(capi, env):
    store, ids, T = env["store"], env["ids"], env["T"]
    L = capi.lib()
    nan = store.add(np.full((400, 3), np.nan, np.float32))
    inf = store.add(np.full((300, 3), np.inf, np.float32))
    big = store.add(np.zeros((1 << 20, 3), np.float32))             # 2048 members of 2^20 points hold 2^31
    released = store.add(env["scans"][0][:100])                     # (last: no later add takes the id over)
    store.release(released)
    state = (len(store), store.bytes())
    bad_T = T.copy()
    bad_T[1, 3, 3] = np.nan                                          # any of the 16 entries
    inf_T = T.copy()
    inf_T[2, 0, 3] = np.inf
    prm = capi.default_submap_params
    calls = [lambda: store.add_submaps([]),                                                       # count = 0
             lambda: store.add_submaps([(ids, T), ([], np.zeros((0, 4, 4), np.float32))]),        # an empty member range
             lambda: store.add_submap([ids[0], 123456], T[:2]),                                   # an unknown id
             lambda: store.add_submap([ids[0], released], T[:2]),                                 # a released id
             lambda: store.add_submap(ids, T, prm(leaf=0.0)),
             lambda: store.add_submap(ids, T, prm(leaf=-0.2)),
             lambda: store.add_submap(ids, T, prm(leaf=float("nan"))),
             lambda: store.add_submap(ids, T, prm(leaf=float("inf"))),
             lambda: store.add_submap(ids, bad_T),
             lambda: store.add_submaps([([ids[0]], EYE[None]), (ids, inf_T)]),
             lambda: store.add_submap([big] * 2048, np.tile(EYE, (2048, 1, 1))),                  # 2^31 points
             lambda: store.add_submap([nan, inf], T[:2]),                                         # every point of every member skipped
             lambda: store.add_submap(ids, T, prm(min_scans=4)),                                  # no cell stays
             # a batch whose SECOND group is the empty one: nothing of the first group stays behind
             lambda: store.add_submaps([(ids, T), ([nan], EYE[None]), ([ids[1]], EYE[None])], prm(group_points=5000))]
    for i, call in enumerate(calls):
        with pytest.raises(capi.GlocError) as e:
            call()
            pytest.fail(f"call {i} did not fail")
        assert e.value.code == 1, i
        assert (len(store), store.bytes()) == state, i
    # null arguments, straight at the C ABI
    p = prm()
    mi, mt, first, new = np.array(ids, np.uint32), np.ascontiguousarray(T), np.array([0, 3], np.uint32), np.zeros(1, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [store._h, vp(mi), vp(mt), vp(first), 1, C.byref(p), vp(new), None]
    for k in (0, 1, 2, 3, 5, 6):
        args = list(good)
        args[k] = None
        assert L.gloc_scan_store_add_submaps(*args) == 1, k
        assert (len(store), store.bytes()) == state, k
    assert L.gloc_scan_store_add_submap(store._h, vp(mi), vp(mt), 0, C.byref(p), new.ctypes.data_as(C.POINTER(C.c_uint32)), None) == 1   # n = 0
    assert (len(store), store.bytes()) == state
    assert L.gloc_scan_store_add_submaps(*good) == 0                 # ... and the same arguments, complete, succeed
    store.release(int(new[0]))
    for s in (nan, inf, big):
        store.release(s)


def test_detector_matches_against_submaps(capi, oracle_mod):
    from gloc3d_amd import loop_detector as ld
    places, P, queries, Q = cases.trajectory()
    sub, _ = ref.submap([(places[j], t) for j, t in enumerate(cases.member_poses(P, cases.ANCHOR, range(5)))], leaf=0.2)
    det = ld.RpyPCLoopDetector(8)
    try:
        det.use_coarse_match = False
        for i, p in enumerate(places):
            det.add_keyframe(np.full(8, float(i), np.float32), p)
        alone = [det.match(q, [cases.ANCHOR])[2]["T"][0] for q in queries]
        n0 = det._reg.scan_count()
        new = det.build_submaps(P, half_window=2)
        assert len(new) == 5 and det._reg.scan_count() == n0 + 5
        for qi, q in enumerate(queries):
            r, T, res = det.match(q, [cases.ANCHOR])
            o = oracle_mod.reg_one(q, sub, ransac_iters=3000, icp_iters=30)
            gt = cases.truth(P, Q, qi)
            e_sub, e_one = cases.position_error(res["T"][0], gt), cases.position_error(alone[qi], gt)
            print(f"query {qi}: position error {e_one:.3f} m against the place's scan, {e_sub:.3f} m against its submap; "
                  f"|dt| to the checker {np.abs(res['T'][0][:3, 3] - o['T'][:3, 3]).max():.2e} m")
            assert np.abs(res["T"][0][:3, 3] - o["T"][:3, 3]).max() < 1e-4
            assert cases.rotation_error_rad(res["T"][0], o["T"]) < 1e-4
            assert bool(res["ok"][0]) == o["ok"]
            assert e_sub < e_one
        ok_rule = lambda T, gt: (lambda er, ep: ep < 1.0 and er < 5.0)(*ld.pose_error(gt, T))
        gt3 = cases.truth(P, Q, 3)
        assert ok_rule(det.match(queries[3], [cases.ANCHOR])[2]["T"][0], gt3) and not ok_rule(alone[3], gt3)
        again = det.build_submaps(P, half_window=1, max_member_dist=1.0)         # replaces: the old submaps are released
        assert det._reg.scan_count() == n0 + 5 and len(again) == 5
        det.add_keyframe(np.full(8, 9.0, np.float32), places[0])                 # a place added afterwards: its own scan
        assert det._target_id(5) == det._db_scan_ids[5] and det._target_id(2) == again[2]
    finally:
        det.close()
