"""GPU: point-to-plane ICP refinement (gloc_scan_store_build_normals / _normals, gloc_reg_p2l_batch_ids, gloc_reg_p2l_system)
against the oracle's normals (bit for bit) and the float64 restatement tests/p2l_ref.py: the normal equations of one pass,
whole alignments behind perturbed ground-truth poses, batching and determinism, frozen jobs, degenerate targets, the
normals' lifecycle in the scan store."""
import numpy as np
import pytest

import p2l_ref as R
from util import bits

pytestmark = pytest.mark.gpu

N_AZ = 300     # ~19 k points per scan: the O(n^2) oracle k-NN takes about a second


@pytest.fixture(scope="module")
def env(capi, oracle_mod):
    from gloc3d_amd import synth
    world = synth.make_world(1001, n_boxes=400, extent=50.0)
    other = synth.make_world(2002, n_boxes=400, extent=50.0)
    truth = [synth.se3(2.0, (0.2, 0.0, 0.0)), synth.se3(-1.5, (0.1, 0.15, 0.02)), synth.se3(1.0, (-0.15, 0.1, 0.0), roll_deg=-0.5)]
    store = capi.ScanStore()
    ids = store.add_raycast(world, [np.eye(4)] + truth, np.array([5, 6, 7, 8], np.uint64), n_az=N_AZ)
    far = store.add_raycast(other, [np.eye(4)], np.array([9], np.uint64), n_az=N_AZ)[0]
    reg = capi.Registrar(store=store)
    tgt, srcs = ids[0], ids[1:]
    for t in (tgt, far):
        store.build_normals(t, 10)
    pts = {i: store.download(i) for i in ids + [far]}
    nrm = {t: store.normals(t) for t in (tgt, far)}
    nn = lambda s, t: oracle_mod.nn3(s, t, grid=True)
    yield dict(store=store, reg=reg, tgt=tgt, far=far, srcs=srcs, truth=truth, pts=pts, nrm=nrm, nn=nn, world=world)
    reg.close()
    store.close()


def _ref(env, capi, src, tgt, init, prm):
    return R.align(env["pts"][src], env["pts"][tgt], env["nrm"][tgt], env["nn"], init_T=init, max_iters=prm.max_iters,
                   max_corr_dist=prm.max_corr_dist, trans_eps=prm.trans_eps, rot_eps=prm.rot_eps)


def _offsets():
    from gloc3d_amd import synth
    return [synth.se3(1.0, (0.10, -0.05, 0.02)), synth.se3(-2.0, (-0.15, 0.10, -0.03), roll_deg=0.4),
            synth.se3(0.5, (0.25, 0.20, 0.05))]


def test_normals_equal_the_oracle_bit_for_bit(capi, env, oracle_mod):
    st = env["store"]
    for k in (10, 5):
        xyz = env["pts"][env["srcs"][0]]
        sid = st.add(xyz)
        st.build_normals(sid, k)
        dev = st.normals(sid)
        ref, _ = oracle_mod.ground_normals(xyz, oracle_mod.ground_knn(xyz, k)[0])
        assert dev.shape == ref.shape and (bits(dev) == bits(ref)).all()
        lens = np.linalg.norm(dev.astype(np.float64), axis=1)
        assert (np.abs(lens - 1) < 1e-6).mean() > 0.99
        st.release(sid)
    # NaN rows and duplicated points
    odd = env["pts"][env["srcs"][1]][:6000].copy()
    odd[100:140] = odd[0:40]
    odd[::97, 1] = np.nan
    odd[5::301, 0] = np.inf
    sid = st.add(odd)
    st.build_normals(sid, 10)
    dev = st.normals(sid)
    ref, _ = oracle_mod.ground_normals(odd, oracle_mod.ground_knn(odd, 10)[0])
    print(f"scan with NaN / inf rows and duplicates: {int((bits(dev) != bits(ref)).any(1).sum())} of {len(odd)} rows differ")
    assert (bits(dev) == bits(ref)).all()
    assert not dev[::97].any() and not dev[5::301].any()         # a non-finite point has no normal
    st.release(sid)
    # k outside [3, 16], no normals yet
    sid = st.add(odd[:500])
    for k in (2, 17):
        with pytest.raises(capi.GlocError) as e:
            st.build_normals(sid, k)
        assert e.value.code == 1
    with pytest.raises(capi.GlocError) as e:
        st.normals(sid)
    assert e.value.code == 5
    with pytest.raises(capi.GlocError) as e:
        env["reg"].p2l_batch(env["srcs"][0], [sid], params=capi.default_p2l_params(normal_k=2))
    assert e.value.code == 1
    st.release(sid)


@pytest.mark.parametrize("gate", [0.0, 0.3])
def test_system_matches_the_restatement(capi, env, oracle_mod, gate):
    reg = env["reg"]
    prm = capi.default_p2l_params(max_corr_dist=gate)
    for s, truth, off in zip(env["srcs"], env["truth"], _offsets()):
        T = (off @ truth).astype(np.float32)
        H, g, s2, cnt = reg.p2l_system(s, env["tgt"], T, prm)
        Hr, gr, s2r, cntr = R.system(env["pts"][s], env["pts"][env["tgt"]], env["nrm"][env["tgt"]], T, oracle_mod.nn3,
                                     max_corr_dist=prm.max_corr_dist)
        scale = max(np.abs(Hr).max(), np.abs(gr).max(), s2r)
        err = max(np.abs(H - Hr).max(), np.abs(g - gr).max(), abs(s2 - s2r)) / scale
        print(f"gate {gate}: pairs {cnt} / {cntr} of {len(env['pts'][s])}, error {err:.3e} of the largest entry")
        assert cnt == cntr and 1000 < cnt <= len(env["pts"][s])
        assert (H == H.T).all()
        assert err <= 1e-9
    if gate > 0:
        _, _, _, c0 = reg.p2l_system(env["srcs"][0], env["tgt"], (_offsets()[0] @ env["truth"][0]).astype(np.float32))
        _, _, _, c1 = reg.p2l_system(env["srcs"][0], env["tgt"], (_offsets()[0] @ env["truth"][0]).astype(np.float32), prm)
        assert c1 < c0


@pytest.mark.parametrize("eps", [False, True])
def test_alignments_follow_the_restatement(capi, env, eps):
    reg = env["reg"]
    prm = capi.default_p2l_params(max_iters=10, max_corr_dist=1.0)
    if eps:
        prm = capi.default_p2l_params(max_iters=30, max_corr_dist=1.0, trans_eps=1e-4, rot_eps=1e-5)
    jobs = [(s, env["tgt"], (off @ t).astype(np.float32)) for s, t, off in zip(env["srcs"], env["truth"], _offsets())]
    jobs.append((env["srcs"][0], env["far"], env["truth"][0].astype(np.float32)))          # a different world
    for s, tgt, init in jobs:
        T, rmse, iters, status = reg.p2l_batch(s, [tgt], init_T=init[None], params=prm)
        r = _ref(env, capi, s, tgt, init, prm)
        dt, da = R.pose_err(r["T"], T[0])
        print(f"eps {eps} target {tgt}: iters {iters[0]} / {r['iters']}, status {status[0]} / {r['status']}, "
              f"rmse {rmse[0]:.5f} / {r['rmse']:.5f}, against the restatement {dt:.2e} m {da:.2e} rad")
        assert dt < 1e-4 and da < 1e-4
        assert status[0] == r["status"]
        assert abs(int(iters[0]) - r["iters"]) <= 1 if eps else int(iters[0]) == r["iters"] == prm.max_iters
        assert abs(rmse[0] - r["rmse"]) <= 1e-4
        if tgt == env["tgt"]:
            truth = env["truth"][env["srcs"].index(s)]
            dt, da = R.pose_err(truth, T[0])
            assert dt < 0.02 and da < 2e-3, (dt, da)
            if eps:
                assert status[0] == 1 and iters[0] < 30


def test_a_batch_equals_single_calls_bit_for_bit(capi, env):
    reg = env["reg"]
    s = env["srcs"][0]
    offs = _offsets()
    tg = [env["tgt"], env["far"], env["srcs"][1], env["tgt"]] * 3          # mixed targets; srcs[1] gets its normals here
    init = np.stack([(offs[i % 3] @ env["truth"][0]) for i in range(12)]).astype(np.float32)
    for prm in (capi.default_p2l_params(max_iters=6), capi.default_p2l_params(max_iters=12, trans_eps=1e-3, rot_eps=1e-4)):
        T, rmse, iters, status = reg.p2l_batch(s, tg, init_T=init, params=prm)
        T2, rmse2, iters2, status2 = reg.p2l_batch(s, tg, init_T=init, params=prm)
        assert (bits(T) == bits(T2)).all() and (bits(rmse) == bits(rmse2)).all() and (iters == iters2).all() and (status == status2).all()
        for c in range(12):
            t1, r1, i1, s1 = reg.p2l_batch(s, [tg[c]], init_T=init[c:c + 1], params=prm)
            assert (bits(t1[0]) == bits(T[c])).all(), c
            assert bits(r1)[0] == bits(rmse)[c] and i1[0] == iters[c] and s1[0] == status[c]


def test_a_stopped_job_is_frozen(capi, env):
    reg = env["reg"]
    s, truth = env["srcs"][0], env["truth"][0]
    near = truth.astype(np.float32)
    far = (_offsets()[2] @ truth).astype(np.float32)
    prm = capi.default_p2l_params(max_iters=20, trans_eps=2e-3, rot_eps=2e-4)
    T, _, iters, status = reg.p2l_batch(s, [env["tgt"], env["tgt"]], init_T=np.stack([near, far]), params=prm)
    assert status[0] == 1 and status[1] == 1 and iters[0] < iters[1] <= 20
    # exactly that many updates with the stop test off: the pose the job had when it stopped, bit for bit -- the passes the
    # batch ran for the other job did not touch it
    T0, _, i0, s0 = reg.p2l_batch(s, [env["tgt"]], init_T=near[None], params=capi.default_p2l_params(max_iters=int(iters[0])))
    assert i0[0] == iters[0] and s0[0] == 0
    assert (bits(T0[0]) == bits(T[0])).all()


def test_a_flat_plane_is_degenerate(capi, env):
    st, reg = env["store"], env["reg"]
    g = np.arange(-10, 10, 0.2, dtype=np.float32)
    plane = np.stack([np.repeat(g, len(g)), np.tile(g, len(g)), np.full(len(g) ** 2, -1.7, np.float32)], axis=1)
    pid = st.add(plane)
    guess = (_offsets()[0] @ env["truth"][0]).astype(np.float32)
    tg = [pid, env["tgt"]]
    T, rmse, iters, status = reg.p2l_batch(env["srcs"][0], tg, init_T=np.stack([guess, guess]),
                                           params=capi.default_p2l_params(max_iters=5))
    n = st.normals(pid)                                         # built by the call, k = 10
    assert (n[:, :2] == 0).all() and (np.abs(n[:, 2]) == 1).all()
    assert status[0] == 2 and iters[0] == 0 and (bits(T[0]) == bits(guess)).all()
    assert status[1] == 0 and iters[1] == 5                     # the job beside it ran
    st.release(pid)


def test_normals_lifecycle(capi, env):
    st, reg = env["store"], env["reg"]
    xyz = env["pts"][env["srcs"][2]]
    live0, _ = st.bytes()
    sid = st.add(xyz)
    live1, _ = st.bytes()
    st.build_normals(sid, 10)
    live2, _ = st.bytes()
    assert live2 - live1 == 12 * len(xyz)
    st.build_normals(sid, 10)                                   # the same k again: nothing new
    assert st.bytes()[0] == live2
    before = st.normals(sid)
    st.build_target_index(sid)                                  # re-sorts the points: the normals follow them
    after = st.normals(sid)
    assert (bits(before) == bits(after)).all() and after.any()
    T = (_offsets()[1] @ env["truth"][0]).astype(np.float32)
    sys_kd = reg.p2l_system(env["srcs"][0], sid, T)
    plain = st.add(xyz)
    sys_plain = reg.p2l_system(env["srcs"][0], plain, T)        # (normals built by the call)
    assert sys_kd[3] == sys_plain[3] and np.abs(sys_kd[0] - sys_plain[0]).max() <= 1e-9 * np.abs(sys_plain[0]).max()
    st.release(plain)
    # a batch between begin and end: the handle refuses, the store still builds normals for a scan the batch has pinned
    reg.batch_multi_begin([env["srcs"][0]], [[sid, env["srcs"][1]]], params=capi.default_reg_params(ransac_iters=0, icp_iters=2))
    with pytest.raises(capi.GlocError) as e:
        reg.p2l_batch(env["srcs"][0], [sid])
    assert e.value.code == 5
    with pytest.raises(capi.GlocError) as e:
        reg.p2l_system(env["srcs"][0], sid)
    assert e.value.code == 5
    st.build_normals(env["srcs"][0], 10)                        # pinned by the batch: adds data, moves nothing
    reg.batch_multi_end()
    assert (bits(st.normals(sid)) == bits(after)).all()
    st.release(sid)
    assert st.bytes()[0] == live0 + 12 * len(env["pts"][env["srcs"][0]])
