"""GPU: generalized ICP refinement (gloc_reg_gicp_batch_ids, gloc_reg_gicp_system) against the float64 restatement
tests/gicp_ref.py: the normal equations of one pass, whole alignments behind perturbed ground-truth poses, batching and
determinism, frozen jobs, degenerate inputs, a source in kd order, normals built on demand.

Tolerances are not constants: each test measures the restatement's own noise floor on its inputs -- the same formulas
evaluated two ways, the pairs summed forward and reversed (one after the other: no reduction tree is further from the
other order) and M by numpy.linalg.inv and by the adjugate -- and allows the device 10 x that for its different
reduction tree, which must stay below SYSTEM_CAP.  Measured on an MI355X: see the figures beside the constants."""
import numpy as np
import pytest

import gicp_ref as R
from util import bits

pytestmark = pytest.mark.gpu

N_AZ = 300     # ~19 k points per scan: the O(n^2) oracle k-NN takes about a second

# 10 x the floor may not exceed this, relative to the largest entry: far above any fp64 ordering effect (19 k pairs summed
# one after the other: ~1e-13), far below any error in a formula (a wrong term is 1e-3 or more).
# Measured on an MI355X: floor by order 3.1e-15 .. 7.4e-15, by inverse 1.2e-16 .. 4.4e-16, so tolerances of 3.1e-14 .. 7.4e-14;
# the device's error 2.1e-15 .. 7.5e-15.
SYSTEM_CAP = 1e-9
# Poses: 10 x the floor -- the restatement's final pose computed the two ways -- may not exceed the point-to-plane
# refinement's class ...
POSE_CAP = 1e-8
# ... and the pose comes back in fp32: to the floor is added twice the distance from the restatement's fp64 pose to its
# own fp32 rounding (half an ulp an entry; a device pose that differs by the floor may round the other way in an entry,
# one ulp at most).  Measured: floor 5e-16 .. 4e-15 m, 8e-17 .. 4e-16 rad; the fp32 output 8e-10 .. 2.8e-8 m, 4.5e-9 .. 2.6e-8
# rad, which is also what the device's poses are off the restatement's by.


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
    for t in ids + [far]:
        store.build_normals(t, 10)
    pts = {i: store.download(i) for i in ids + [far]}
    nrm = {i: store.normals(i) for i in ids + [far]}
    nn = lambda s, t: oracle_mod.nn3(s, t, grid=True)
    yield dict(store=store, reg=reg, tgt=tgt, far=far, srcs=srcs, truth=truth, pts=pts, nrm=nrm, nn=nn, world=world)
    reg.close()
    store.close()


def _ref(env, src, tgt, init, prm, **kw):
    return R.align(env["pts"][src], env["nrm"][src], env["pts"][tgt], env["nrm"][tgt], env["nn"], init_T=init, max_iters=prm.max_iters,
                   max_corr_dist=prm.max_corr_dist, trans_eps=prm.trans_eps, rot_eps=prm.rot_eps, plane_eps=prm.plane_eps, **kw)


def _offsets():
    from gloc3d_amd import synth
    return [synth.se3(1.0, (0.10, -0.05, 0.02)), synth.se3(-2.0, (-0.15, 0.10, -0.03), roll_deg=0.4),
            synth.se3(0.5, (0.25, 0.20, 0.05))]


def _rel(a, b, scale):
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max(), abs(a[2] - b[2])) / scale


def _system_floor(env, s, tgt, T, prm):
    """The restatement's H, g, sum, count, their scale, and its noise floor on these inputs."""
    p, q, ns, nt = R.pairs(env["pts"][s], env["nrm"][s], env["pts"][tgt], env["nrm"][tgt], T, env["nn"], prm.max_corr_dist)
    Rm = R.rotation(T)
    ref = R.system_of_pairs(p, q, ns, nt, Rm, prm.plane_eps)
    rev = R.system_of_pairs(p, q, ns, nt, Rm, prm.plane_eps, order="reversed")
    adj = R.system_of_pairs(p, q, ns, nt, Rm, prm.plane_eps, how="adj")
    scale = max(np.abs(ref[0]).max(), np.abs(ref[1]).max(), ref[2])
    return ref, scale, _rel(ref, rev, scale), _rel(ref, adj, scale)


@pytest.mark.parametrize("gate", [0.0, 0.3])
def test_system_matches_the_restatement(capi, env, gate):
    reg = env["reg"]
    prm = capi.default_gicp_params(max_corr_dist=gate)
    for s, truth, off in zip(env["srcs"], env["truth"], _offsets()):
        T = (off @ truth).astype(np.float32)
        H, g, s2, cnt = reg.gicp_system(s, env["tgt"], T, prm)
        ref, scale, f_order, f_inv = _system_floor(env, s, env["tgt"], T, prm)
        tol = 10 * max(f_order, f_inv)
        err = _rel((H, g, s2), ref, scale)
        print(f"gate {gate}: pairs {cnt} / {ref[3]} of {len(env['pts'][s])}, floor: order {f_order:.3e}, inverse {f_inv:.3e} -> tolerance "
              f"{tol:.3e}; device error {err:.3e} of the largest entry")
        assert tol <= SYSTEM_CAP
        assert cnt == ref[3] and 1000 < cnt <= len(env["pts"][s])
        assert (H == H.T).all()
        assert err <= tol
    if gate > 0:
        T = (_offsets()[0] @ env["truth"][0]).astype(np.float32)
        assert reg.gicp_system(env["srcs"][0], env["tgt"], T, prm)[3] < reg.gicp_system(env["srcs"][0], env["tgt"], T)[3]


@pytest.mark.parametrize("eps", [False, True])
def test_alignments_follow_the_restatement(capi, env, eps):
    reg = env["reg"]
    prm = capi.default_gicp_params(max_iters=10, max_corr_dist=1.0)
    if eps:
        prm = capi.default_gicp_params(max_iters=30, max_corr_dist=1.0, trans_eps=1e-4, rot_eps=1e-5)
    jobs = [(s, env["tgt"], (off @ t).astype(np.float32)) for s, t, off in zip(env["srcs"], env["truth"], _offsets())]
    jobs.append((env["srcs"][0], env["far"], env["truth"][0].astype(np.float32)))          # a different world
    for s, tgt, init in jobs:
        T, rmse, iters, status = reg.gicp_batch(s, [tgt], init_T=init[None], params=prm)
        r = _ref(env, s, tgt, init, prm)
        r2 = _ref(env, s, tgt, init, prm, how="adj", order="reversed")
        ft, fa = R.pose_err(r["T"], r2["T"])
        ot, oa = R.pose_err(r["T"], r["T"].astype(np.float32))
        dt, da = R.pose_err(r["T"], T[0])
        print(f"eps {eps} target {tgt}: iters {iters[0]} / {r['iters']} / {r2['iters']}, status {status[0]} / {r['status']}, "
              f"rmse {rmse[0]:.5f} / {r['rmse']:.5f}; floor {ft:.2e} m {fa:.2e} rad, fp32 output {ot:.2e} m {oa:.2e} rad; "
              f"against the restatement {dt:.2e} m {da:.2e} rad")
        assert r2["iters"] == r["iters"] and r2["status"] == r["status"]
        assert 10 * ft <= POSE_CAP and 10 * fa <= POSE_CAP
        assert dt <= 10 * ft + 2 * ot and da <= 10 * fa + 2 * oa
        assert status[0] == r["status"]
        assert int(iters[0]) == r["iters"] and (eps or r["iters"] == prm.max_iters)
        assert abs(rmse[0] - r["rmse"]) <= 1e-6 * max(r["rmse"], 1.0)                       # (fp32 output)
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
    tg = [env["tgt"], env["far"], env["srcs"][1], env["tgt"]] * 3
    init = np.stack([(offs[i % 3] @ env["truth"][0]) for i in range(12)]).astype(np.float32)
    for prm in (capi.default_gicp_params(max_iters=6), capi.default_gicp_params(max_iters=12, trans_eps=1e-3, rot_eps=1e-4)):
        T, rmse, iters, status = reg.gicp_batch(s, tg, init_T=init, params=prm)
        T2, rmse2, iters2, status2 = reg.gicp_batch(s, tg, init_T=init, params=prm)
        assert (bits(T) == bits(T2)).all() and (bits(rmse) == bits(rmse2)).all() and (iters == iters2).all() and (status == status2).all()
        for c in range(12):
            t1, r1, i1, s1 = reg.gicp_batch(s, [tg[c]], init_T=init[c:c + 1], params=prm)
            assert (bits(t1[0]) == bits(T[c])).all(), c
            assert bits(r1)[0] == bits(rmse)[c] and i1[0] == iters[c] and s1[0] == status[c]


def test_a_stopped_job_is_frozen(capi, env):
    reg = env["reg"]
    s, truth = env["srcs"][0], env["truth"][0]
    near = truth.astype(np.float32)
    far = (_offsets()[2] @ truth).astype(np.float32)
    prm = capi.default_gicp_params(max_iters=20, trans_eps=2e-3, rot_eps=2e-4)
    T, _, iters, status = reg.gicp_batch(s, [env["tgt"], env["tgt"]], init_T=np.stack([near, far]), params=prm)
    assert status[0] == 1 and status[1] == 1 and iters[0] < iters[1] <= 20
    # exactly that many updates with the stop test off: the pose the job had when it stopped, bit for bit -- the passes the
    # batch ran for the other job did not touch it
    T0, _, i0, s0 = reg.gicp_batch(s, [env["tgt"]], init_T=near[None], params=capi.default_gicp_params(max_iters=int(iters[0])))
    assert i0[0] == iters[0] and s0[0] == 0
    assert (bits(T0[0]) == bits(T[0])).all()


def test_the_degenerate_case_returns_status_2_and_the_guess(capi, env):
    """Degenerate as the contract has it (tests/test_gicp_ref_cpu.py): fewer than 6 pairs, no pair within the gate, points on
    one line.  A flat plane is NOT degenerate for generalized ICP -- a pair keeps weight 1 / 2 along the plane -- and there
    the device follows the restatement like anywhere else."""
    st, reg = env["store"], env["reg"]
    guess = (_offsets()[0] @ env["truth"][0]).astype(np.float32)
    src = env["srcs"][0]
    few = st.add(env["pts"][src][:5])
    line = st.add(np.outer(np.linspace(-5, 5, 200), [1.0, 0.0, 0.0]).astype(np.float32))
    I = np.eye(4, dtype=np.float32)
    prm = capi.default_gicp_params(max_iters=5)
    T, rmse, iters, status = reg.gicp_batch(few, [env["tgt"]], init_T=guess[None], params=prm)
    assert status[0] == 2 and iters[0] == 0 and (bits(T[0]) == bits(guess)).all()
    T, rmse, iters, status = reg.gicp_batch(line, [line], init_T=I[None], params=prm)
    assert status[0] == 2 and iters[0] == 0 and (bits(T[0]) == bits(I)).all()
    away = guess.copy()
    away[:3, 3] += 500.0
    T, rmse, iters, status = reg.gicp_batch(src, [env["tgt"], env["tgt"]], init_T=np.stack([away, guess]),
                                            params=capi.default_gicp_params(max_iters=5, max_corr_dist=1.0))
    assert status[0] == 2 and iters[0] == 0 and rmse[0] == 0 and (bits(T[0]) == bits(away)).all()
    assert status[1] == 0 and iters[1] == 5                     # the job beside it ran
    # the flat plane that stops point-to-plane at once
    g = np.arange(-10, 10, 0.2, dtype=np.float32)
    plane = np.stack([np.repeat(g, len(g)), np.tile(g, len(g)), np.full(len(g) ** 2, -1.7, np.float32)], axis=1)
    pid = st.add(plane)
    assert reg.p2l_batch(src, [pid], init_T=guess[None], params=capi.default_p2l_params(max_iters=5))[3][0] == 2
    T, rmse, iters, status = reg.gicp_batch(src, [pid], init_T=guess[None], params=prm)
    r = R.align(env["pts"][src], env["nrm"][src], plane, st.normals(pid), env["nn"], init_T=guess, max_iters=5)
    assert status[0] == r["status"] == 0 and iters[0] == r["iters"] == 5
    dt, da = R.pose_err(r["T"], T[0])
    assert dt < 1e-6 and da < 1e-6, (dt, da)
    for i in (few, line, pid):
        st.release(i)


def test_a_source_in_kd_order_gives_the_same_result(capi, env):
    """DevScan::nrm follows idx.pts through the kd re-sort, so the source's normal is read at the slot of its point whatever
    the order: the pairs are the same set, summed in another order."""
    st, reg = env["store"], env["reg"]
    src = env["srcs"][1]
    xyz = env["pts"][src]
    kd = st.add(xyz)
    st.build_normals(kd, 10)
    st.build_target_index(kd)                                   # the source now carries a target index: kd order
    assert (bits(st.normals(kd)) == bits(env["nrm"][src])).all()
    T = (_offsets()[1] @ env["truth"][1]).astype(np.float32)
    prm = capi.default_gicp_params()
    a = reg.gicp_system(kd, env["tgt"], T, prm)
    b = reg.gicp_system(src, env["tgt"], T, prm)
    ref, scale, f_order, f_inv = _system_floor(env, src, env["tgt"], T, prm)
    tol = 10 * max(f_order, f_inv)
    print(f"kd-ordered source against curve-ordered: {_rel(a, b, scale):.3e}; against the restatement {_rel(a, ref, scale):.3e}; tolerance {tol:.3e}")
    assert a[3] == b[3] == ref[3]
    assert _rel(a, ref, scale) <= tol and _rel(b, ref, scale) <= tol
    # normals first or re-sort first: the same scan
    kd2 = st.add(xyz)
    st.build_target_index(kd2)
    c = reg.gicp_system(kd2, env["tgt"], T, prm)                # (normals built by the call, in kd order)
    assert c[3] == a[3] and (bits(c[0]) == bits(a[0])).all() and (bits(c[1]) == bits(a[1])).all()
    p10 = capi.default_gicp_params(max_iters=10, max_corr_dist=1.0)
    Ta, _, ia, sa = reg.gicp_batch(kd, [env["tgt"]], init_T=T[None], params=p10)
    Tb, _, ib, sb = reg.gicp_batch(src, [env["tgt"]], init_T=T[None], params=p10)
    dt, da = R.pose_err(Ta[0], Tb[0])
    assert ia[0] == ib[0] and sa[0] == sb[0] and dt <= 2e-7 and da <= 2e-7, (dt, da)     # (fp32 outputs: an ulp or two)
    st.release(kd)
    st.release(kd2)


def test_normals_absent_on_the_source_are_built_on_demand(capi, env):
    st, reg = env["store"], env["reg"]
    src = env["srcs"][2]
    xyz = env["pts"][src]
    T = (_offsets()[2] @ env["truth"][2]).astype(np.float32)
    bare = st.add(xyz)
    tbare = st.add(env["pts"][env["tgt"]])
    with pytest.raises(capi.GlocError) as e:
        st.normals(bare)
    assert e.value.code == 5
    live0, _ = st.bytes()
    a = reg.gicp_system(bare, tbare, T)                         # builds both scans' normals with normal_k = 10
    live1, _ = st.bytes()
    assert live1 - live0 == 12 * (len(xyz) + len(env["pts"][env["tgt"]]))
    assert (bits(st.normals(bare)) == bits(env["nrm"][src])).all()
    b = reg.gicp_system(src, env["tgt"], T)
    assert a[3] == b[3] and (bits(a[0]) == bits(b[0])).all() and (bits(a[1]) == bits(b[1])).all() and a[2] == b[2]
    reg.gicp_system(bare, tbare, T)                             # again: nothing new
    assert st.bytes()[0] == live1
    # existing normals are used as they are, whatever normal_k says
    c = reg.gicp_system(bare, tbare, T, capi.default_gicp_params(normal_k=5))
    assert (bits(c[0]) == bits(a[0])).all() and st.bytes()[0] == live1
    # refusals: a bad k or plane_eps, an unknown id, a batch in flight
    for bad in (capi.default_gicp_params(normal_k=2), capi.default_gicp_params(plane_eps=0.0), capi.default_gicp_params(max_iters=0)):
        with pytest.raises(capi.GlocError) as e:
            reg.gicp_batch(bare, [tbare], params=bad)
        assert e.value.code == 1
    with pytest.raises(capi.GlocError) as e:
        reg.gicp_batch(10 ** 6, [tbare])
    assert e.value.code == 1
    reg.batch_multi_begin([src], [[env["tgt"]]], params=capi.default_reg_params(ransac_iters=0, icp_iters=2))
    with pytest.raises(capi.GlocError) as e:
        reg.gicp_batch(src, [env["tgt"]])
    assert e.value.code == 5
    with pytest.raises(capi.GlocError) as e:
        reg.gicp_system(src, env["tgt"])
    assert e.value.code == 5
    reg.batch_multi_end()
    st.release(bare)
    st.release(tbare)


def test_plane_eps_one_is_half_the_point_to_point_system(capi, env):
    reg = env["reg"]
    s, tgt = env["srcs"][0], env["tgt"]
    T = (_offsets()[0] @ env["truth"][0]).astype(np.float32)
    prm = capi.default_gicp_params(plane_eps=1.0)
    H, g, s2, cnt = reg.gicp_system(s, tgt, T, prm)
    p, q, _, _ = R.pairs(env["pts"][s], None, env["pts"][tgt], None, T, env["nn"])
    J, e = R.jacobian(p), p - q
    Hp, gp, sp = np.einsum("mia,mib->ab", J, J), np.einsum("mia,mi->a", J, e), float(np.einsum("mi,mi->", e, e))
    ref, scale, f_order, f_inv = _system_floor(env, s, tgt, T, prm)
    tol = 10 * max(f_order, f_inv, _rel((0.5 * Hp, 0.5 * gp, 0.5 * sp), ref, scale))
    err = _rel((H, g, s2), (0.5 * Hp, 0.5 * gp, 0.5 * sp), scale)
    print(f"plane_eps 1: device against half the point-to-point system {err:.3e}, tolerance {tol:.3e}")
    assert cnt == len(p) and tol <= SYSTEM_CAP and err <= tol
    # ... and so is its rmse: sqrt(1 / 2) of the point-to-point residual at the final pose
    _, rmse, iters, status = reg.gicp_batch(s, [tgt], init_T=T[None], params=capi.default_gicp_params(plane_eps=1.0, max_iters=1))
    assert iters[0] == 1 and status[0] == 0 and rmse[0] > 0
