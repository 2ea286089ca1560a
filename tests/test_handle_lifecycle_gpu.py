"""GPU: a handle that is gone holds nothing.  Every wrapper class of gloc3d_amd.capi over a device handle is built, used
once for real (so that its workspaces exist) and closed, again and again: the device's free memory after the last cycle
equals the free memory after cycle 2.  Also: what a kNN view and an attached scan store promise about lifetimes.

(Comm is left out: it owns an RCCL communicator, not device buffers, and needs several ranks to exist.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GLOC_ERR_STATE = 5
# Cycles per class.  Sized from the leak this file was written against (LAB_NOTES, "Handle lifecycle"): a registration
# handle that did not free its chained-launch buffer cost 2 MiB of free memory (one allocation granule) in 8 of 12
# cycles on an MI355X, 7 granules (14 680 064 B) between the two readings compared below.
CYCLES = 12
READS = 5


def free_bytes():
    """Free device memory with nothing of ours in flight: the largest of a few readings (another process on the card may
    hold memory for a moment; identical cycles are compared by their quiet state, not with a tolerance in bytes)."""
    import torch
    best = 0
    for _ in range(READS):
        torch.cuda.synchronize()
        best = max(best, torch.cuda.mem_get_info()[0])
    return best


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def clouds():
    from gloc3d_amd import synth
    w = synth.make_world(1001)
    A = synth.lidar_scan(w, None, seed=1001, n_az=300)
    B = synth.lidar_scan(w, synth.se3(3.0, (0.4, -0.2, 0.05)), seed=1002, n_az=300)
    return np.ascontiguousarray(A, np.float32), np.ascontiguousarray(B, np.float32)


@pytest.fixture(scope="module")
def vgg_layers(capi):
    rng = np.random.default_rng(5)
    out = []
    for l in range(capi.VGG_LAYERS):
        cin, cout, _, _ = capi.vgg_layer_shape(l)
        out.append(((rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32),
                    (rng.standard_normal(cout) * 0.01).astype(np.float32)))
    return out


def use_knn(capi, clouds):
    rng = np.random.default_rng(1)
    ix = capi.KnnIndex(64)
    ix.add(rng.standard_normal((3000, 64)).astype(np.float32))
    v = ix.view()
    q = rng.standard_normal((16, 64)).astype(np.float32)
    for algo in (capi.ALGO_EXACT, capi.ALGO_MFMA):
        ix.set_option(capi.KNN_OPT_ALGO, algo)
        ix.search(q, 10)
    v.search(q, 10)
    v.close()
    return [ix]


def use_scan_store(capi, clouds):
    st = capi.ScanStore()
    ids = [st.add(c[:, :3]) for c in clouds]
    st.build_target_index(ids[0])
    return [st]


def use_registrar(capi, clouds):
    """A 20-job batch with ICP: small enough for the warm passes to run as one chained launch, whose buffer is the one
    gloc_reg_destroy once forgot."""
    A, B = (c[:, :3] for c in clouds)
    r = capi.Registrar()
    q = r.scan_upload(np.ascontiguousarray(B[::2]))
    cands = [r.scan_upload(np.ascontiguousarray(A[i % 3::2 + i % 4])) for i in range(20)]
    out = r.batch_multi([q], np.array([cands], np.uint32), params=capi.default_reg_params(ransac_iters=200, icp_iters=6))
    launches, timeouts = r.debug_chain()
    assert launches >= 1 and timeouts == 0, (launches, timeouts)   # (else this case exercises no chained launch)
    assert out["ok"].any()
    return [r]


def use_registrar_on_store(capi, clouds):
    st = capi.ScanStore()
    a, b = (st.add(c[:, :3]) for c in clouds)
    r = capi.Registrar(store=st)
    r.batch_ids(b, [a], params=capi.default_reg_params(ransac_iters=100, icp_iters=3))
    r.ndt_batch(b, [a])
    return [r, st]


def use_registrar_refinements(capi, clouds):
    """Point-to-plane, then generalized ICP on one handle: the workspace they share (p2l::Ws: states, partials, the
    pinned stop counter and its event) and the normals the calls build beside the scans."""
    st = capi.ScanStore()
    a, b = (st.add(c[:, :3]) for c in clouds)
    r = capi.Registrar(store=st)
    I = np.eye(4, dtype=np.float32)[None]
    _, _, iters, status = r.p2l_batch(b, [a, a], init_T=np.concatenate([I, I]), params=capi.default_p2l_params(max_iters=5, trans_eps=1e-3, rot_eps=1e-4))
    assert (status != 2).all() and (iters >= 1).all()
    _, _, iters, status = r.gicp_batch(b, [a], init_T=I, params=capi.default_gicp_params(max_iters=3))
    assert status[0] == 0 and iters[0] == 3
    r.p2l_system(b, a)
    return [r, st]


def use_vlad(capi, clouds):
    rng = np.random.default_rng(2)
    K, Cc, D = 16, 64, 128
    nv = capi.NetVladFC(rng.standard_normal((K, Cc)).astype(np.float32), rng.standard_normal((K, Cc)).astype(np.float32),
                        (rng.standard_normal((K * Cc, D)) * 0.05).astype(np.float32))
    nv.set_gating(rng.standard_normal((D, D)).astype(np.float32) * 0.1, np.ones(D, np.float32), np.zeros(D, np.float32))
    nv.forward(rng.standard_normal((3, Cc, 40)).astype(np.float32))
    return [nv]


def use_bev(capi, clouds):
    bp = capi.BevProjector()
    _, info = bp.project(clouds[0])
    bp.raw_image(info)
    return [bp]


def use_pillar(capi, clouds):
    rng = np.random.default_rng(3)
    e = capi.PillarEncoder()
    e.set_pointnet(rng.standard_normal((64, 14)).astype(np.float32) * 0.2, np.ones(64, np.float32), np.zeros(64, np.float32),
                   np.zeros(64, np.float32), np.ones(64, np.float32))
    p = capi.default_pillar_params(num_points=4096)
    e.inputs(clouds[0], p)
    e.canvas([clouds[0], clouds[1]], p)
    return [e]


def use_coarse(capi, clouds):
    cm = capi.CoarseMatcher()
    g = [cm.add_scan(c) for c in clouds]
    cm.match(g[1], [g[0]])
    cm.release(g[0])     # (a released grid's block is parked in the handle's cache: it goes with the handle)
    return [cm]


def use_ground(capi, clouds):
    ge = capi.GroundEstimator()
    ge.estimate(clouds[0], want_cloud=True)
    return [ge]


USES = {"KnnIndex": use_knn, "ScanStore": use_scan_store, "Registrar": use_registrar,
        "Registrar+ScanStore": use_registrar_on_store, "Registrar p2l+gicp": use_registrar_refinements, "NetVladFC": use_vlad, "BevProjector": use_bev,
        "PillarEncoder": use_pillar, "CoarseMatcher": use_coarse, "GroundEstimator": use_ground}


def cycles(name, use):
    """Free memory after each of CYCLES rounds of (build, use, close)."""
    free = []
    for c in range(CYCLES):
        for h in use():
            h.close()
        free.append(free_bytes())
        print(f"{name}: free after cycle {c + 1}: {free[-1]} B ({free[-1] - free[0]:+d})")
    return free


@pytest.mark.parametrize("name", list(USES))
def test_a_closed_handle_holds_no_device_memory(capi, clouds, name):
    free = cycles(name, lambda: USES[name](capi, clouds))
    assert free[-1] == free[1], (name, [f - free[1] for f in free])


def test_a_closed_vgg_encoder_holds_no_device_memory(capi, vgg_layers):
    img = np.random.default_rng(4).random((2, 3, 32, 48), np.float32)

    def use():
        e = capi.VggEncoder()
        e.set_layers(vgg_layers)
        e.forward(img)
        return [e]

    free = cycles("VggEncoder", use)
    assert free[-1] == free[1], [f - free[1] for f in free]


def test_a_view_reads_the_rows_its_parent_has_now(capi):
    """A view made before the parent grew (twice, so that the parent's buffers moved) searches all the rows and returns
    the parent's indices and distance bits; it cannot add; the parent cannot go before it (GLOC_ERR_STATE), and goes
    after it."""
    rng = np.random.default_rng(11)
    rows = rng.standard_normal((5000, 128)).astype(np.float32)
    q = rows[::250] + rng.standard_normal((20, 128)).astype(np.float32) * 0.05
    ix = capi.KnnIndex(128)
    ix.add(rows[:300])
    v = ix.view()
    assert len(v) == 300
    v.search(q, 5)
    ix.add(rows[300:2000])
    ix.add(rows[2000:])
    assert len(v) == len(ix) == 5000
    for algo in (capi.ALGO_EXACT, capi.ALGO_MFMA):
        ix.set_option(capi.KNN_OPT_ALGO, algo)
        v.set_option(capi.KNN_OPT_ALGO, algo)
        pi, pd = ix.search(q, 10)
        vi, vd = v.search(q, 10)
        assert (pi[:, 0] == np.arange(0, 5000, 250)).all()
        assert (vi == pi).all() and (bits(vd) == bits(pd)).all()
    assert v.device_rows() == ix.device_rows()
    with pytest.raises(capi.GlocError) as e:
        v.add(rows[:1])
    assert e.value.code == GLOC_ERR_STATE
    with pytest.raises(capi.GlocError) as e:
        ix.close()
    assert e.value.code == GLOC_ERR_STATE
    pi2, pd2 = ix.search(q, 10)     # (the refused destroy tore nothing down)
    assert (pi2 == pi).all() and (bits(pd2) == bits(pd)).all()
    v.close()
    ix.close()


def test_a_store_outlives_the_handles_attached_to_it(capi, clouds):
    st = capi.ScanStore()
    a, b = (st.add(c[:, :3]) for c in clouds)
    r = capi.Registrar(store=st)
    with pytest.raises(capi.GlocError) as e:
        st.close()
    assert e.value.code == GLOC_ERR_STATE
    out = r.batch_ids(b, [a], params=capi.default_reg_params(ransac_iters=100, icp_iters=3))   # (nothing was torn down)
    assert out["ok"][0]
    r.close()
    st.close()
