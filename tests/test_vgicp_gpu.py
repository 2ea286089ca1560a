"""GPU: voxelized generalized ICP (gloc_reg_vgicp_voxels, gloc_reg_vgicp_system, gloc_reg_vgicp_batch_ids) against the
float64 restatement tests/vgicp_ref.py: the voxel maps, the normal equations of one pass across neighbourhoods, gates,
source sizes and edge targets, whole alignments over tests/vgicp_cases.py, batching and determinism, targets with and
without a target index, the handle's lifecycle.

Tolerances are those of tests/test_gicp_gpu.py and no others: the restatement's own floor on the test's inputs -- the
sums of a voxel and of the pairs taken forward and reversed, M by numpy.linalg.inv and by the adjugate -- times 10, which
must stay under gn_cases.SYSTEM_CAP (systems, voxels) and POSE_CAP (poses, plus twice the fp32 rounding of the
restatement's pose); rmse to 1e-6 relative; keys, counts, status and iters exact.  The restatement takes the normals the
device built (tests/test_p2l_gpu.py pins those to the oracle's bit for bit).  Measured figures: DESIGN.md."""
import numpy as np
import pytest

import gn_cases as GC
import vgicp_cases as VC
import vgicp_ref as V
from util import bits

pytestmark = pytest.mark.gpu

SYSTEM_CAP, POSE_CAP = GC.SYSTEM_CAP, GC.POSE_CAP
GLOC_ERR_INVALID, GLOC_ERR_STATE = 1, 5
RESOLUTIONS = (0.05, 0.5, 1.0, 4.0)    # 0.05: nearly every voxel of a scan holds one point; 4.0: hundreds in some


class Dev:
    """A scan store and a registrar with the clouds of gn_cases uploaded by name -- uploaded only: no normals, no index."""

    def __init__(self, capi, index=False):
        self.capi, self.index = capi, index
        self.store = capi.ScanStore()
        self.reg = capi.Registrar(store=self.store)
        self.ids = {}

    def id(self, name):
        if name not in self.ids:
            self.ids[name] = self.store.add(GC.cloud(name))
            if self.index and len(GC.cloud(name)) and name != "a2":        # (a2 is the tests' source: the same order on both sides)
                self.store.build_target_index(self.ids[name])
        return self.ids[name]

    def normals(self, name):
        """The cloud's normals as the device built them (k = 10), upload order; built here if no call has yet."""
        if not len(GC.cloud(name)):
            return np.zeros((0, 3), np.float32)
        self.store.build_normals(self.id(name), GC.NORMAL_K)
        return self.store.normals(self.id(name))

    def prm(self, case=None, **over):
        return self.capi.default_vgicp_params(**(VC.params(case) if case else over))

    def batch(self, src, tgts, init, prm):
        return self.reg.vgicp_batch(self.id(src), [self.id(t) for t in tgts], init_T=np.ascontiguousarray(init, np.float32), params=prm)

    def run(self, case):
        return self.batch(case["src"], [case["tgt"]], VC.guess(case)[None], self.prm(case))

    def close(self):
        self.reg.close()
        self.store.close()


@pytest.fixture(scope="module")
def dev(capi):
    d = Dev(capi)
    yield d
    d.close()


_VOX = {}


def _voxels(dev, name, res, order="forward", min_points=1):
    """The restatement's voxel map of a cloud (made once per process and left alone)."""
    key = (name, res, order, min_points)
    if key not in _VOX:
        _VOX[key] = V.voxels(GC.cloud(name), dev.normals(name), res, min_points, order)
    return _VOX[key]


_REFS = {}


def _ref(dev, name):
    """The restatement's verdict on a case (made once per process and left alone)."""
    if name not in _REFS:
        _REFS[name] = VC.reference(VC.by_name(name), dev.normals)
    return _REFS[name]


def _same(a, b):
    return bool((bits(a[0]) == bits(b[0])).all() and (bits(a[1]) == bits(b[1])).all() and (a[2] == b[2]).all() and (a[3] == b[3]).all())


def _rel(a, b, scale):
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max(), abs(a[2] - b[2])) / scale


# ---- 1. the voxel maps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", RESOLUTIONS)
def test_voxels_match_the_restatement(dev, res):
    seen = []
    for name in ("a0", "a0_odd", "a0_dup", "a0_zn", "empty"):
        for min_points in (1, 3):
            got = dev.reg.vgicp_voxels(dev.id(name), dev.prm(resolution=res, min_points=min_points))
            ref, rev = _voxels(dev, name, res, "forward", min_points), _voxels(dev, name, res, "reversed", min_points)
            assert (got["key3"] == ref["key3"]).all() and got["key3"].shape == ref["key3"].shape, (name, res)
            assert (got["count"] == ref["count"]).all()
            if not len(ref["count"]):                                          # (an empty cloud, or no voxel of min_points)
                assert name == "empty" or min_points == 3
                continue
            scale = np.abs(ref["mean"]).max()
            floor = max(np.abs(ref["mean"] - rev["mean"]).max() / scale, np.abs(ref["nn6"] - rev["nn6"]).max())
            err = max(np.abs(got["mean"] - ref["mean"]).max() / scale, np.abs(got["nn6"] - ref["nn6"]).max())
            seen.append((floor, err))
            print(f"{name} res {res} min_points {min_points}: {len(ref['count'])} voxels, {(ref['count'] == 1).mean():.2f} of one point, largest "
                  f"{ref['count'].max()}; floor {floor:.3e} -> tolerance {10 * floor:.3e}; device error {err:.3e}")
            assert 10 * floor <= SYSTEM_CAP and err <= 10 * floor
            order = np.lexsort((got["key3"][:, 2], got["key3"][:, 1], got["key3"][:, 0]))
            assert (order == np.arange(len(order))).all()                     # sorted by (kx, ky, kz)
            if name == "a0_zn":
                assert not got["nn6"].any()                                   # no normals: Nbar = 0
    one = (_voxels(dev, "a0", res)["count"] == 1).mean()
    assert res != 0.05 or one > 0.9                                           # most voxels hold one point
    assert res != 4.0 or _voxels(dev, "a0", res)["count"].max() > 64          # some voxel holds more than 64
    a = np.array(seen)
    print(f"res {res}: floor {a[:, 0].min():.1e} .. {a[:, 0].max():.1e}, device error {a[:, 1].min():.1e} .. {a[:, 1].max():.1e}")
    small, m = np.empty((1, 3), np.int32), dev.capi.C.c_size_t()             # buffers too small: refused, the count still returned
    with pytest.raises(dev.capi.GlocError) as e:
        dev.capi.check(dev.capi.lib().gloc_reg_vgicp_voxels(dev.reg._h, dev.id("a0"), dev.capi.C.byref(dev.prm(resolution=res)), 1,
                                                            small.ctypes.data, None, None, None, dev.capi.C.byref(m)))
    assert e.value.code == GLOC_ERR_INVALID and m.value == len(_voxels(dev, "a0", res)["count"])


# ---- 2. the systems -----------------------------------------------------------------------------------------------------------
SYSTEM_PAIRS = [(s, "a0") for s in GC.EDGE_SOURCES] + [("a2", t) for t in GC.EDGE_TARGETS] + [("a2_odd", "a0_odd"), ("a2", "a0")]


def _ref_system(dev, s, t, T, res, nb, gate):
    """The restatement's system, its scale and its own floor (the order of every sum; the inverse)."""
    sn = dev.normals(s)
    fwd, rev = _voxels(dev, t, res), _voxels(dev, t, res, "reversed")
    R = V.rotation(T)
    pq = V.pairs(GC.cloud(s), sn, fwd, T, res, nb, gate)
    ref = V.system_of_pairs(*pq, R)
    floors = [V.system_of_pairs(*V.pairs(GC.cloud(s), sn, rev, T, res, nb, gate), R, order="reversed"), V.system_of_pairs(*pq, R, how="adj")]
    scale = max(np.abs(ref[0]).max(), np.abs(ref[1]).max(), ref[2], 1e-300)
    assert all(f[3] == ref[3] for f in floors)
    return ref, scale, max(_rel(ref, f, scale) for f in floors)


@pytest.mark.parametrize("nb", [1, 7, 27])
def test_systems_on_edge_inputs_and_sizes(dev, nb):
    seen = []
    for s, t in SYSTEM_PAIRS:
        for gate, res in ((0.0, 1.0), (0.5, 1.0), (0.0, 4.0)):
            T = GC.guess(GC._case("x", "vgicp", s, t, yaw=0.7, t=(0.08, -0.05, 0.02)))
            H, g, s2, cnt = dev.reg.vgicp_system(dev.id(s), dev.id(t), T, dev.prm(max_corr_dist=gate, resolution=res, neighbors=nb))
            ref, scale, floor = _ref_system(dev, s, t, T, res, nb, gate)
            tol, err = 10 * floor, _rel((H, g, s2), ref, scale)
            seen.append((floor, tol, err))
            print(f"{s} -> {t} neighbors {nb} gate {gate} res {res}: pairs {cnt} / {ref[3]} of {len(GC.cloud(s))} points, floor {floor:.3e} -> "
                  f"tolerance {tol:.3e}; device error {err:.3e}")
            assert tol <= SYSTEM_CAP
            assert cnt == ref[3]
            assert (H == H.T).all() and np.isfinite(H).all() and np.isfinite(g).all()
            assert err <= tol
            if ref[3] == 0:
                assert not H.any() and not g.any() and s2 == 0.0
    a = np.array(seen)
    print(f"neighbors {nb}: floor {a[:, 0].min():.1e} .. {a[:, 0].max():.1e}, tolerance {a[:, 1].min():.1e} .. {a[:, 1].max():.1e}, "
          f"device error {a[:, 2].min():.1e} .. {a[:, 2].max():.1e}")
    # more neighbours, more pairs; a gate, fewer
    T = GC.guess(GC._case("x", "vgicp", "a2", "a0", yaw=0.7, t=(0.08, -0.05, 0.02)))
    c = [dev.reg.vgicp_system(dev.id("a2"), dev.id("a0"), T, dev.prm(neighbors=k))[3] for k in (1, 7, 27)]
    assert 1000 < c[0] < c[1] < c[2]
    assert dev.reg.vgicp_system(dev.id("a2"), dev.id("a0"), T, dev.prm(neighbors=nb, max_corr_dist=0.5))[3] < c[(1, 7, 27).index(nb)]


@pytest.mark.parametrize("nb", [1, 7, 27])
def test_no_source_point_in_any_voxel(dev, nb):
    away = GC.guess(GC._case("x", "vgicp", "a2", "a0", yaw=1.0, t=GC.FAR))
    H, g, s2, cnt = dev.reg.vgicp_system(dev.id("a2"), dev.id("a0"), away, dev.prm(neighbors=nb))
    assert cnt == 0 and not H.any() and not g.any() and s2 == 0.0
    near = GC.guess(GC._case("x", "vgicp", "a2", "a0", yaw=1.0, t=(0.1, 0.0, 0.0)))
    T, rmse, iters, status = dev.batch("a2", ["a0", "a0"], np.stack([away, near]), dev.prm(neighbors=nb, max_iters=5))
    assert status[0] == 2 and iters[0] == 0 and rmse[0] == 0 and (bits(T[0]) == bits(away)).all()
    assert status[1] == 0 and iters[1] == 5                              # the job beside it ran
    # beyond the key range and non-finite: |k| >= 2^20 at 0.5 m voxels, inf, NaN -- no pair, no fault
    for t in (3.0e6, np.inf, np.nan):
        out = near.copy()
        out[0, 3] = t
        assert dev.reg.vgicp_system(dev.id("a2"), dev.id("a0"), out, dev.prm(neighbors=nb, resolution=0.5))[3] == 0


# ---- 3. whole alignments ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in VC.CASES])
def test_alignments_follow_the_restatement(dev, name):
    case = VC.by_name(name)
    r, prm = _ref(dev, name), VC.params(case)
    T, rmse, iters, status = out = dev.run(case)
    assert np.isfinite(T).all() and status[0] in (0, 1, 2) and iters[0] <= prm["max_iters"]
    assert _same(out, dev.run(case))                                        # the same bits on a second run
    if status[0] == 2 and iters[0] == 0:
        assert (bits(T[0]) == bits(VC.guess(case))).all()                   # degenerate at once: the guess comes back
    if not r["stable"]:
        print(f"{name}: unstable in the restatement, held only to what holds regardless")
        return
    ref = r["ref"]
    ft, fa = r["floor"]
    ot, oa = V.pose_err(ref["T"], ref["T"].astype(np.float32))
    dt, da = V.pose_err(ref["T"], T[0])
    print(f"{name}: iters {iters[0]} / {ref['iters']}, status {status[0]} / {ref['status']}, rmse {rmse[0]:.6f} / {ref['rmse']:.6f}; "
          f"floor {ft:.2e} m {fa:.2e} rad, fp32 output {ot:.2e} m {oa:.2e} rad; against the restatement {dt:.2e} m {da:.2e} rad")
    assert 10 * ft <= POSE_CAP and 10 * fa <= POSE_CAP
    assert status[0] == ref["status"]
    assert int(iters[0]) == ref["iters"]
    assert dt <= 10 * ft + 2 * ot and da <= 10 * fa + 2 * oa
    assert abs(rmse[0] - ref["rmse"]) <= 1e-6 * max(ref["rmse"], 1.0)


def test_at_most_a_tenth_of_the_cases_is_unstable(dev):
    """(The references are those of the test above: nothing is computed again when both run.)"""
    stable = [_ref(dev, c["name"])["stable"] for c in VC.CASES]
    print(f"{sum(stable)} of {len(stable)} cases stable")
    assert len(stable) - sum(stable) <= VC.MAX_UNSTABLE * len(stable)


def test_a_mixed_batch_equals_single_calls_bit_for_bit(dev):
    refs = {n: _ref(dev, n) for n in VC.MIXED}
    cs = [VC.by_name(n) for n in VC.MIXED]
    assert len(cs) >= 6
    prm = dev.prm(cs[0])
    init = np.stack([VC.guess(c) for c in cs])
    tgts = [c["tgt"] for c in cs]
    T, rmse, iters, status = out = dev.batch("a2", tgts, init, prm)
    assert _same(out, dev.batch("a2", tgts, init, prm))
    print(f"mixed batch: status {status.tolist()}, iters {iters.tolist()}")
    assert all(refs[n]["stable"] for n in VC.MIXED)
    assert status.tolist() == [refs[n]["ref"]["status"] for n in VC.MIXED] and iters.tolist() == [refs[n]["ref"]["iters"] for n in VC.MIXED]
    assert {int(s) for s in status} == {0, 1, 2} and len({int(i) for i, s in zip(iters, status) if s == 1}) >= 2
    for j, c in enumerate(cs):
        one = dev.run(c)
        assert _same(one, (T[j:j + 1], rmse[j:j + 1], iters[j:j + 1], status[j:j + 1])), c["name"]
        if status[j] == 1:
            # a job that stopped holds the pose of a run of exactly that many updates with the stop test off
            p = dict(VC.params(c), max_iters=int(iters[j]), trans_eps=0.0, rot_eps=0.0)
            T0, _, i0, s0 = dev.batch("a2", [c["tgt"]], init[j:j + 1], dev.prm(**p))
            assert i0[0] == iters[j] and s0[0] == 0 and (bits(T0[0]) == bits(T[j])).all(), c["name"]
    # the same jobs many times over, in another order: every job still its single call
    order = [(3 * j) % len(cs) for j in range(50)]
    T2, rmse2, iters2, status2 = dev.batch("a2", [tgts[j] for j in order], init[order], prm)
    for k, j in enumerate(order):
        assert (bits(T2[k]) == bits(T[j])).all() and bits(rmse2)[k] == bits(rmse)[j] and iters2[k] == iters[j] and status2[k] == status[j]


# ---- 4. no target index needed ------------------------------------------------------------------------------------------------
def test_a_target_without_a_target_index_gives_the_same_bits(capi, dev):
    """The voxels are summed in upload order, whatever order the store keeps the scan in."""
    d = Dev(capi, index=True)                                             # the same clouds, every target with a kd-ordered target index
    try:
        for name in ("a0", "a0_odd"):
            for res in (0.5, 4.0):
                a, b = d.reg.vgicp_voxels(d.id(name), d.prm(resolution=res)), dev.reg.vgicp_voxels(dev.id(name), dev.prm(resolution=res))
                assert all((bits(a[k]) == bits(b[k])).all() if a[k].dtype.kind == "f" else (a[k] == b[k]).all() for k in a), (name, res)
        cs = [VC.by_name(n) for n in VC.MIXED]
        init = np.stack([VC.guess(c) for c in cs])
        for nb in (1, 7, 27):
            prm = dict(VC.params(cs[0]), neighbors=nb)
            assert _same(d.batch("a2", [c["tgt"] for c in cs], init, d.prm(**prm)), dev.batch("a2", [c["tgt"] for c in cs], init, dev.prm(**prm))), nb
            sa, sb = d.reg.vgicp_system(d.id("a2"), d.id("a0"), init[1], d.prm(**prm)), dev.reg.vgicp_system(dev.id("a2"), dev.id("a0"), init[1], dev.prm(**prm))
            assert sa[3] == sb[3] and (bits(sa[0]) == bits(sb[0])).all() and (bits(sa[1]) == bits(sb[1])).all() and sa[2] == sb[2]
    finally:
        d.close()


# ---- 5. normals on demand, refusals, the handle's lifecycle -------------------------------------------------------------------
def test_normals_are_built_on_demand_and_refusals(capi):
    d = Dev(capi)
    try:
        src, tgt = d.id("a2_n257"), d.id("a0_odd")
        with pytest.raises(capi.GlocError) as e:
            d.store.normals(tgt)
        assert e.value.code == GLOC_ERR_STATE
        live0, _ = d.store.bytes()
        T = GC.guess(GC._case("x", "vgicp", "a2", "a0", yaw=0.7, t=(0.08, -0.05, 0.02)))
        a = d.reg.vgicp_system(src, tgt, T)                               # builds both scans' normals with normal_k = 10
        assert d.store.bytes()[0] - live0 == 12 * (257 + len(GC.cloud("a0_odd")))
        b = d.reg.vgicp_system(src, tgt, T, d.prm(normal_k=5))            # existing normals are used as they are
        assert a[3] == b[3] > 0 and (bits(a[0]) == bits(b[0])).all() and d.store.bytes()[0] - live0 == 12 * (257 + len(GC.cloud("a0_odd")))
        for bad in (dict(normal_k=2), dict(plane_eps=0.0), dict(max_iters=0), dict(resolution=0.0), dict(neighbors=6), dict(min_points=0)):
            with pytest.raises(capi.GlocError) as e:
                d.reg.vgicp_batch(src, [tgt], params=d.prm(**bad))
            assert e.value.code == GLOC_ERR_INVALID, bad
        for call in (lambda: d.reg.vgicp_batch(10 ** 6, [tgt]), lambda: d.reg.vgicp_batch(src, [10 ** 6]), lambda: d.reg.vgicp_voxels(10 ** 6),
                     lambda: d.reg.vgicp_batch(d.id("empty"), [tgt]), lambda: d.reg.vgicp_batch(src, [])):
            with pytest.raises(capi.GlocError) as e:
                call()
            assert e.value.code == GLOC_ERR_INVALID
        d.reg.batch_multi_begin([src], [[tgt]], params=capi.default_reg_params(ransac_iters=0, icp_iters=2))
        for call in (lambda: d.reg.vgicp_batch(src, [tgt]), lambda: d.reg.vgicp_system(src, tgt), lambda: d.reg.vgicp_voxels(tgt)):
            with pytest.raises(capi.GlocError) as e:
                call()
            assert e.value.code == GLOC_ERR_STATE
        d.reg.batch_multi_end()
    finally:
        d.close()


def test_handle_lifecycle_and_a_workspace_shared_with_generalized_icp(capi):
    """Create, refine, destroy, create again; and on ONE handle generalized ICP (which leaves its targets and partials in the
    shared Gauss-Newton workspace), then the voxelized refinement, then a smaller batch and a shorter source: each call
    equals the same call on a fresh handle bit for bit."""
    cs = [VC.by_name(n) for n in VC.MIXED]
    init = np.stack([VC.guess(c) for c in cs])
    tgts = [c["tgt"] for c in cs]

    def call(d, kind, src, n):
        if kind == "gicp":
            return d.reg.gicp_batch(d.id(src), [d.id(t) for t in tgts[:n]], init_T=init[:n], params=capi.default_gicp_params(max_iters=3, max_corr_dist=1.0))
        return d.batch(src, tgts[:n], init[:n], d.prm(cs[0]))

    first = Dev(capi)
    want = {k: call(first, "vgicp", *k) for k in (("a2", 7), ("a2", 2), ("a2_n65", 5))}
    first.close()                                                         # destroyed with its workspaces ...
    d = Dev(capi)                                                         # ... and a new one made
    try:
        for kind, src, n in (("vgicp", "a2", 7), ("gicp", "a2", 7), ("vgicp", "a2", 7), ("vgicp", "a2", 2), ("gicp", "a2_n65", 3), ("vgicp", "a2_n65", 5),
                             ("vgicp", "a2", 7)):
            got = call(d, kind, src, n)
            if kind == "vgicp":
                assert _same(got, want[(src, n)]), (kind, src, n)
        live = d.store.bytes()[0]
        for sid in d.ids.values():
            d.store.release(sid)
        assert d.store.bytes()[0] < live
    finally:
        d.close()


def test_ndt_and_vgicp_interleaved_on_one_handle_equal_fresh_handles(capi):
    """NDT and the voxelized refinement build their maps with one builder, each in a workspace of its own: called in turn on
    ONE handle -- maps of one scan, batches over [A, empty, A, 70 points] (a repeated id, an empty target, a table of the
    minimum size), then maps of another scan -- every call equals the same call made alone on a fresh handle, bit for bit.
    NDT at 0.5 m and the voxelized refinement at 1.0 m: the two maps of a scan differ."""
    from gloc3d_amd import synth
    world = synth.make_world(1001)
    a = np.ascontiguousarray(synth.lidar_scan(world, None, seed=1001, n_az=32)[:, :3])
    s = np.ascontiguousarray(synth.lidar_scan(world, synth.se3(2.0, (0.3, -0.2, 0.05)), seed=1002, n_az=32)[:, :3])
    c = np.ascontiguousarray(a[::len(a) // 70][:70])
    assert 1900 < len(a) < 2100 and 1900 < len(s) < 2100 and len(c) == 70
    store = capi.ScanStore()
    src, A, B, C = (store.add(x) for x in (s, a, np.zeros((0, 3), np.float32), c))
    tgts = [A, B, A, C]
    ndt, vg = capi.default_ndt_params(resolution=0.5), capi.default_vgicp_params(resolution=1.0, neighbors=7, max_iters=3)
    steps = [("ndt_cells A", lambda r: r.ndt_cells(A, ndt)), ("vgicp_voxels A", lambda r: r.vgicp_voxels(A, vg)),
             ("ndt_batch", lambda r: r.ndt_batch(src, tgts, params=ndt)), ("vgicp_batch", lambda r: r.vgicp_batch(src, tgts, params=vg)),
             ("ndt_cells C", lambda r: r.ndt_cells(C, ndt)), ("vgicp_voxels C", lambda r: r.vgicp_voxels(C, vg)),
             ("ndt_batch again", lambda r: r.ndt_batch(src, tgts, params=ndt))]

    def arrays(out):
        return [out[k] for k in sorted(out)] if isinstance(out, dict) else list(out)

    one = capi.Registrar(store=store)
    try:
        for name, call in steps:
            fresh = capi.Registrar(store=store)
            try:
                want = arrays(call(fresh))
            finally:
                fresh.close()
            got = arrays(call(one))
            assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want)), name
            if name == "ndt_cells A":
                assert len(got[0]) > 0                                          # (there are cells to compare)
            if name == "vgicp_voxels A":
                assert len(got[0]) > 100
    finally:
        one.close()
        store.close()
