"""GPU: the robust weighting of the three Gauss-Newton refinements (gloc_reg_{p2l,gicp,vgicp}_*_robust) against the float64
restatement tests/robust_ref.py -- the weighted systems of every kind across the shapes of the reduction, the kinks of
Huber and Tukey on residuals that are exact, kind NONE against the plain entries bit for bit, whole alignments over the
case table tests/test_robust_ref_cpu.py proves stable, the schedule's hold on the stop test, a batch whose weights are
all zero beside one whose are all one, mixed batches, refusals.

Tolerances: a system within SYSTEM_CAP (1e-9) of its largest entry; a pose within 1e-4 m / 1e-4 rad and an rmse within 1e-4
(tests/test_p2l_gpu.py's); the mean weight within 1e-6; counts, status and, without eps, iterations exact."""
import numpy as np
import pytest

import gicp_ref as G
import gn_cases as GC
import p2l_ref as P
import robust_cases as RC
import robust_ref as RR
import vgicp_ref as V
from util import bits

pytestmark = pytest.mark.gpu

SYSTEM_CAP = GC.SYSTEM_CAP
INVALID, STATE = 1, 5
SYSTEM_SOURCES = tuple("a2_n%d" % n for n in (1, 5, 6, 63, 64, 65, 255, 256, 257)) + ("a2",)


class Dev:
    """A scan store and a registrar with clouds uploaded by name (robust_cases.cloud; normals built with k = 10)."""

    def __init__(self, capi):
        self.capi = capi
        self.store = capi.ScanStore()
        self.reg = capi.Registrar(store=self.store)
        self.ids = {}

    def add(self, name, xyz):
        self.ids[name] = self.store.add(np.ascontiguousarray(xyz, np.float32))
        if len(xyz):
            self.store.build_normals(self.ids[name], GC.NORMAL_K)
        return self.ids[name]

    def id(self, name):
        return self.ids[name] if name in self.ids else self.add(name, RC.cloud(name))

    def prm(self, method, **p):
        if method == "p2l":
            p = {k: v for k, v in p.items() if k != "plane_eps"}
        return getattr(self.capi, "default_%s_params" % method)(**p)

    def rb(self, block):
        return None if block is None else self.capi.default_robust_params(**block)

    def batch(self, method, src, tgts, init, prm, block=None):
        return getattr(self.reg, method + "_batch")(self.id(src), [self.id(t) for t in tgts], init_T=np.ascontiguousarray(init, np.float32),
                                                    params=prm, robust=self.rb(block))

    def system(self, method, src, tgt, T, prm, block=None, k=0):
        return getattr(self.reg, method + "_system")(self.id(src), self.id(tgt), np.ascontiguousarray(T, np.float32), prm,
                                                     robust=self.rb(block), robust_pass=k)

    def run(self, case):
        return self.batch(case["method"], case["src"], [case["tgt"]], RC.guess(case)[None], self.prm(case["method"], **RC.params(case)),
                          case["robust"])

    def close(self):
        self.reg.close()
        self.store.close()


@pytest.fixture(scope="module")
def dev(capi):
    d = Dev(capi)
    yield d
    d.close()


def _same(a, b):
    return bool(all((bits(x) == bits(y)).all() for x, y in ((a[0], b[0]), (a[1], b[1]))) and (a[2] == b[2]).all() and (a[3] == b[3]).all()
                and (len(a) < 5 or (bits(a[4]) == bits(b[4])).all()))


def _row(out, j):
    return tuple(o[j:j + 1] for o in out)


# ---- 1. the weighted systems ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", RC.METHODS)
def test_systems_match_the_restatement(dev, oracle_mod, method):
    """Every kind at pass 0 of no schedule and at pass 1 of one (4 c, 2 c, c: a scale that is neither end), on sources of
    1 .. 257 points and a whole scan: H, g, the squared sum and the weights' sum within SYSTEM_CAP of the largest of them."""
    nn = GC.finite_nn(oracle_mod)
    tgt, tn = GC.cloud("a0"), GC.normals("a0", oracle_mod)
    vox = V.voxels(tgt, tn) if method == "vgicp" else None
    T = (GC.truth("a2", "a0") @ GC._se3(0.7, (0.08, -0.05, 0.02))).astype(np.float32)
    prm = dev.prm(method, max_corr_dist=1.0)
    worst = 0.0
    for s in SYSTEM_SOURCES:
        src, sn = GC.cloud(s), GC.normals(s, oracle_mod)
        if method == "p2l":
            pq = P.pairs(src, tgt, tn, T, nn, 1.0)
            ref_of = lambda rb, c: RR.p2l_system_of_pairs(*pq, rb, c)
        elif method == "gicp":
            pq = G.pairs(src, sn, tgt, tn, T, nn, 1.0)
            ref_of = lambda rb, c: RR.gicp_system_of_pairs(*pq, G.rotation(T), rb, c)
        else:
            pq = V.pairs(src, sn, vox, T, 1.0, 7, 1.0)
            ref_of = lambda rb, c: RR.vgicp_system_of_pairs(*pq, G.rotation(T), rb, c)
        for kind in RR.KINDS:
            for rb, k in ((RC.robust(method, kind), 0), (RC.robust(method, kind, 4.0, 0.5), 1)):
                c = RR.scale(rb, k)
                assert c == rb["scale"] * (1 if k == 0 else 2)
                H, g, s2, cnt, wsum = dev.system(method, s, "a0", T, prm, rb, k)
                Hr, gr, s2r, cntr, wr = ref_of(rb, c)
                scale = max(np.abs(Hr).max(), np.abs(gr).max(), s2r, wr, 1e-300) if cntr else 1.0
                err = max(np.abs(H - Hr).max(), np.abs(g - gr).max(), abs(s2 - s2r), abs(wsum - wr)) / scale
                worst = max(worst, err)
                assert cnt == cntr, (s, kind, k)
                assert (H == H.T).all() and np.isfinite(H).all() and np.isfinite(g).all()
                assert 0.0 <= wsum <= cnt
                assert err <= SYSTEM_CAP, (s, kind, k, err)
    print(f"{method}: worst system error {worst:.3e} of the largest entry")


# ---- 2. the kinks, on residuals that are exact -------------------------------------------------------------------------------------
def test_huber_and_tukey_at_their_kinks(dev, capi):
    """A plane lattice at z = -2 (spacing 0.25: normals exactly +-z), sources directly above lattice points: the residual is
    the height + 2, exact in fp64.  scale 0.5: the kink is at height -1.5.  One pair a system, so a sum has one order: the
    weights' sum and g equal the restatement's, bit for bit."""
    u = np.arange(0.0, 3.0, 0.25, dtype=np.float32)
    lat = np.stack([np.repeat(u, len(u)) + 1.0, np.tile(u, len(u)) + 0.5, np.full(len(u) ** 2, -2.0, np.float32)], 1)
    tid = dev.add("lattice", lat)
    n = dev.store.normals(tid)
    assert (n[:, :2] == 0).all() and (np.abs(n[:, 2]) == 1).all()
    below, above = np.nextafter(np.float32(-1.5), np.float32(-2)), np.nextafter(np.float32(-1.5), np.float32(-1))
    heights = [0.0, 0.25, 0.5, float(below), -1.5, float(above), 1.0]
    at = lat[5 * len(u) + 7]
    nn = lambda p, t: (np.array([np.argmin(((t.astype(np.float64) - x) ** 2).sum(1)) for x in p.astype(np.float64)], np.uint32),
                       np.array([((t.astype(np.float64) - x) ** 2).sum(1).min() for x in p.astype(np.float64)], np.float32))
    prm = dev.prm("p2l")
    for kind in (RR.HUBER, RR.TUKEY):
        rb = RR.block(kind, 0.5)
        for i, h in enumerate(heights):
            src = np.array([[at[0], at[1], h]], np.float32)
            if "above%d" % i not in dev.ids:
                dev.add("above%d" % i, src)
            H, g, s2, cnt, wsum = dev.system("p2l", "above%d" % i, "lattice", np.eye(4), prm, rb)
            Hr, gr, s2r, cntr, wr = RR.p2l_system(src, lat, n, np.eye(4), nn, rb, 0.5)
            r = np.float64(np.float32(h)) + 2.0
            assert cnt == cntr == 1 and s2 == s2r == r * r
            assert wsum == wr and (g == gr).all() and (H == Hr).all(), (kind, h)
            if h == -1.5:                                       # the exact kink: Huber still counts the pair fully, Tukey not at all
                assert wsum == (1.0 if kind == RR.HUBER else 0.0)
            if h == float(below):                               # just inside
                assert wsum == 1.0 if kind == RR.HUBER else 0.0 < wsum < 1e-12
            if h == float(above):                               # just outside
                assert 1.0 - 1e-6 < wsum < 1.0 if kind == RR.HUBER else wsum == 0.0
        # ... and all seven at once, to the systems' bound
        every = np.array([[lat[k * len(u) + 3 + k][0], lat[k * len(u) + 3 + k][1], h] for k, h in enumerate(heights)], np.float32)
        if "above_all" not in dev.ids:
            dev.add("above_all", every)
        H, g, s2, cnt, wsum = dev.system("p2l", "above_all", "lattice", np.eye(4), prm, rb)
        Hr, gr, s2r, cntr, wr = RR.p2l_system(every, lat, n, np.eye(4), nn, rb, 0.5)
        scale = max(np.abs(Hr).max(), np.abs(gr).max(), s2r, wr)
        assert cnt == cntr == 7 and max(np.abs(H - Hr).max(), np.abs(g - gr).max(), abs(s2 - s2r), abs(wsum - wr)) <= SYSTEM_CAP * scale


# ---- 3. kind NONE is the plain entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", RC.METHODS)
def test_kind_none_equals_the_plain_entries_bit_for_bit(dev, method):
    none = RR.block()
    junk = dict(kind=0, scale=-1.0, scale_start=float("nan"), anneal=7.0)         # (NONE: the other fields are ignored)
    tg = ["a0", "b0", "empty", "a0"]
    init = np.stack([RC.truth("a2", "a0") @ GC._se3(0.5 * j, (0.05 * j, -0.03, 0.01)) for j in range(4)]).astype(np.float32)
    for p in (dict(max_iters=5, max_corr_dist=1.0), dict(max_iters=12, max_corr_dist=1.0, trans_eps=2e-3, rot_eps=2e-4)):
        prm = dev.prm(method, **p)
        plain = dev.batch(method, "a2", tg, init, prm)
        for block in (none, junk):
            got = dev.batch(method, "a2", tg, init, prm, block)
            assert _same(plain, got[:4])
            assert got[4].tolist() == [1.0, 1.0, 0.0, 1.0]                         # exactly 1 where there are pairs
    prm = dev.prm(method, max_corr_dist=1.0)
    for t in ("a0", "empty"):
        H, g, s, c = dev.system(method, "a2", t, init[1], prm)
        for k in (0, 3):
            H2, g2, s2, c2, w2 = dev.system(method, "a2", t, init[1], prm, none, k)
            assert (H.view(np.uint64) == H2.view(np.uint64)).all() and (g.view(np.uint64) == g2.view(np.uint64)).all()
            assert s == s2 and c == c2 and w2 == float(c)
        assert (c > 1000) == (t == "a0")


# ---- 4. whole alignments over the proven table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in RC.CASES])
def test_an_alignment_follows_the_restatement(dev, oracle_mod, name):
    """Every case of the table, which tests/test_robust_ref_cpu.py proves stable (the restatement run here is the first of
    the two it compares there)."""
    case = RC.by_name(name)
    prm, ref = RC.params(case), RC.run(case, oracle_mod)
    T, rmse, iters, status, weight = out = dev.run(case)
    assert _same(out, dev.run(case))                                                # the same bits on a second run
    dt, da = P.pose_err(ref["T"], T[0])
    print(f"{name}: iters {iters[0]} / {ref['iters']}, status {status[0]} / {ref['status']}, rmse {rmse[0]:.6f} / {ref['rmse']:.6f}, "
          f"mean weight {weight[0]:.6f} / {ref['weight']:.6f}; against the restatement {dt:.2e} m {da:.2e} rad")
    assert dt <= 1e-4 and da <= 1e-4
    assert status[0] == ref["status"]
    eps = prm["trans_eps"] > 0 and prm["rot_eps"] > 0
    assert abs(int(iters[0]) - ref["iters"]) <= 1 if eps else int(iters[0]) == ref["iters"]
    assert abs(rmse[0] - ref["rmse"]) <= 1e-4 and abs(weight[0] - ref["weight"]) <= 1e-6


@pytest.mark.parametrize("method", RC.METHODS)
def test_the_moved_object_pulls_the_plain_refinement_not_the_robust_one(dev, method):
    """The device shows the ordering tests/test_robust_ref_cpu.py asserts of the restatement: the plain refinement's
    translation error to the truth is more than twice Cauchy's and Tukey's."""
    err = {}
    for k in ("none", "cauchy", "tukey"):
        case = RC.by_name("moved_%s_%s" % (k, method))
        err[k] = P.pose_err(RC.truth(case["src"], case["tgt"]), dev.run(case)[0][0])[0]
    plain, cauchy, tukey = err["none"], err["cauchy"], err["tukey"]
    print(f"{method}, moved object: translation error plain {plain:.4f} m, Cauchy {cauchy:.4f} m, Tukey {tukey:.4f} m")
    assert plain > 2 * cauchy and plain > 2 * tukey


# ---- 5. the schedule holds the stop test -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", RC.METHODS)
def test_the_schedule_holds_the_stop_test(dev, method):
    """eps so large that every update passes the stop test: without a schedule the job stops at its first update; with one
    that settles at update 3 it stops there and not before; with one that has not settled by the cap it never does.  The
    stopped job's pose is that of exactly as many updates with the stop test off, bit for bit."""
    case = RC.by_name("a20_cauchy_" + method)
    init, p = RC.guess(case)[None], dict(RC.params(case), max_iters=8, trans_eps=10.0, rot_eps=10.0)
    off = dict(p, trans_eps=0.0, rot_eps=0.0)
    for block, iters, status in ((RC.robust(method, RR.CAUCHY), 1, 1), (RC.robust(method, RR.CAUCHY, 8.0, 0.5), 4, 1),
                                 (RC.robust(method, RR.CAUCHY, 8.0, 0.999), 8, 0)):
        T, rmse, it, st, w = dev.batch(method, "a2", ["a0"], init, dev.prm(method, **p), block)
        assert (int(it[0]), int(st[0])) == (iters, status), block
        T0, _, it0, st0, w0 = dev.batch(method, "a2", ["a0"], init, dev.prm(method, **dict(off, max_iters=iters)), block)
        assert it0[0] == iters and st0[0] == 0 and (bits(T0) == bits(T)).all() and (bits(w0) == bits(w)).all()


# ---- 6. all weights zero beside all weights one ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", RC.METHODS)
def test_tukey_at_a_tiny_scale(dev, method):
    """Tukey with a scale of a micrometre: every pair of two different corner scenes weighs 0, H is 0, the job is degenerate
    at once and its guess comes back -- and it is still counted (rmse > 0, mean weight 0).  The job beside it matches a
    scene against itself at the identity: its residuals to its own points are zero, their weights one, and it runs as if
    alone."""
    rb = RC.robust(method, RR.TUKEY, scale=1e-6)
    p = dict(max_iters=4, resolution=0.1, neighbors=7) if method == "vgicp" else dict(max_iters=4)
    prm = dev.prm(method, **p)
    init = np.stack([GC._se3(0.4, (0.02, -0.03, -0.04)), np.eye(4)]).astype(np.float32)
    T, rmse, iters, status, weight = out = dev.batch(method, "k1_t", ["k14_t", "k1_t"], init, prm, rb)
    assert status[0] == 2 and iters[0] == 0 and (bits(T[0]) == bits(init[0])).all() and rmse[0] > 0 and weight[0] == 0.0
    # (voxelized: the point's own voxel weighs one, the voxels around it, centimetres off, zero)
    assert status[1] == 0 and iters[1] == 4 and (0.5 < weight[1] < 1.0 if method == "vgicp" else weight[1] == 1.0)
    dt, da = P.pose_err(np.eye(4), T[1])
    assert dt <= 1e-6 and da <= 1e-6
    for j in (0, 1):
        assert _same(_row(out, j), dev.batch(method, "k1_t", [["k14_t", "k1_t"][j]], init[j:j + 1], prm, rb)), j


# ---- 7. a mixed batch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,kind", [("p2l", RR.HUBER), ("gicp", RR.TUKEY), ("vgicp", RR.GEMAN_MCCLURE)])
def test_a_mixed_batch_equals_its_single_calls_bit_for_bit(dev, method, kind):
    tg = ["a0", "b0", "empty", "a0"] * 3
    init = np.stack([RC.truth("a2", "a0") @ GC._se3(0.4 * (j % 5) - 1.0, (0.04 * (j % 7), -0.03, 0.01 * (j % 3))) for j in range(12)]).astype(np.float32)
    prm = dev.prm(method, max_iters=10, max_corr_dist=1.0, trans_eps=2e-3, rot_eps=2e-4)
    for rb in (RC.robust(method, kind), RC.robust(method, RR.CAUCHY, 4.0, 0.5)):
        T, rmse, iters, status, weight = out = dev.batch(method, "a2", tg, init, prm, rb)
        assert _same(out, dev.batch(method, "a2", tg, init, prm, rb))
        print(f"{method} {RR.NAMES[rb['kind']]}: status {status.tolist()}, iters {iters.tolist()}")
        assert (status[2::4] == 2).all() and (weight[2::4] == 0).all() and (status == 1).any() and (weight[0::4] > 0.5).all()
        if rb["scale_start"]:
            assert (iters[status == 1] >= 3).all()                                  # (the schedule settles at update 2)
        for j in range(12):
            assert _same(_row(out, j), dev.batch(method, "a2", [tg[j]], init[j:j + 1], prm, rb)), j


# ---- 8. refusals, and the handle after them ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", RC.METHODS)
def test_refusals_leave_the_handle_usable(dev, capi, method):
    case = RC.by_name("a20_huber_" + method)
    prm, rb, init = dev.prm(method, **RC.params(case)), case["robust"], RC.guess(case)[None]
    want = dev.run(case)
    want_sys = dev.system(method, "a2", "a0", init[0], prm, rb, 1)

    def refused(code, f):
        with pytest.raises(capi.GlocError) as e:
            f()
        assert e.value.code == code
        got, got_sys = dev.run(case), dev.system(method, "a2", "a0", init[0], prm, rb, 1)
        assert _same(want, got) and (want_sys[0] == got_sys[0]).all() and (want_sys[1] == got_sys[1]).all() and want_sys[2:] == got_sys[2:]

    for bad in (dict(kind=5, scale=1.0), dict(kind=1, scale=0.0), dict(kind=2, scale=1.0, scale_start=0.5, anneal=0.5),
                dict(kind=3, scale=1.0, scale_start=2.0, anneal=1.0)):
        refused(INVALID, lambda: dev.batch(method, "a2", ["a0"], init, prm, bad))
        refused(INVALID, lambda: dev.system(method, "a2", "a0", init[0], prm, bad))
    refused(INVALID, lambda: getattr(dev.reg, method + "_batch")(dev.id("a2"), [12345], init_T=init, params=prm, robust=dev.rb(rb)))
    # between batch_multi_begin and _end
    dev.reg.batch_multi_begin([dev.id("a2")], [[dev.id("a0")]], params=capi.default_reg_params(ransac_iters=0, icp_iters=2))
    try:
        for f in (lambda: dev.run(case), lambda: dev.system(method, "a2", "a0", init[0], prm, rb, 1)):
            with pytest.raises(capi.GlocError) as e:
                f()
            assert e.value.code == STATE
    finally:
        dev.reg.batch_multi_end()
    assert _same(want, dev.run(case))
