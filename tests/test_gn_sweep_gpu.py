"""GPU: the two Gauss-Newton refinements (gloc_reg_p2l_*, gloc_reg_gicp_*: gn6.hpp, gn6_kernels.hpp, run_refine in reg.hip)
against the float64 restatements across inputs, sizes and stops -- the accumulate kernels' guards (an empty target,
non-finite and duplicated points, zero normals), the shapes of the reduction (sources of 1 .. 257 points and a full-size
scan), the solve kernel and the host loop over the case list of tests/gn_cases.py (whose coverage of the loop's branches
tests/test_gn_sweep_cpu.py proves on the restatements alone), mixed batches, the search settings, batch sizes and one
handle across many calls.

Tolerances are those of tests/test_gicp_gpu.py and no others: a system within 10 x the restatement's own floor (two
summation orders; for generalized ICP two inverses), which stays under SYSTEM_CAP; a pose within 10 x floor + 2 x the
fp32 output's rounding with 10 x floor under POSE_CAP; rmse to 1e-6 relative; counts, status and iters exact.

The edge inputs' path was read before they were first run: the culled search returns no correspondence (0xFFFFFFFF) for
an empty target (`ix.n &&` before every read of the index: nn_compact.hpp) and for a non-finite source, and a NaN or inf
target never wins (`d2 == d2 && k < bk`); the accumulate kernels read the target only behind `j < T.n`.
tests/test_reg_gpu.py::test_empty_scans and ::test_nn_with_nan_points_in_source_and_target run the same search."""
import numpy as np
import pytest

import gicp_ref as G
import gn_cases as GC
import p2l_ref as P
from util import bits

pytestmark = pytest.mark.gpu

SYSTEM_CAP, POSE_CAP = GC.SYSTEM_CAP, GC.POSE_CAP
GLOC_ERR_INVALID = 1


class Dev:
    """A scan store and a registrar with the clouds of gn_cases uploaded by name (normals built with k = 10)."""

    def __init__(self, capi, kd=False):
        self.capi, self.kd = capi, kd                  # kd: every cloud but the sources' scan "a2" gets a kd-ordered target index
        self.store = capi.ScanStore()
        self.reg = capi.Registrar(store=self.store)
        self.ids = {}

    def id(self, name):
        if name not in self.ids:
            sid = self.store.add(GC.cloud(name))
            if len(GC.cloud(name)):
                self.store.build_normals(sid, GC.NORMAL_K)
                if self.kd and name != "a2":
                    self.store.build_target_index(sid)
            self.ids[name] = sid
        return self.ids[name]

    def prm(self, case_or_method, **over):
        if isinstance(case_or_method, dict):
            m, p = case_or_method["method"], GC.params(case_or_method)
        else:
            m, p = case_or_method, dict(over)
        if m == "p2l":
            p = {k: v for k, v in p.items() if k != "plane_eps"}
            return self.capi.default_p2l_params(**p)
        return self.capi.default_gicp_params(**p)

    def batch(self, method, src, tgts, init, prm):
        f = self.reg.p2l_batch if method == "p2l" else self.reg.gicp_batch
        return f(self.id(src), [self.id(t) for t in tgts], init_T=np.ascontiguousarray(init, np.float32), params=prm)

    def system(self, method, src, tgt, T, prm=None):
        f = self.reg.p2l_system if method == "p2l" else self.reg.gicp_system
        return f(self.id(src), self.id(tgt), np.ascontiguousarray(T, np.float32), prm)

    def run(self, case):
        return self.batch(case["method"], case["src"], [case["tgt"]], GC.guess(case)[None], self.prm(case))

    def close(self):
        self.reg.close()
        self.store.close()


@pytest.fixture(scope="module")
def dev(capi):
    d = Dev(capi)
    yield d
    d.close()


def _same(a, b):
    return bool((bits(a[0]) == bits(b[0])).all() and (bits(a[1]) == bits(b[1])).all() and (a[2] == b[2]).all() and (a[3] == b[3]).all())


def _rel(a, b, scale):
    return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max(), abs(a[2] - b[2])) / scale


def _ref_system(method, src, sn, tgt, tn, T, nn, gate=0.0):
    """The restatement's system, its scale and its own floor (summation order; for generalized ICP also the inverse)."""
    if method == "p2l":
        pq = P.pairs(src, tgt, tn, T, nn, gate)
        ref, rev = P.system_of_pairs(*pq), P.system_of_pairs(*pq, order="reversed")
        floors = [(ref, rev)]
    else:
        p, q, ns, nt = G.pairs(src, sn, tgt, tn, T, nn, gate)
        Rm = G.rotation(T)
        ref = G.system_of_pairs(p, q, ns, nt, Rm)
        floors = [(ref, G.system_of_pairs(p, q, ns, nt, Rm, order="reversed")), (ref, G.system_of_pairs(p, q, ns, nt, Rm, how="adj"))]
    scale = max(np.abs(ref[0]).max(), np.abs(ref[1]).max(), ref[2], 1e-300)
    return ref, scale, max(_rel(a, b, scale) for a, b in floors)


# ---- 1, 2. the systems: guards of the accumulate kernels, shapes of the reduction ---------------------------------------
SYSTEM_PAIRS = [(s, "a0") for s in GC.EDGE_SOURCES] + [("a2", t) for t in GC.EDGE_TARGETS] + [("a2_odd", "a0_odd"), ("a0_dup", "a0_dup"), ("a2", "a0")]


@pytest.mark.parametrize("method", ["p2l", "gicp"])
def test_systems_on_edge_inputs_and_sizes(dev, oracle_mod, method):
    nn = GC.finite_nn(oracle_mod)
    seen = []
    for s, t in SYSTEM_PAIRS:
        for gate in (0.0, 0.5):
            case = GC._case("x", method, s, t, yaw=0.7, t=(0.08, -0.05, 0.02))
            T = GC.guess(case)
            # the device's normals are the oracle's, bit for bit, on every cloud the sweep uses
            for name in (s, t):
                if len(GC.cloud(name)) and (name == t or method == "gicp"):
                    assert (bits(dev.store.normals(dev.id(name))) == bits(GC.normals(name, oracle_mod))).all(), name
            H, g, s2, cnt = dev.system(method, s, t, T, dev.prm(method, max_corr_dist=gate))
            ref, scale, floor = _ref_system(method, GC.cloud(s), GC.normals(s, oracle_mod), GC.cloud(t), GC.normals(t, oracle_mod), T, nn, gate)
            # (one pair -- a2_n1 -- has one summation order: floor and tolerance are 0 for point-to-plane, whose
            # products the device then has to form as numpy does, bit for bit; it does, and a kernel that re-associates
            # them would have to be given a floor of its own here, from the fp64 formats, not from what it returns)
            tol, err = 10 * floor, _rel((H, g, s2), ref, scale)
            seen.append((floor, tol, err))
            print(f"{method} {s} -> {t} gate {gate}: pairs {cnt} / {ref[3]} of {len(GC.cloud(s))}, floor {floor:.3e} -> tolerance {tol:.3e}; device error {err:.3e}")
            assert tol <= SYSTEM_CAP
            assert cnt == ref[3]
            assert (H == H.T).all() and np.isfinite(H).all() and np.isfinite(g).all()
            assert err <= tol
            if ref[3] == 0:
                assert not H.any() and not g.any() and s2 == 0.0
    a = np.array(seen)
    print(f"{method}: floor {a[:, 0].min():.1e} .. {a[:, 0].max():.1e}, tolerance {a[:, 1].min():.1e} .. {a[:, 1].max():.1e}, device error {a[:, 2].min():.1e} .. {a[:, 2].max():.1e}")


@pytest.mark.parametrize("method", ["p2l", "gicp"])
def test_system_at_full_size(dev, oracle_mod, method):
    """The headline scan size: ~122 k points, ~480 partials a job.  The restatement takes both scans' normals from the
    device here: an O(n^2) neighbour search at 122 k on the CPU is minutes, and tests/test_p2l_gpu.py pins the device's
    normals to the oracle's bit for bit at 19 k.  The 1-NN search is the oracle's grid search."""
    nn = GC.finite_nn(oracle_mod)
    s, t = "full_s", "full_t"
    assert len(GC.cloud(s)) > 100000 and len(GC.cloud(t)) > 100000
    sn, tn = dev.store.normals(dev.id(s)), dev.store.normals(dev.id(t))
    T = (GC._se3(1.5, (0.3, -0.1, 0.0)) @ GC._se3(0.5, (0.1, 0.05, 0.01))).astype(np.float32)
    for gate in (0.0, 0.5):
        H, g, s2, cnt = dev.system(method, s, t, T, dev.prm(method, max_corr_dist=gate))
        ref, scale, floor = _ref_system(method, GC.cloud(s), sn, GC.cloud(t), tn, T, nn, gate)
        tol, err = 10 * floor, _rel((H, g, s2), ref, scale)
        print(f"{method} full size gate {gate}: pairs {cnt} / {ref[3]} of {len(GC.cloud(s))}, floor {floor:.3e} -> tolerance {tol:.3e}; device error {err:.3e}")
        assert tol <= SYSTEM_CAP and cnt == ref[3] and cnt > 50000 and (H == H.T).all() and err <= tol


# ---- 3. whole alignments over the case list ----------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["p2l", "gicp"])
def test_alignments_follow_the_restatement(dev, oracle_mod, method):
    refs = GC.references(oracle_mod)
    seen, n_stable = [], 0
    for case in (c for c in GC.CASES if c["method"] == method):
        r, prm = refs[case["name"]], GC.params(case)
        T, rmse, iters, status = out = dev.run(case)
        assert np.isfinite(T).all() and status[0] in (0, 1, 2) and iters[0] <= prm["max_iters"]
        assert _same(out, dev.run(case)), case["name"]                      # the same bits on a second run
        if status[0] == 2 and iters[0] == 0:
            assert (bits(T[0]) == bits(GC.guess(case))).all()               # degenerate at once: the guess comes back
        if not r["stable"]:
            print(f"{case['name']}: unstable in the restatement, held only to what holds regardless")
            continue
        n_stable += 1
        ref = r["ref"]
        ft, fa = r["floor"]
        ot, oa = P.pose_err(ref["T"], ref["T"].astype(np.float32))
        dt, da = P.pose_err(ref["T"], T[0])
        seen.append((ft, fa, 10 * ft + 2 * ot, 10 * fa + 2 * oa, dt, da))
        print(f"{case['name']}: iters {iters[0]} / {ref['iters']}, status {status[0]} / {ref['status']}, rmse {rmse[0]:.6f} / {ref['rmse']:.6f}; "
              f"floor {ft:.2e} m {fa:.2e} rad, fp32 output {ot:.2e} m {oa:.2e} rad; against the restatement {dt:.2e} m {da:.2e} rad")
        assert 10 * ft <= POSE_CAP and 10 * fa <= POSE_CAP
        assert status[0] == ref["status"], case["name"]
        assert int(iters[0]) == ref["iters"], case["name"]
        assert dt <= 10 * ft + 2 * ot and da <= 10 * fa + 2 * oa, case["name"]
        assert abs(rmse[0] - ref["rmse"]) <= 1e-6 * max(ref["rmse"], 1.0), case["name"]
    a = np.array(seen)
    print(f"{method}: {n_stable} stable cases; floor {a[:, 0].min():.1e} .. {a[:, 0].max():.1e} m, {a[:, 1].min():.1e} .. {a[:, 1].max():.1e} rad; "
          f"tolerance {a[:, 2].min():.1e} .. {a[:, 2].max():.1e} m, {a[:, 3].min():.1e} .. {a[:, 3].max():.1e} rad; "
          f"device {a[:, 4].min():.1e} .. {a[:, 4].max():.1e} m, {a[:, 5].min():.1e} .. {a[:, 5].max():.1e} rad")


@pytest.mark.parametrize("method", ["p2l", "gicp"])
def test_a_mixed_batch(dev, oracle_mod, method):
    """One call whose jobs end at the cap, converged at different passes, degenerate at once and degenerate mid-run: every
    job equals its own single-job call bit for bit, and a job that stopped holds the pose of a run of exactly that many
    updates with the stop test off -- the passes the batch ran for the others did not touch it."""
    refs = GC.references(oracle_mod)
    for names in GC.MIXED[method]:
        cs = [GC.by_name(n) for n in names]
        prm = dev.prm(cs[0])
        init = np.stack([GC.guess(c) for c in cs])
        T, rmse, iters, status = out = dev.batch(method, cs[0]["src"], [c["tgt"] for c in cs], init, prm)
        assert _same(out, dev.batch(method, cs[0]["src"], [c["tgt"] for c in cs], init, prm))
        print(f"{method} {names[0]} ..: status {status.tolist()}, iters {iters.tolist()}")
        assert status.tolist() == [refs[n]["ref"]["status"] for n in names] and iters.tolist() == [refs[n]["ref"]["iters"] for n in names]
        for j, c in enumerate(cs):
            one = dev.run(c)
            assert _same(one, (T[j:j + 1], rmse[j:j + 1], iters[j:j + 1], status[j:j + 1])), names[j]
            if status[j] != 0 and iters[j] > 0:
                p = dict(GC.params(c), max_iters=int(iters[j]), trans_eps=0.0, rot_eps=0.0)
                T0, _, i0, s0 = dev.batch(method, c["src"], [c["tgt"]], init[j:j + 1], dev.prm(method, **p))
                assert i0[0] == iters[j] and s0[0] == 0 and (bits(T0[0]) == bits(T[j])).all(), names[j]
            elif status[j] != 0:
                assert (bits(T[j]) == bits(init[j])).all(), names[j]


# ---- 4. search settings: identical correspondences, so identical bits ---------------------------------------------------------
def _settings(capi):
    c = capi
    return [("default", []), ("exhaustive", [(c.REG_OPT_NN_MODE, c.REG_NN_EXHAUSTIVE)]), ("1 per lane", [(c.REG_OPT_NN_SRC_PER_LANE, 1)]),
            ("4 per lane", [(c.REG_OPT_NN_SRC_PER_LANE, 4)]), ("job group 8", [(c.REG_OPT_NN_JOB_GROUP, 8)]),
            ("job group 16, 4 per lane", [(c.REG_OPT_NN_JOB_GROUP, 16), (c.REG_OPT_NN_SRC_PER_LANE, 4)])]


@pytest.mark.parametrize("method", ["p2l", "gicp"])
def test_search_settings_and_target_order_change_no_bit(capi, oracle_mod, method):
    tg = ["a0", "a1", "a0_odd", "b0", "empty", "a0_dup"]
    # (job 0 is the case mix_near_<method> -- the truth as the guess, the same parameters -- which the restatement converges)
    offs = [np.eye(4), GC._se3(-2.0, (-0.15, 0.10, -0.03), roll_deg=0.4), GC._se3(0.5, (0.25, 0.20, 0.05))]
    first = {}
    for kd in (False, True):
        for label, opts in _settings(capi):
            d = Dev(capi, kd=kd)
            try:
                for o, v in opts:
                    d.reg.set_option(o, v)
                prm = d.prm(method, max_iters=6, max_corr_dist=1.0, trans_eps=2e-3, rot_eps=2e-4)
                for n in (3, 60):
                    tgts = [tg[j % len(tg)] for j in range(n)]
                    init = np.stack([(GC.truth("a2", "a0") @ offs[j % 3]) for j in range(n)]).astype(np.float32)
                    got = d.batch(method, "a2", tgts, init, prm) + tuple(d.system(method, "a2", "a0", init[1], prm)[:2])
                    want = first.setdefault(n, got)
                    assert _same(got, want), (kd, label, n)
                    assert (got[4] == want[4]).all() and (got[5] == want[5]).all(), (kd, label, n)
            finally:
                d.close()
    near = GC.by_name("mix_near_" + method)
    assert GC.params(near) == dict(max_iters=6, max_corr_dist=1.0, trans_eps=float(np.float32(2e-3)), rot_eps=float(np.float32(2e-4)),
                                   plane_eps=float(np.float32(1e-3))) and (GC.guess(near) == GC.truth("a2", "a0").astype(np.float32)).all()
    ref = GC.references(oracle_mod)[near["name"]]["ref"]
    for n in (3, 60):
        assert first[n][3][0] == ref["status"] == 1 and first[n][2][0] == ref["iters"]
    assert {int(s) for s in first[60][3]} == {0, 1, 2}        # (the batch converges, hits the cap and has an empty target)


# ---- 5. batch sizes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["p2l", "gicp"])
def test_batch_sizes(dev, oracle_mod, method):
    tg = ["a0", "a1", "b0", "a0_odd", "empty"]
    near = GC.by_name("mix_near_" + method)                    # job 0: that case, which the restatement converges
    prm = dev.prm(near)
    rng = np.random.default_rng(3)
    init = np.stack([GC.truth("a2", "a0") @ GC._se3(rng.uniform(-2, 2), tuple(rng.uniform(-0.2, 0.2, 3))) for _ in range(300)]).astype(np.float32)
    init[0] = GC.guess(near)
    init[7, 0, 3] += 1000.0                                     # no pair in reach
    ref = GC.references(oracle_mod)[near["name"]]["ref"]
    single = {}
    for n in (1, 47, 48, 49, 300):
        tgts = [tg[j % len(tg)] for j in range(n)]
        T, rmse, iters, status = dev.batch(method, "a2", tgts, init[:n], prm)
        for j in range(n):
            if j not in single:                                 # (every job of every call, the 300 included)
                single[j] = dev.batch(method, "a2", [tgts[j]], init[j:j + 1], prm)
            assert _same(single[j], (T[j:j + 1], rmse[j:j + 1], iters[j:j + 1], status[j:j + 1])), (n, j)
        if n == 300:
            assert status[7] == 2 and iters[7] == 0 and (status[4::5] == 2).all()
        assert status[0] == ref["status"] == 1 and iters[0] == ref["iters"]
    for n in (0, 4097):
        with pytest.raises(dev.capi.GlocError) as e:
            dev.batch(method, "a2", ["a0"] * n, np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)), prm)
        assert e.value.code == GLOC_ERR_INVALID


# ---- 6. one handle, many calls ------------------------------------------------------------------------------------------------
def test_one_handle_across_methods_sizes_and_sources(capi):
    """Point-to-plane, generalized ICP, a RANSAC + ICP batch, point-to-plane again; a small batch after a large one; a
    short source after a long one -- all on ONE registrar, whose workspaces (p2l::Ws, states, partials, corr) are re-used:
    every call equals the same call on a fresh handle bit for bit, and the store's bytes come back after the releases."""
    d = Dev(capi)
    live_fresh = d.store.bytes()[0]
    off = GC.truth("a2", "a0") @ GC._se3(0.8, (0.1, -0.1, 0.02))
    tg = ["a0", "a1", "b0", "empty"]

    def call(h, kind, src, n):
        init = np.stack([off @ GC._se3(0.1 * (j % 5), (0.01 * (j % 7), 0.0, 0.0)) for j in range(n)]).astype(np.float32)
        tgts = [tg[j % len(tg)] for j in range(n)]
        if kind == "reg":
            o = h.reg.batch_ids(h.id(src), [h.id(t) for t in tgts], init_T=init, params=capi.default_reg_params(ransac_iters=64, icp_iters=4))
            return o["T"], o["rmse"], o["inliers"], o["ok"]
        return h.batch(kind, src, tgts, init, h.prm(kind, max_iters=5, max_corr_dist=1.0, trans_eps=5e-3, rot_eps=5e-4))

    seq = [("p2l", "a2", 60), ("gicp", "a2", 60), ("reg", "a2", 20), ("p2l", "a2", 60), ("gicp", "a2", 3), ("p2l", "a2", 2),
           ("p2l", "a2_n65", 5), ("gicp", "a2_n5", 2), ("gicp", "a2", 7), ("p2l", "a2_n257", 49)]
    for k, (kind, src, n) in enumerate(seq):
        got = call(d, kind, src, n)
        fresh = Dev(capi)
        try:
            want = call(fresh, kind, src, n)
        finally:
            fresh.close()
        assert _same(got, want), (k, kind, src, n)
    for sid in d.ids.values():
        d.store.release(sid)
    assert d.store.bytes()[0] == live_fresh
    d.close()
