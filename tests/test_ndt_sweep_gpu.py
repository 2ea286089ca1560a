"""GPU: NDT scan registration (gloc_reg_ndt_*, gloc_scan_store_add_approx_voxel) against the float64 restatement
tests/ndt_ref.py across parameters, poses and line-search branches -- the cells at the min_points / degenerate /
cell-face edges, the derivatives on both sides of the small-angle rule and at every parameter, whole alignments over the
case list of tests/ndt_cases.py (whose coverage of the Newton / More-Thuente branches tests/test_ndt_sweep_cpu.py proves
on the restatement alone), and the source filter's flush rule.

Every tolerance is that of tests/test_ndt_gpu.py; the stability rule (1e-6, two summation orders of the restatement)
decides without a look at the device which cases are held to the restatement's trajectory."""
import ctypes as C

import numpy as np
import pytest

import ndt_cases as NC
import ndt_ref as R

pytestmark = pytest.mark.gpu


def _params(capi, over=None):
    """gloc_ndt_params for `over`, and the dict of the float32 values the device sees (what the restatement runs with)."""
    prm = capi.default_ndt_params(**(over or {}))
    seen = {f: getattr(prm, f) for f, _ in prm._fields_}
    assert seen == NC.ref_params(over)
    return prm, seen


def _bits_equal(a, b):
    return (R.sort_rows_by_bits(a).view(np.uint32) == R.sort_rows_by_bits(b).view(np.uint32)).all()


@pytest.fixture(scope="module")
def env(capi):
    store = capi.ScanStore()
    reg = capi.Registrar(store=store)
    yield dict(store=store, reg=reg)
    reg.close()
    store.close()


# ---- 1. cells -------------------------------------------------------------------------------------------------------
def _tie_keys(pts, res, min_points):
    """Packed keys of the cells whose validity the restatement itself decides on rounding noise: an eigenvalue of the
    covariance within the rounding error of its fp64 sums (n terms of at most res^2 each: 8 n eps res^2) of zero, where
    `l0 < 0` drops the cell and `l0 >= 0` inflates it.  Rays at an azimuth of a multiple of 45 deg make such cells
    (y = 0, x = 0 or x = -+y exactly in every point): far cells that one such ray alone fills.  Seen on scan 1 of world
    "b" at 0.5 m, cell (14, -15, -1): 7 points with x = -y, l0 = 5.5e-18 under LAPACK (kept, inflated), dropped by the
    device's Jacobi; the scans of tests/test_ndt_gpu.py (n_az = 500) have no cell on such a tie."""
    p = np.ascontiguousarray(pts, np.float32)
    p = p[np.isfinite(p).all(1)]
    k = np.floor(p * (np.float32(1.0) / np.float32(res))).astype(np.int64)
    uniq, inv, n = np.unique(k, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    ties = []
    for c in np.nonzero(n >= min_points)[0]:
        rel = p[inv == c].astype(np.float64) - uniq[c] * float(res)
        lam = np.linalg.eigvalsh(np.cov(rel.T, bias=True))
        if np.abs(lam).min() <= 8 * n[c] * np.finfo(np.float64).eps * float(res) ** 2:
            ties.append(uniq[c])
    return R.pack_keys(np.array(ties, np.int64).reshape(-1, 3))


def _check_cells(env, capi, pts, over=None, min_cells=1, ties=False):
    """Upload pts, compare gloc_reg_ndt_cells with ndt_ref.build_cells as test_ndt_gpu's test_cells_match_the_restatement
    does; returns the restatement's cells.  ties: a cell of _tie_keys (ray-cast scans only; the hand-built clouds are
    exact by construction and get no such allowance) may be valid on one side and dropped on the other, and its inverse
    covariance is not compared; where both sides keep it, its key, count and mean are held like any other cell's."""
    st, reg = env["store"], env["reg"]
    prm, seen = _params(capi, over)
    sid = st.add(pts)
    try:
        dev = reg.ndt_cells(sid, params=prm)
    finally:
        st.release(sid)
    ref = R.build_cells(pts, seen["resolution"], seen["min_points_per_cell"], seen["min_covar_eigvalue_mult"])
    full = ref
    if ties:
        tk = _tie_keys(pts, seen["resolution"], seen["min_points_per_cell"])
        dp, rp = R.pack_keys(dev["key3"]), ref["packed"]
        both = np.intersect1d(np.intersect1d(dp, rp), tk)
        print("\ncells on an eigenvalue tie: %d of %d, kept by both sides: %d, by the restatement only: %d, by the device only: %d"
              % (len(tk), len(rp), len(both), np.isin(rp, tk).sum() - len(both), np.isin(dp, tk).sum() - len(both)))
        assert len(tk) <= 0.06 * len(rp)                    # (what these scans hold: at most 34 of 678; an exception)
        di, ri = np.searchsorted(dp, both), np.searchsorted(rp, both)
        assert (dev["count"][di] == ref["count"][ri]).all()
        if len(both):
            assert np.abs(dev["mean"][di] - ref["mean"][ri]).max() <= 1e-6 * np.abs(ref["mean"]).max()
        keep_d, keep_r = ~np.isin(dp, tk), ~np.isin(rp, tk)
        dev = {k: v[keep_d] for k, v in dev.items()}
        ref = {k: v[keep_r] for k, v in ref.items()}
    assert len(ref["count"]) >= min_cells
    assert len(dev["count"]) == len(ref["count"])
    assert (dev["key3"] == ref["key3"]).all() and (dev["count"] == ref["count"]).all()
    if len(ref["count"]):
        assert np.abs(dev["mean"] - ref["mean"]).max() <= 1e-6 * np.abs(ref["mean"]).max()
        nrm = np.linalg.norm(ref["icov"].reshape(-1, 9), axis=1)
        assert (np.abs(dev["icov"] - ref["icov"]).reshape(-1, 9).max(1) <= 1e-4 * nrm).all()
    return full


def _blob(rng, cell, n, res=0.5, spread=0.3):
    """n points well inside cell `cell` (integer index) of a grid of size res.  Three points span a plane, so their
    smallest eigenvalue is rounding noise around zero: they are put at the cell's mid height exactly, which makes that
    eigenvalue an exact zero on both sides (inflated, valid)."""
    p = (np.asarray(cell, np.float64) + 0.5 + rng.uniform(-spread, spread, (n, 3))) * res
    if n <= 3:
        p[:, 2] = (cell[2] + 0.5) * res
    return p.astype(np.float32)


@pytest.mark.parametrize("min_points", [3, 6, 10])
def test_cells_at_the_min_points_boundary(capi, env, min_points):
    rng = np.random.default_rng(min_points)
    cells = [(-7, 3, 1), (0, 0, 0), (5, -2, -1), (40, 40, 2)]
    counts = [min_points - 1, min_points, min_points + 1, 2 * min_points]
    pts = np.concatenate([_blob(rng, c, n) for c, n in zip(cells, counts)])
    pts = pts[rng.permutation(len(pts))]
    ref = _check_cells(env, capi, pts, dict(min_points_per_cell=min_points), min_cells=3)
    keys = {tuple(k): int(n) for k, n in zip(ref["key3"], ref["count"])}
    assert cells[0] not in keys
    assert [keys[c] for c in cells[1:]] == counts[1:]


def _degenerate_cloud():
    """One cell each (0.5 m grid, coordinates exact in binary so that a zero variance is an exact zero on both sides):
    8 identical points; 8 collinear along x; a 3 x 3 coplanar grid in xy; 12 points spread over 1e-4 of the cell size;
    a plain blob."""
    rng = np.random.default_rng(11)
    same = np.tile(np.array([[0.25, 0.25, 0.25]]), (8, 1))
    line = np.array([[2.0 + 0.0625 * (i + 0.5), 0.25, 0.25] for i in range(8)])
    gx, gy = np.meshgrid([0.125, 0.25, 0.375], [0.125, 0.25, 0.375])
    plane = np.stack([4.0 + gx.ravel(), -3.0 + gy.ravel(), np.full(9, -0.25)], 1)
    tiny = np.array([6.25, 1.25, -1.25]) + rng.uniform(-0.5, 0.5, (12, 3)) * (1e-4 * 0.5)
    return np.concatenate([same, line, plane, tiny, _blob(rng, (20, 0, 0), 15)]).astype(np.float32)


@pytest.mark.parametrize("eig_mult", [0.001, 0.01, 0.1])
def test_degenerate_cells_are_dropped_or_inflated_as_the_restatement_does(capi, env, eig_mult):
    pts = _degenerate_cloud()
    ref = _check_cells(env, capi, pts, dict(min_covar_eigvalue_mult=eig_mult), min_cells=4)
    keys = {tuple(k) for k in ref["key3"]}
    assert (0, 0, 0) not in keys                       # identical points: l2 = 0, dropped
    assert {(4, 0, 0), (8, -6, -1), (12, 2, -3), (20, 0, 0)} <= keys


def test_cell_faces_and_negative_coordinates_floor(capi, env):
    up, down = np.float32(np.inf), np.float32(-np.inf)
    f = np.float32
    special = [f(-0.5), f(-0.0), f(0.0), np.nextafter(f(0.5), down), f(0.5), np.nextafter(f(-0.5), down),
               np.nextafter(f(-0.5), up), np.nextafter(f(0.0), down), f(-1.0), f(-0.25), f(-37.5), np.nextafter(f(-37.5), down)]
    rows = []
    for axis in range(3):
        for i, v in enumerate(special):
            for j in range(7):                          # 7 points per special value: one cell each
                p = np.roll(np.array([0.0, 3.1 + 1.5 * i + 0.05 * j, 100.0 * (axis + 1) + 0.13 + 0.04 * ((j * j) % 5)], np.float32), axis)
                cell = np.floor(v * (f(1.0) / f(0.5)))        # the first point sits at v itself, the other six inside v's cell
                p[axis] = v if j == 0 else f((cell + 0.2 + 0.1 * j) * 0.5)
                rows.append(p)
    pts = np.array(rows, np.float32)
    ref = _check_cells(env, capi, pts, min_cells=3 * len(special))
    # the restatement itself floors: -0.5 is cell -1, -0.5 - ulp is cell -2, -0.0 is cell 0, 0.5 - ulp is cell 0
    for axis in range(3):
        got = sorted(set(int(k[axis]) for k in ref["key3"] if 6 <= k[(axis + 1) % 3] < 50))
        assert {-76, -75, -2, -1, 0, 1} <= set(got), got


@pytest.mark.parametrize("resolution", [0.25, 1.0, 2.0])
def test_cells_at_other_resolutions_and_far_from_the_origin(capi, env, resolution):
    scan = NC.scan("a", 0)
    _check_cells(env, capi, scan, dict(resolution=resolution), min_cells=100, ties=True)
    far = (scan + np.array([300.0, -295.0, 5.0], np.float32)).astype(np.float32)
    assert np.abs(far).max() > 300
    _check_cells(env, capi, far, dict(resolution=resolution), min_cells=100, ties=True)


def test_cells_ignore_nan_and_inf_rows(capi, env):
    scan = NC.scan("b", 1).copy()
    clean = _check_cells(env, capi, scan, min_cells=100, ties=True)
    bad = scan.copy()
    bad[::5, 2] = np.nan
    bad[::13, 0] = np.inf
    bad[7::29, 1] = -np.inf
    ref = _check_cells(env, capi, bad, min_cells=100, ties=True)
    assert ref["count"].sum() < clean["count"].sum()
    ok = np.isfinite(bad).all(1)
    again = _check_cells(env, capi, np.ascontiguousarray(bad[ok]), min_cells=100, ties=True)
    assert (again["packed"] == ref["packed"]).all() and (again["count"] == ref["count"]).all()


def test_cells_capacity_and_the_count_query(capi, env):
    st, reg = env["store"], env["reg"]
    L = capi.lib()
    prm, _ = _params(capi)
    pts = NC.scan("c", 0)
    sid = st.add(pts)
    k = len(R.build_cells(pts, 0.5)["count"])
    m = C.c_size_t(0)
    assert L.gloc_reg_ndt_cells(reg._h, sid, C.byref(prm), 0, None, None, None, None, C.byref(m)) == 0   # NULL arrays: ask
    assert m.value == k > 100
    key, cnt = np.zeros((k, 3), np.int32), np.zeros(k, np.uint32)
    mean, icov = np.zeros((k, 3)), np.zeros((k, 3, 3))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    m = C.c_size_t(0)
    rc = L.gloc_reg_ndt_cells(reg._h, sid, C.byref(prm), k - 1, ptr(key), ptr(cnt), ptr(mean), ptr(icov), C.byref(m))
    assert rc == 1 and m.value == k                        # GLOC_ERR_INVALID, and how many there are
    assert (key[k - 1] == 0).all() and cnt[k - 1] == 0     # nothing written behind the capacity
    m = C.c_size_t(0)
    assert L.gloc_reg_ndt_cells(reg._h, sid, C.byref(prm), k + 5, ptr(key), None, None, None, C.byref(m)) == 0
    assert m.value == k and (key == R.build_cells(pts, 0.5)["key3"]).all()
    st.release(sid)


# ---- 2. derivatives -------------------------------------------------------------------------------------------------
def _small_angle_threshold():
    """The threshold of ndt_ref._cs_small, found by bisection on the function itself (no second copy of the number)."""
    lo, hi = 1e-12, 1.0
    assert R._cs_small(lo) == (1.0, 0.0) and R._cs_small(hi) != (1.0, 0.0)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if R._cs_small(mid) == (1.0, 0.0):
            lo = mid
        else:
            hi = mid
    return hi


def _check_derivatives(reg, src_id, tgt_id, x, cells, p, prm, seen):
    sd, gd, Hd = reg.ndt_derivatives(src_id, tgt_id, p, params=prm)
    sr, gr, Hr = R.derivatives(x, cells, np.array(p, np.float64), seen["resolution"], seen["outlier_ratio"])
    assert abs(sd - sr) <= 1e-5 * abs(sr), (p, sd, sr)
    if np.linalg.norm(gr) == 0:
        assert sr == 0 and sd == 0 and (gd == 0).all() and (Hd == 0).all(), p
    else:
        assert np.abs(gd - gr).max() <= 1e-4 * np.linalg.norm(gr), p
        assert np.abs(Hd - Hr).max() <= 1e-4 * np.linalg.norm(Hr), p
    return sr


@pytest.fixture(scope="module")
def pair(env):
    st = env["store"]
    src, tgt = NC.scan("a", 2), NC.scan("a", 0)
    ids = dict(src=st.add(src), tgt=st.add(tgt), src_pts=src, tgt_pts=tgt)
    yield ids
    st.release(ids["src"])
    st.release(ids["tgt"])


def test_derivatives_around_the_small_angle_rule_and_at_large_angles(capi, env, pair):
    reg = env["reg"]
    prm, seen = _params(capi)
    x = R.approx_voxel(pair["src_pts"], seen["source_leaf"])
    cells = R.build_cells(pair["tgt_pts"], seen["resolution"])
    thr = _small_angle_threshold()
    mags = [1e-6, 9e-6, 1.1e-5, 0.9 * thr, np.nextafter(thr, 0), thr, 1.1 * thr, 1e-3, 0.3, 1.5]
    angles = [s * m for m in mags for s in (1.0, -1.0)] + [3.0]
    n_pos = 0
    for i, a in enumerate(angles):
        t = [2.0 * np.sin(0.7 * i), 2.0 * np.cos(1.3 * i), 0.3 * np.sin(2.1 * i)]       # translations up to 2 m
        for which in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]):
            for tt in (t, [0.1, -0.05, 0.0]):
                p = tt + [a * w for w in which]
                n_pos += _check_derivatives(reg, pair["src"], pair["tgt"], x, cells, p, prm, seen) > 0
    assert n_pos > len(angles) * 4                       # most poses score: the relative bounds were not void
    # mixed: one angle under the rule, one over, one large
    for p in ([0.1, 0.0, 0.0, 0.5 * thr, 2.0 * thr, 1.2], [0.0, 0.1, 0.0, -2.0 * thr, 0.9 * thr, -0.02]):
        assert _check_derivatives(reg, pair["src"], pair["tgt"], x, cells, p, prm, seen) > 0
    # out of reach of every cell: score 0, zero gradient and Hessian, exactly
    assert _check_derivatives(reg, pair["src"], pair["tgt"], x, cells, [1000.0, 0, 0, 0.01, 0, 0.02], prm, seen) == 0


POSES = ([0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.15, -0.02, 0.01, 0.003, -0.002, 0.03], [-0.4, 0.3, 0.05, -0.02, 0.01, -0.08],
         [1.2, -1.6, 0.1, 5e-5, 0.3, 2e-4])


@pytest.mark.parametrize("over", [dict(resolution=0.25), dict(resolution=1.0), dict(outlier_ratio=0.1), dict(outlier_ratio=0.55),
                                  dict(outlier_ratio=0.9), dict(source_leaf=0.1), dict(source_leaf=0.4),
                                  dict(resolution=1.0, outlier_ratio=0.9, source_leaf=0.4)],
                         ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_derivatives_at_other_parameters(capi, env, pair, over):
    prm, seen = _params(capi, over)
    x = R.approx_voxel(pair["src_pts"], seen["source_leaf"])
    cells = R.build_cells(pair["tgt_pts"], seen["resolution"])
    for p in POSES:
        assert _check_derivatives(env["reg"], pair["src"], pair["tgt"], x, cells, p, prm, seen) > 0


def test_derivatives_without_a_source_filter_take_the_finite_points(capi, env, pair):
    st, reg = env["store"], env["reg"]
    src = pair["src_pts"][:6000].copy()
    src[::7, 1] = np.nan
    src[3::11, 0] = np.inf
    sid = st.add(src)
    cells = R.build_cells(pair["tgt_pts"], 0.5)
    for leaf in (0.0, -1.0):
        prm, seen = _params(capi, dict(source_leaf=leaf))
        x = R.approx_voxel(src, leaf)
        assert len(x) == np.isfinite(src).all(1).sum() < len(src)
        for p in POSES:
            assert _check_derivatives(reg, sid, pair["tgt"], x, cells, p, prm, seen) > 0
    st.release(sid)


# ---- 3. whole alignments --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scans(env):
    """(world, k) -> scan id, uploaded on first use."""
    st, ids = env["store"], {}

    def get(world, k):
        if (world, k) not in ids:
            ids[(world, k)] = st.add(NC.scan(world, k))
        return ids[(world, k)]
    yield get
    for i in ids.values():
        st.release(i)


def _same(a, b):
    return ((a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[1].view(np.uint64) == b[1].view(np.uint64)).all()
            and (a[2] == b[2]).all() and (a[3] == b[3]).all())


@pytest.mark.parametrize("name", [c["name"] for c in NC.CASES])
def test_alignment_follows_the_restatement(capi, env, scans, name):
    case = next(c for c in NC.CASES if c["name"] == name)
    verdict = NC.references()[name]
    r = verdict["ref"]
    prm, seen = _params(capi, case["params"])
    s, t, g = scans(case["world"], case["src"]), scans(case["world"], case["tgt"]), NC.guess(case)
    out = env["reg"].ndt_batch(s, [t], init_T=g[None], params=prm)
    T, prob, iters, conv = out
    dt, da = NC.pose_gap(r["T"], T[0])
    print("\n%s %s: device iters %d conv %d prob %.9g | restatement iters %d conv %d prob %.9g | gap %.3g m %.3g rad"
          % (name, "stable" if verdict["stable"] else "UNSTABLE", iters[0], conv[0], prob[0], r["iters"], r["converged"], r["prob"], dt, da))
    if verdict["stable"]:
        assert dt < 1e-3 and da < 1e-3
        assert abs(int(iters[0]) - r["iters"]) <= 1
        assert abs(prob[0] - r["prob"]) <= 1e-3 * abs(r["prob"])
        assert bool(conv[0]) == r["converged"]
        if "end_iteration_cap" in verdict["events"]:
            assert int(iters[0]) == r["iters"] == seen["max_iters"] + 2
    else:
        assert np.isfinite(T[0]).all() and int(iters[0]) <= seen["max_iters"] + 2 and prob[0] >= 0
    assert _same(out, env["reg"].ndt_batch(s, [t], init_T=g[None], params=prm))      # bit-identical on a second run


def test_batches_of_mixed_targets_and_guesses_equal_single_calls(capi, env, scans):
    """Per source, its cases (grouped by parameter set: a call takes one) go through one call of 24 candidates --
    several waves of states -- filled up with further guesses against both targets; every candidate equals its single
    call bit for bit (for the fill-ups this is checked on each source's first group)."""
    from gloc3d_amd import synth
    reg = env["reg"]
    groups = {}
    for c in NC.CASES:
        groups.setdefault((c["world"], c["src"]), {}).setdefault(tuple(sorted(c["params"].items())), []).append(c)
    assert len(groups) >= 6
    for (world, src), by_prm in groups.items():
        s = scans(world, src)
        for gi, (pk, cases) in enumerate(by_prm.items()):
            prm, _ = _params(capi, dict(pk))
            tg = [scans(world, c["tgt"]) for c in cases]
            init = [NC.guess(c) for c in cases]
            n_own = len(cases)
            for i in range(24 - n_own):
                k = 0 if world[0] == "t" else i % 2
                tg.append(scans(world, k))
                init.append((NC.truth(world, src, k) @ synth.se3(0.4 * (i % 7) - 1.0, (0.03 * (i % 5), -0.02 * (i % 3), 0.0))).astype(np.float32))
            init = np.stack(init)
            assert len(tg) == 24 > 20
            T, prob, iters, conv = reg.ndt_batch(s, tg, init_T=init, params=prm)
            for c in range(24 if gi == 0 else n_own):
                one = reg.ndt_batch(s, [tg[c]], init_T=init[c:c + 1], params=prm)
                assert _same(one, (T[c:c + 1], prob[c:c + 1], iters[c:c + 1], conv[c:c + 1])), (world, src, pk, c)


# ---- 4. the source filter and what goes with it -----------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [0.05, 0.5, 2.0])
def test_filter_at_other_leaf_sizes_and_the_flush_rule(capi, env, leaf):
    st = env["store"]
    rng = np.random.default_rng(int(leaf * 100))
    # two cells that share hash slot 0 ((0,0,0) and (512,0,0): 7171 * 512 = 0 mod 512), alternating in runs of 1, 2, 3 ...:
    # every change of cell flushes the slot, so each run is an output point of its own
    runs = []
    for i in range(40):
        base = np.array([0.0 if i % 2 == 0 else 512.0 * leaf, 0.0, 0.0])
        runs.append(base + rng.uniform(0.1, 0.9, (1 + i % 4, 3)) * leaf)
    alternating = np.concatenate(runs).astype(np.float32)
    assert len(R.approx_voxel(alternating, leaf)) == 40
    # 600 distinct cells (512 i, 0, 0), all of slot 0, visited three times over in turn: every point flushes the slot
    one_slot = np.array([[(512.0 * i + 0.5) * leaf, (0.2 + 0.2 * r) * leaf, 0.5 * leaf] for r in range(3) for i in range(600)], np.float32)
    k1, h1, ok1 = R.voxel_slots(one_slot, leaf)
    assert ok1.all() and (h1 == 0).all() and len(np.unique(k1, axis=0)) == 600 > R.HIST
    assert len(R.approx_voxel(one_slot, leaf)) == len(R.approx_voxel_sequential(one_slot, leaf)) == 1800
    wide = rng.uniform(-60, 60, (20000, 3)) * (leaf / 0.2)                         # far more than 512 distinct cells
    wide = wide.astype(np.float32)
    scan = NC.scan("c", 3)
    holes = scan[:5000].copy()
    holes[::5, 2] = np.nan
    holes[::13, 0] = np.inf
    negative = (scan[:5000] - np.float32(37.3)).astype(np.float32)
    for pts in (alternating, one_slot, wide, scan, holes, negative, np.array([[-1.25, 3.5, 0.75]], np.float32)):
        sid = st.add(pts)
        fid = st.add_approx_voxel(sid, leaf)
        dev = st.download(fid)
        st.release(fid)
        st.release(sid)
        ref = R.approx_voxel(pts, leaf)
        assert len(dev) == len(ref) >= 1
        assert _bits_equal(dev, ref)
    k, _, _ = R.voxel_slots(wide, leaf)
    assert len(R.approx_voxel(wide, leaf)) >= len(np.unique(k, axis=0)) > 512


def test_no_filter_equals_the_alignment_of_the_cleaned_cloud(capi, env, scans):
    st, reg = env["store"], env["reg"]
    src = NC.scan("b", 2)[:7000].copy()
    src[::9, 0] = np.nan
    src[4::17, 2] = -np.inf
    clean = np.ascontiguousarray(src[np.isfinite(src).all(1)])
    a, b, t = st.add(src), st.add(clean), scans("b", 0)
    g = NC.guess(dict(world="b", src=2, tgt=0, off=(1.0, (0.1, -0.05, 0.0), 0.0, 0.0)))
    for leaf in (0.0, -0.2):
        prm, seen = _params(capi, dict(source_leaf=leaf))
        one, two = reg.ndt_batch(a, [t], init_T=g[None], params=prm), reg.ndt_batch(b, [t], init_T=g[None], params=prm)
        assert _same(one, two) and one[2][0] >= 1 and one[1][0] > 0
        fid = st.add_approx_voxel(a, leaf)
        assert (st.download(fid).view(np.uint32) == clean.view(np.uint32)).all()       # the finite points, in order
        st.release(fid)
    st.release(a)
    st.release(b)


def test_another_stream_gives_the_same_bits(capi, env, scans):
    """Real alignments (every candidate iterates and scores, asserted) of cases a_31 and a_32 and of further guesses
    against both targets, on the default stream and on another one."""
    import torch
    from gloc3d_amd import synth
    reg = env["reg"]
    stream = torch.cuda.Stream()
    for name in ("a_31", "a_32"):
        c = next(c for c in NC.CASES if c["name"] == name)
        assert NC.references()[name]["stable"] and NC.references()[name]["ref"]["iters"] >= 2
        s, tg, init = scans("a", c["src"]), [scans("a", c["tgt"])], [NC.guess(c)]
        for i in range(7):
            tg.append(scans("a", i % 2))
            init.append((NC.truth("a", c["src"], i % 2) @ synth.se3(0.5 * i - 1.5, (0.04 * i, 0.1 - 0.03 * i, 0.0))).astype(np.float32))
        init = np.stack(init)
        prm, _ = _params(capi, c["params"])
        p6 = [0.1, 0.0, 0.0, 0.0, 0.01, 0.02]
        ref = reg.ndt_batch(s, tg, init_T=init, params=prm)
        d0 = reg.ndt_derivatives(s, tg[0], p6, params=prm)
        assert (ref[2] >= 1).all() and (ref[1] > 0).all() and np.isfinite(ref[0]).all() and d0[0] > 0
        if name == "a_31":                                           # (trans_eps 0.2 ends all of a_32's after two steps)
            assert len({int(i) for i in ref[2]}) > 1                 # candidates that stop in different rounds
        reg.set_stream(stream.cuda_stream)
        try:
            other = reg.ndt_batch(s, tg, init_T=init, params=prm)
            d = reg.ndt_derivatives(s, tg[0], p6, params=prm)
        finally:
            reg.set_stream(0)
        assert _same(ref, other)
        assert d[0] == d0[0] and (d[1] == d0[1]).all() and (d[2] == d0[2]).all()


def test_ndt_calls_refuse_a_handle_with_a_batch_in_flight(capi, env, scans):
    reg = env["reg"]
    s, t = scans("a", 2), scans("a", 0)
    ref = reg.ndt_batch(s, [t])
    reg.batch_multi_begin([s], np.array([[t]], np.uint32), params=capi.default_reg_params(ransac_iters=50, icp_iters=2))
    try:
        for call in (lambda: reg.ndt_batch(s, [t]), lambda: reg.ndt_derivatives(s, t, np.zeros(6)), lambda: reg.ndt_cells(t)):
            with pytest.raises(capi.GlocError) as e:
                call()
            assert e.value.code == 5                                                    # GLOC_ERR_STATE
    finally:
        reg.batch_multi_end()
    assert _same(ref, reg.ndt_batch(s, [t]))
