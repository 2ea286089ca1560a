"""GPU: the point-to-point evaluation of registered pairs (gloc_reg_evaluate_pairs; eval_kernels.hpp) against its float64
restatement tests/eval_ref.py on the rows of tests/eval_cases.py, whose branches tests/test_eval_cases_cpu.py proves.

  (a), (b)   every output equals the restatement exactly: all terms and partial sums are exactly representable, so no
             summation order can matter (+0 and -0 compare equal: a sum of nothing but zero terms has no other bits);
  (c) - (e)  count and fitness exactly; every sum within eval_ref.bound -- 2 (count + 4) 2^-53 A_k, derived there from the
             number formats, nothing measured; rmse within one fp32 ulp; info exactly symmetric;
  a second opinion from an existing kernel: generalized ICP at plane_eps = 1 has S = 2I, M = I / 2, so 2 x its H, g and sum
             are the same mathematical sums and its count the same count -- the same bound, an exact count;
  (f)        rows of a list equal their single-row calls bit for bit, in any order, at two positions, with and without
             target indices; the absent and the empty target give the zero row;
  the wrapper's symmetric form, the loop detector's evaluate, and the handle after refusals."""
import numpy as np
import pytest

import eval_cases as EC
import eval_ref as E

pytestmark = pytest.mark.gpu

FIELDS = ("fitness", "rmse", "count", "info", "g")


class Dev:
    """A scan store and a registrar with the clouds of eval_cases uploaded by name."""

    def __init__(self, capi):
        self.capi = capi
        self.store = capi.ScanStore()
        self.reg = capi.Registrar(store=self.store)
        self.ids = {}

    def id(self, name):
        if name is None:
            return None
        if name not in self.ids:
            self.ids[name] = self.store.add(EC.cloud(name))
        return self.ids[name]

    def evaluate(self, rows, reg=None, **kw):
        """One call on rows that share a gate."""
        gates = {r["gate"] for r in rows}
        assert len(gates) == 1
        T = np.stack([np.eye(4, dtype=np.float32) if r["T"] is None else r["T"] for r in rows])
        return (reg or self.reg).evaluate_pairs([self.id(r["src"]) for r in rows], [self.id(r["tgt"]) for r in rows], T=T,
                                                params=self.capi.default_eval_params(max_corr_dist=gates.pop()), **kw)

    def close(self):
        self.reg.close()
        self.store.close()


@pytest.fixture(scope="module")
def dev(capi):
    d = Dev(capi)
    yield d
    d.close()


def bits(a):
    """The bit patterns of a float32 or float64 array."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _row(out, c):
    return {f: out[f][c] for f in FIELDS}


def _same(a, b):
    """Two rows (or stacks of rows), bit for bit."""
    return all((bits(np.asarray(a[f])) == bits(np.asarray(b[f]))).all() if np.asarray(a[f]).dtype.kind == "f" else (a[f] == b[f]).all() for f in FIELDS)


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ---- (a), (b): exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["a", "b", "b0"])
def test_lattice_rows_equal_the_restatement_exactly(dev, oracle_mod, group):
    rows = EC.rows(group)
    assert group != "a" or [len(EC.cloud(r["src"])) for r in rows] == [1, 5, 63, 64, 65, 255, 256, 257, 513]
    out = dev.evaluate(rows)
    for c, r in enumerate(rows):
        ref = EC.reference(r, oracle_mod)
        print(f"({group}) {r['src']}: count {out['count'][c]} / {ref['count']}, fitness {out['fitness'][c]}, rmse {out['rmse'][c]}")
        assert out["count"][c] == ref["count"] and out["fitness"][c] == ref["fitness"] and out["rmse"][c] == ref["rmse"]
        assert np.array_equal(out["info"][c], ref["info"]) and np.array_equal(out["g"][c], ref["g"])
        if group == "b0":
            assert out["count"][c] == 0 and not out["info"][c].any() and not out["g"][c].any()


# ---- (c) - (e): within the bound ------------------------------------------------------------------------------------------------
def _check_against(ref, info, g, count, what):
    tol = E.bound(ref)
    got = np.concatenate([[info[r, c] for r, c in E.TRI], g])
    err = np.abs(got - ref["S"][:27])
    print(f"{what}: {count} / {ref['count']} pairs; worst error / bound {np.max(err / np.maximum(tol[:27], 1e-300)):.4f}")
    assert int(count) == ref["count"]
    assert (err <= tol[:27]).all(), (err / np.maximum(tol[:27], 1e-300)).tolist()


@pytest.mark.parametrize("group", ["c", "d", "e"])
def test_scene_rows_follow_the_restatement(dev, oracle_mod, group):
    for gate, rows in EC.by_gate(EC.rows(group)).items():
        out = dev.evaluate(rows)
        for c, r in enumerate(rows):
            ref = EC.reference(r, oracle_mod)
            _check_against(ref, out["info"][c], out["g"][c], out["count"][c], f"({group}) {r['src']} -> {r['tgt']} gate {gate:.1f}")
            assert out["fitness"][c] == ref["fitness"] and bits(out["fitness"][c]) == bits(ref["fitness"])
            print(f"    rmse {out['rmse'][c]:.7f} / {ref['rmse']:.7f}")
            assert abs(float(out["rmse"][c]) - float(ref["rmse"])) <= _ulp32(ref["rmse"])
            assert (out["info"][c] == out["info"][c].T).all()
            assert ref["count"] > 0 and out["info"][c][3, 3] == ref["count"]


def test_generalized_icp_at_plane_eps_one_gives_the_same_sums(dev, oracle_mod, capi):
    """S = 2I and M = I / 2 for every pair: 2 H, 2 g and 2 sum of gloc_reg_gicp_system are info, g and the squared
    residual, formed by another kernel."""
    for r in EC.rows("c"):
        ref = EC.reference(r, oracle_mod)
        prm = capi.default_gicp_params(plane_eps=1.0, max_corr_dist=r["gate"])
        H, g, s, cnt = dev.reg.gicp_system(dev.id(r["src"]), dev.id(r["tgt"]), r["T"], prm)
        _check_against(ref, 2.0 * H, 2.0 * g, cnt, f"gicp {r['src']} gate {r['gate']:.1f}")
        tol = E.bound(ref)[27]
        print(f"    sum {2.0 * s:.12g} / {ref['sum']:.12g}; error / bound {abs(2.0 * s - ref['sum']) / tol:.4f}")
        assert abs(2.0 * s - ref["sum"]) <= tol


# ---- (f): the list ----------------------------------------------------------------------------------------------------------------
_SINGLES = {}


def _singles(dev):
    """Every row of the mixed list as a call of its own: computed once, never changed."""
    if "rows" not in _SINGLES:
        outs = [dev.evaluate([r]) for r in EC.MIXED]
        got = {f: np.concatenate([o[f] for o in outs]) for f in FIELDS}
        for v in got.values():
            v.setflags(write=False)
        _SINGLES["rows"] = got
    return _SINGLES["rows"]


def _take(out, idx):
    return {f: out[f][np.asarray(idx, np.int64)] for f in FIELDS}


def test_rows_of_a_list_equal_their_single_row_calls(dev, oracle_mod):
    want = _singles(dev)
    got = dev.evaluate(EC.MIXED)
    print(f"(f) counts {got['count'].tolist()}, fitness {got['fitness'].tolist()}")
    assert _same(want, got), [c for c in range(len(EC.MIXED)) if not _same(_row(want, c), _row(got, c))]
    assert _same(got, dev.evaluate(EC.MIXED))                                  # the same bits on a second run
    a, b = EC.TWICE
    assert _same(_row(got, a), _row(got, b))                                   # one row at two positions
    for c, r in enumerate(EC.MIXED):
        ref = EC.reference(r, oracle_mod)
        assert got["count"][c] == ref["count"] and got["fitness"][c] == ref["fitness"]
        if r["tgt"] in (None, "empty"):                                        # the zero row
            assert got["count"][c] == 0 and got["fitness"][c] == 0 and got["rmse"][c] == 0
            assert not got["info"][c].any() and not got["g"][c].any()
    n = len(EC.MIXED)
    for what, idx in {"reversed": list(range(n))[::-1], "rotated": list(range(3, n)) + [0, 1, 2], "twice": [c for c in range(n) for _ in (0, 1)]}.items():
        assert _same(_take(want, idx), dev.evaluate([EC.MIXED[c] for c in idx])), what


def test_target_indices_change_no_bit(capi, dev):
    """In a store of its own every target of the list gets a target index (its points re-sorted into kd order); the
    sources stay as uploaded, so the self pair, whose target is its source, is left out.  The same bits as without."""
    d = Dev(capi)
    try:
        keep = [c for c, r in enumerate(EC.MIXED) if r["tgt"] is not None and r["src"] != r["tgt"]]
        rows = [EC.MIXED[c] for c in keep]
        assert len(keep) >= 6 and not {r["src"] for r in rows} & {r["tgt"] for r in rows}
        for t in sorted({r["tgt"] for r in rows if len(EC.cloud(r["tgt"]))}):
            d.store.build_target_index(d.id(t))
        assert _same(_take(_singles(dev), keep), d.evaluate(rows))
    finally:
        d.close()


def test_a_row_without_a_target_alone(dev):
    out = dev.evaluate([EC.MIXED[3]])
    assert EC.MIXED[3]["tgt"] is None
    assert out["count"][0] == 0 and out["fitness"][0] == 0 and out["rmse"][0] == 0 and not out["info"].any() and not out["g"].any()


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------
def test_symmetric_is_the_doubled_list(dev):
    rows = EC.rows("c")[3:6] + [EC.MIXED[5]]
    assert len({r["gate"] for r in rows}) == 1
    sym = dev.evaluate(rows, symmetric=True)
    T = np.stack([r["T"] for r in rows])
    Tinv = np.linalg.inv(T.astype(np.float64)).astype(np.float32)
    back = [dict(r, src=r["tgt"], tgt=r["src"], T=Tinv[c]) for c, r in enumerate(rows)]
    both = dev.evaluate(rows + back)
    n = len(rows)
    assert _same(_take(both, range(n)), sym)
    for f in ("fitness", "rmse", "count"):
        assert (bits(both[f][n:]) == bits(sym[f + "_rev"])).all()
    assert (sym["overlap"] == np.minimum(sym["fitness"], sym["fitness_rev"])).all() and (sym["overlap"] > 0.5).all()
    print(f"symmetric: fitness {sym['fitness'].tolist()}, reversed {sym['fitness_rev'].tolist()}")
    with pytest.raises(ValueError):
        dev.reg.evaluate_pairs([dev.id("s1")], [None], symmetric=True)


def test_loop_detector_evaluate_equals_evaluate_pairs(capi):
    from gloc3d_amd.loop_detector import RpyPCLoopDetector
    det = RpyPCLoopDetector(k_dim=8)
    try:
        places = ["t", "s2", "far"]
        for k, name in enumerate(places):
            det.add_keyframe(np.full(8, float(k), np.float32), EC.cloud(name))
        T = np.stack([EC.truth("s1"), np.linalg.inv(EC.truth("s2")) @ EC.truth("s1"), np.eye(4)]).astype(np.float32)
        q = EC.cloud("s1")
        for gate in (None, 2.0):
            got = det.evaluate(q, [0, 1, 2], T, max_corr_dist=gate)
            qid = det._reg.scan_upload(q)
            try:
                prm = capi.default_eval_params() if gate is None else capi.default_eval_params(max_corr_dist=gate)
                want = det._reg.evaluate_pairs([qid] * 3, [det._db_scan_ids[i] for i in range(3)], T=T, params=prm)
            finally:
                det._reg.scan_release(qid)
            assert _same(want, got) and set(got) == set(FIELDS)
            assert got["fitness"][0] > got["fitness"][2] > 0
    finally:
        det.close()


def test_a_handle_after_refusals_answers_as_a_fresh_one(capi, dev):
    import ctypes as C
    rows = EC.MIXED
    want = _singles(dev)
    src, tgt = [dev.id(r["src"]) for r in rows], [capi.NO_SCAN if r["tgt"] is None else dev.id(r["tgt"]) for r in rows]
    T = np.ascontiguousarray(np.stack([r["T"] for r in rows]), np.float32)
    fn = capi.lib().gloc_reg_evaluate_pairs

    def raw(s, t, prm):
        """The C entry on arrays of sentinels: (return code, are the outputs untouched)."""
        s, t = np.ascontiguousarray(s, np.uint32), np.ascontiguousarray(t, np.uint32)
        n = len(s)
        fit, rmse, cnt = np.full(n, 7.0, np.float32), np.full(n, 7.0, np.float32), np.full(n, 77, np.uint32)
        info, g = np.full((n, 36), 7.0), np.full((n, 6), 7.0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = fn(dev.reg._h, p(s), p(t), n, p(T), C.byref(prm), p(fit), p(rmse), p(cnt), p(info), p(g))
        return rc, bool((fit == 7.0).all() and (rmse == 7.0).all() and (cnt == 77).all() and (info == 7.0).all() and (g == 7.0).all())

    good = capi.default_eval_params()
    bad_src, bad_tgt, empty_src = list(src), list(tgt), list(src)
    bad_src[2], bad_tgt[2], empty_src[-1] = 123456, 123456, dev.id("empty")
    for s, t, prm in ((bad_src, tgt, good), (src, bad_tgt, good), (empty_src, tgt, good), (src, tgt, capi.default_eval_params(max_corr_dist=0.0))):
        assert raw(s, t, prm) == (1, True)                                     # GLOC_ERR_INVALID, outputs untouched
        assert _same(want, dev.evaluate(rows))
    dev.reg.batch_multi_begin([dev.id("s1")], [[dev.id("t")]], params=capi.default_reg_params(ransac_iters=0, icp_iters=2))
    try:
        assert raw(src, tgt, good) == (5, True)                                # GLOC_ERR_STATE: a batch in flight
    finally:
        dev.reg.batch_multi_end()
    assert _same(want, dev.evaluate(rows))
    fresh = capi.Registrar(store=dev.store)
    try:
        assert _same(want, dev.evaluate(rows, reg=fresh))
    finally:
        fresh.close()
