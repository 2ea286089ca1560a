"""GPU: the pair-list entries of the three Gauss-Newton refinements (gloc_reg_{p2l,gicp,vgicp}_pairs) -- a ragged batch
through the accumulate and solve kernels: a source, a work-group count and a run of partial rows per job.

What holds, and is asserted bit for bit: row c of a list is the single-source entry's result for (src[c], [tgt[c]]) --
T, rmse, iterations, status and, with a robust block, the mean weight -- whatever the list, the row's position in it and
the other rows' sizes, stops and scans.  Against the float64 restatements (tests/pairs_cases.py, whose verdicts
tests/test_pairs_cases_cpu.py proves): a pose within 1e-4 m / 1e-4 rad and an rmse within 1e-4 (tests/test_p2l_gpu.py's
tolerances), iterations and status exact."""
import numpy as np
import pytest

import gn_cases as GC
import pairs_cases as PC
import p2l_ref as P
from util import bits

pytestmark = pytest.mark.gpu

INVALID, STATE = 1, 5
ROBUST = ("plain", "cauchy")
COMBOS = [(m, b, r) for m in PC.METHODS for b in PC.BLOCKS for r in ROBUST]


class Dev:
    """A scan store and a registrar with clouds uploaded by name (gn_cases.cloud; normals built with k = 10)."""

    def __init__(self, capi, store=None):
        self.capi = capi
        self.own = store is None
        self.store = capi.ScanStore() if store is None else store
        self.reg = capi.Registrar(store=self.store)
        self.ids = {}

    def id(self, name):
        if name is None:
            return None
        if name not in self.ids:
            xyz = GC.cloud(name)
            self.ids[name] = self.store.add(xyz)
            if len(xyz):
                self.store.build_normals(self.ids[name], GC.NORMAL_K)
        return self.ids[name]

    def prm(self, method, block=None, **over):
        p = dict(PC.params(method, block) if block else {}, **over)
        return getattr(self.capi, "default_%s_params" % method)(**p)

    def rb(self, method, robust):
        return None if robust in (None, "plain") else self.capi.default_robust_params(**PC.robust(method))

    def pairs(self, method, names, init, prm, robust=None, reg=None):
        """names: [(source, target or None)]."""
        return getattr(reg or self.reg, method + "_pairs")([self.id(s) for s, _ in names], [self.id(t) for _, t in names],
                                                           init_T=np.ascontiguousarray(init, np.float32), params=prm,
                                                           robust=self.rb(method, robust))

    def batch(self, method, src, tgts, init, prm, robust=None, reg=None):
        return getattr(reg or self.reg, method + "_batch")(self.id(src), [self.id(t) for t in tgts], init_T=np.ascontiguousarray(init, np.float32),
                                                           params=prm, robust=self.rb(method, robust))

    def singles(self, method, names, init, prm, robust=None):
        """The rows of n calls of the single-source entry, one target each."""
        return _stack([self.batch(method, s, [t], init[j:j + 1], prm, robust) for j, (s, t) in enumerate(names)])

    def close(self):
        self.reg.close()
        if self.own:
            self.store.close()


def _stack(outs):
    return tuple(np.concatenate([o[k] for o in outs]) for k in range(len(outs[0])))


def _take(out, idx):
    return tuple(o[np.asarray(idx, np.int64)] for o in out)


def _same(a, b):
    return bool(len(a) == len(b) and (bits(a[0]) == bits(b[0])).all() and (bits(a[1]) == bits(b[1])).all() and (a[2] == b[2]).all()
                and (a[3] == b[3]).all() and (len(a) < 5 or (bits(a[4]) == bits(b[4])).all()))


def _names(prs):
    return [(p["src"], p["tgt"]) for p in prs]


@pytest.fixture(scope="module")
def dev(capi):
    d = Dev(capi)
    yield d
    d.close()


_SINGLES = {}


def _singles(dev, method, block, robust):
    """The single-source entries' rows of the whole list: computed once per (method, block, robust), never changed."""
    key = (method, block, robust)
    if key not in _SINGLES:
        prs = PC.pairs(block)
        out = dev.singles(method, _names(prs), PC.guesses(prs), dev.prm(method, block), robust)
        for o in out:
            o.setflags(write=False)
        _SINGLES[key] = out
    return _SINGLES[key]


# ---- 1. rows equal the single-source entries ------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,block,robust", COMBOS)
def test_rows_equal_the_single_source_entries_bit_for_bit(dev, method, block, robust):
    """The whole list as ONE call: sources of one lane to 47 work-groups, ld and n_groups different per row, rows that freeze
    at different passes while others run on."""
    prs = PC.pairs(block)
    want = _singles(dev, method, block, robust)
    got = dev.pairs(method, _names(prs), PC.guesses(prs), dev.prm(method, block), robust)
    print(f"{method} {block} {robust}: status {got[3].tolist()}, iters {got[2].tolist()}")
    assert len(got) == (4 if robust == "plain" else 5)
    assert _same(want, got), [j for j in range(len(prs)) if not _same(_take(want, [j]), _take(got, [j]))]
    assert _same(got, dev.pairs(method, _names(prs), PC.guesses(prs), dev.prm(method, block), robust))      # the same bits on a second run
    if block == "P1" and robust == "plain":
        assert {0, 1, 2} <= set(got[3].tolist()) and len(set(got[2][got[3] == 1].tolist())) >= 3            # the list's mix of ends


def test_kind_none_is_the_plain_step_with_weights_of_one(dev):
    for method in PC.METHODS:
        prs = PC.pairs("P1")
        none = dev.capi.default_robust_params()
        got = getattr(dev.reg, method + "_pairs")([dev.id(p["src"]) for p in prs], [dev.id(p["tgt"]) for p in prs], init_T=PC.guesses(prs),
                                                  params=dev.prm(method, "P1"), robust=none)
        assert _same(_singles(dev, method, "P1", "plain"), got[:4])
        assert set(got[4].tolist()) <= {0.0, 1.0} and (got[4] == 1.0).sum() >= 15


# ---- 2. against the restatements --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,block,robust", COMBOS)
def test_rows_follow_the_restatements(dev, oracle_mod, method, block, robust):
    """Plain: every pair the restatements call stable -- all but the one tests/pairs_cases.py names.  With the robust block:
    the first six pairs, through tests/robust_ref.py."""
    prs = PC.pairs(block)
    got = dev.pairs(method, _names(prs), PC.guesses(prs), dev.prm(method, block), robust)
    left_out = 0
    for j, p in enumerate(prs if robust == "plain" else prs[:6]):
        if (method, p["src"], p["tgt"]) in PC.LEFT_OUT:
            left_out += 1
            continue
        r = PC.reference(p, method, block, oracle_mod, None if robust == "plain" else PC.robust(method))
        assert r["stable"], (p["src"], p["tgt"])
        ref = r["ref"]
        dt, da = P.pose_err(ref["T"], got[0][j])
        print(f"{method} {block} {robust} ({p['src']}, {p['tgt']}): iters {got[2][j]} / {ref['iters']}, status {got[3][j]} / {ref['status']}, "
              f"rmse {got[1][j]:.6f} / {ref['rmse']:.6f}; against the restatement {dt:.2e} m {da:.2e} rad")
        assert dt <= 1e-4 and da <= 1e-4 and abs(got[1][j] - ref["rmse"]) <= 1e-4
        assert int(got[2][j]) == ref["iters"] and int(got[3][j]) == ref["status"]
        if robust != "plain":
            assert abs(got[4][j] - ref["weight"]) <= 1e-6
    assert left_out == (1 if (method, robust) == ("p2l", "plain") else 0)


# ---- 3. order and repetition change no bit ----------------------------------------------------------------------------------------
def _orders(prs):
    n = len(prs)
    size = [len(GC.cloud(p["src"])) for p in prs]
    one = next(j for j, p in enumerate(prs) if p["src"] == "a2_n1")
    return {"reversed": list(range(n))[::-1], "ascending": sorted(range(n), key=lambda j: (size[j], j)),
            "descending": sorted(range(n), key=lambda j: (-size[j], j)), "twice": [j for j in range(n) for _ in (0, 1)],
            "shortest first": [one] + [j for j in range(n) if j != one]}


@pytest.mark.parametrize("method,block,robust", COMBOS)
def test_order_and_repetition_change_no_bit(dev, method, block, robust):
    """The list reversed, sorted by source size both ways, every pair twice in a row, the one-point source as job 0: every
    row is test 1's row."""
    prs, want = PC.pairs(block), _singles(dev, method, block, robust)
    names, init, prm = _names(prs), PC.guesses(prs), dev.prm(method, block)
    for what, idx in _orders(prs).items():
        got = dev.pairs(method, [names[j] for j in idx], init[idx], prm, robust)
        assert _same(_take(want, idx), got), (what, [k for k, j in enumerate(idx) if not _same(_take(want, [j]), _take(got, [k]))])


@pytest.mark.parametrize("method", PC.METHODS)
def test_a_target_index_on_every_source(capi, dev, method):
    """build_target_index on every scan that is a source re-sorts it into kd order.  As a TARGET such a scan gives the same
    bits as before (the order of a target never changes a result).  As a SOURCE it is summed in its new order -- which is
    what the single-source entries do with it too (tests/test_gicp_gpu.py::test_a_source_in_kd_order_gives_the_same_result:
    the same pairs summed in another order, the same result to an ulp or two of the fp32 outputs, not to the bit): the list's
    rows equal the single-source entries' on the scans as they now are, bit for bit, and test 1's rows in iterations and
    status and to 2e-6 m / 2e-6 rad in the pose -- two ulps of an fp32 translation below 8 m -- but for the pair the
    restatements themselves call unstable under another summation order (pairs_cases.LEFT_OUT)."""
    d = Dev(capi)
    try:
        for block in PC.BLOCKS:
            prs = PC.pairs(block)
            names, init, prm = _names(prs), PC.guesses(prs), d.prm(method, block)
            for s in sorted({p["src"] for p in prs}):
                d.store.build_target_index(d.id(s))
            for robust in ROBUST:
                got = d.pairs(method, names, init, prm, robust)
                assert _same(d.singles(method, names, init, prm, robust), got)
                was = _singles(dev, method, block, robust)
                keep = [j for j, p in enumerate(prs) if (method, p["src"], p["tgt"]) not in PC.LEFT_OUT]
                moved = sum(not _same(_take(was, [j]), _take(got, [j])) for j in keep)
                worst = max(max(P.pose_err(was[0][j], got[0][j])) for j in keep)
                print(f"{method} {block} {robust}: {moved} of {len(keep)} rows differ in some bit from the rows before the re-sort, poses by at most {worst:.2e}")
                assert (was[2][keep] == got[2][keep]).all() and (was[3][keep] == got[3][keep]).all() and worst <= 2e-6
    finally:
        d.close()


# ---- 4. degenerate lists ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", PC.METHODS)
def test_one_source_many_targets_many_sources_one_target_and_one_pair(dev, method):
    prm = dev.prm(method, "P1")
    tgts = ["a0", "a1", "b0", "a0_odd", "empty", "a0_dup"]
    init = np.stack([(GC.truth("a2", t) @ GC._se3(0.3 * j, (0.05, -0.02 * j, 0.01))).astype(np.float32) for j, t in enumerate(tgts)])
    srcs = ["a2", "a3", "a2_n65", "a2_odd", "a0_dup", "a0"]
    init2 = np.stack([(GC.truth(s, "a0") @ GC._se3(-0.3 * j, (0.02 * j, 0.03, 0.0))).astype(np.float32) for j, s in enumerate(srcs)])
    for robust in ROBUST:
        assert _same(dev.batch(method, "a2", tgts, init, prm, robust), dev.pairs(method, [("a2", t) for t in tgts], init, prm, robust))
        names = [(s, "a0") for s in srcs]
        assert _same(dev.singles(method, names, init2, prm, robust), dev.pairs(method, names, init2, prm, robust))
        for j in (0, 2):
            assert _same(dev.batch(method, srcs[j], ["a0"], init2[j:j + 1], prm, robust), dev.pairs(method, names[j:j + 1], init2[j:j + 1], prm, robust))


@pytest.mark.parametrize("method,robust", [(m, r) for m in PC.METHODS for r in ROBUST])
def test_rows_without_a_target(dev, method, robust):
    """None in the first, a middle and the last row: the row of an empty target scan -- the guess, 0 iterations, status 2,
    rmse 0, weight 0 -- and the neighbours' bits stay."""
    prs, want = PC.pairs("P1"), _singles(dev, method, "P1", robust)
    names, init, prm = _names(prs), PC.guesses(prs), dev.prm(method, "P1")
    gone = [0, 10, len(prs) - 1]
    got = dev.pairs(method, [(s, None if j in gone else t) for j, (s, t) in enumerate(names)], init, prm, robust)
    kept = [j for j in range(len(prs)) if j not in gone]
    assert _same(_take(want, kept), _take(got, kept))
    empty = dev.singles(method, [(names[j][0], "empty") for j in gone], init[gone], prm, robust)
    assert _same(empty, _take(got, gone))
    for j in gone:
        assert (bits(got[0][j]) == bits(init[j])).all() and got[1][j] == 0 and got[2][j] == 0 and got[3][j] == 2
        assert robust == "plain" or got[4][j] == 0
    only = dev.pairs(method, [("a2", None)], init[:1], prm, robust)                    # a list of nothing but such a row
    assert _same(_take(got, [0]), only)


# ---- 5. a full-size ragged list -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["p2l", "gicp"])
def test_a_full_size_ragged_list(dev, method):
    """Two ~122 k-point scans and a 12.8 k one: ~480 work-groups against 47 in one launch."""
    big_s, big_t = "full_s", "full_t"
    assert len(GC.cloud(big_s)) > 100000 and len(GC.cloud(big_t)) > 100000
    names = [(big_s, big_t), ("a2", big_t), (big_s, "a0")]
    off = GC._se3(0.5, (0.1, 0.05, 0.01))
    init = np.stack([GC._se3(1.5, (0.3, -0.1, 0.0)) @ off, GC.scan_poses()[2] @ off, GC._se3(1.5, (0.3, -0.1, 0.0)) @ off]).astype(np.float32)
    prm = dev.prm(method, max_iters=2)
    got = dev.pairs(method, names, init, prm)
    print(f"{method} full size: status {got[3].tolist()}, iters {got[2].tolist()}, rmse {got[1].tolist()}")
    assert (got[2] == 2).all() and (got[3] == 0).all() and (got[1] > 0).all()
    assert _same(dev.singles(method, names, init, prm), got)


# ---- 6. one handle --------------------------------------------------------------------------------------------------------------------
def test_one_handle_through_pairs_and_the_other_entries(capi):
    """pairs (the large list), pairs (one tiny pair), p2l_batch, a RANSAC + ICP batch_multi, pairs again, on ONE handle: each
    equals the same call on a fresh handle bit for bit -- the workspaces a call grows or leaves behind change nothing -- and the
    store's bytes come back after the releases."""
    store = capi.ScanStore()
    live0 = store.bytes()[0]
    one = Dev(capi, store)
    try:
        prs = PC.pairs("P1")
        names, init = _names(prs), PC.guesses(prs)
        rprm = capi.default_reg_params(ransac_iters=64, icp_iters=3)
        tiny = [("a2_n1", "a0")]
        calls = [
            lambda d, r: d.pairs("gicp", names, init, d.prm("gicp", "P1"), "cauchy", reg=r),
            lambda d, r: d.pairs("p2l", tiny, init[6:7], d.prm("p2l", "P2"), reg=r),
            lambda d, r: d.batch("p2l", "a2", ["a0", "b0", "empty"], init[:3], d.prm("p2l", "P1"), reg=r),
            lambda d, r: r.batch_multi([d.id("a2"), d.id("a3")], [[d.id("a0"), d.id("a1")], [d.id("a1"), capi.NO_SCAN]], params=rprm),
            lambda d, r: d.pairs("vgicp", names, init, d.prm("vgicp", "P1"), reg=r),
            lambda d, r: d.pairs("p2l", names, init, d.prm("p2l", "P1"), "cauchy", reg=r),
        ]
        for k, call in enumerate(calls):
            got = call(one, one.reg)
            fresh = capi.Registrar(store=store)
            try:
                want = call(one, fresh)
            finally:
                fresh.close()
            if isinstance(got, dict):
                assert all((bits(got[f]) == bits(want[f])).all() if got[f].dtype.kind == "f" else (got[f] == want[f]).all() for f in got), k
            else:
                assert _same(want, got), k
        one.reg.close()
        for sid in one.ids.values():
            store.release(sid)
        assert store.bytes()[0] == live0 and len(store) == 0
    finally:
        store.close()


# ---- 7. refusals on a live handle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", PC.METHODS)
def test_refusals_leave_the_outputs_and_the_handle_alone(capi, dev, method):
    import ctypes as C
    prs = PC.pairs("P2")[:7]
    names, init, prm = _names(prs), PC.guesses(prs), dev.prm(method, "P2")
    want = dev.pairs(method, names, init, prm, "cauchy")
    src, tgt = [dev.id(s) for s, _ in names], [dev.id(t) for _, t in names]
    empty = dev.id("empty")
    fn = getattr(capi.lib(), "gloc_reg_%s_pairs" % method)
    rb = dev.rb(method, "cauchy")

    def raw(s, t):
        """The C entry on arrays of sentinels: (return code, are the outputs untouched)."""
        s, t = np.ascontiguousarray(s, np.uint32), np.ascontiguousarray(t, np.uint32)
        n = len(s)
        T, rmse, w = np.full((n, 16), 7.0, np.float32), np.full(n, 7.0, np.float32), np.full(n, 7.0, np.float32)
        it, st = np.full(n, 77, np.uint32), np.full(n, 77, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = fn(dev.reg._h, p(s), p(t), n, p(np.ascontiguousarray(init, np.float32)), C.byref(prm), C.byref(rb), p(T), p(rmse), p(it), p(st), p(w))
        return rc, bool((T == 7.0).all() and (rmse == 7.0).all() and (w == 7.0).all() and (it == 77).all() and (st == 77).all())

    bad_src, bad_tgt, empty_src = list(src), list(tgt), list(src)
    bad_src[3], bad_tgt[3], empty_src[-1] = 123456, 123456, empty
    for s, t in ((bad_src, tgt), (src, bad_tgt), (empty_src, tgt)):
        assert raw(s, t) == (INVALID, True)
        assert _same(want, dev.pairs(method, names, init, prm, "cauchy"))                 # the next good call: a fresh handle's (below)
    dev.reg.batch_multi_begin([dev.id("a2")], [[dev.id("a0")]], params=capi.default_reg_params(ransac_iters=0, icp_iters=2))
    try:
        assert raw(src, tgt) == (STATE, True)
    finally:
        dev.reg.batch_multi_end()
    assert _same(want, dev.pairs(method, names, init, prm, "cauchy"))
    fresh = capi.Registrar(store=dev.store)
    try:
        assert _same(want, dev.pairs(method, names, init, prm, "cauchy", reg=fresh))
    finally:
        fresh.close()
