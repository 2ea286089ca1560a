"""GPU: the system form of the pair lists (gloc_reg_{p2l,gicp,vgicp}_pairs_system) -- every row of a mixed list equals the
single-pair entry's result bit for bit: gloc_reg_<m>_system with the plain step, gloc_reg_<m>_system_robust with a robust
block at the same pass.  H, g, the squared-residual sum, the count and the weights' sum.

The list is the mixed list of tests/eval_cases.py: sources of 1, 257 and about 6 400 points, non-finite rows, an empty
target, a scan against itself, one row twice, the integer lattice -- and a row without a target, which no single-pair
entry can name: it has to be the row of an empty target scan, all zeros."""
import numpy as np
import pytest

import eval_cases as EC

pytestmark = pytest.mark.gpu

METHODS = ("p2l", "gicp", "vgicp")
SCALE = {"p2l": 0.1, "gicp": 2.0, "vgicp": 2.0}        # metres for point-to-plane, sqrt(e^T M e) for the other two
# (robust, pass): the plain step; Cauchy annealed from 4 x the scale by 0.5 -- at pass 0 (4 x the scale) and 3 (the scale)
MODES = [("plain", 0), ("cauchy", 0), ("cauchy", 3)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b):
    return len(a) == len(b) and all((bits(np.asarray(x)) == bits(np.asarray(y))).all() for x, y in zip(a, b))


@pytest.fixture(scope="module")
def dev(capi):
    store = capi.ScanStore()
    reg = capi.Registrar(store=store)
    ids = {}

    def id_of(name):
        if name not in ids:
            ids[name] = store.add(EC.cloud(name))
        return ids[name]

    yield dict(store=store, reg=reg, id=id_of)
    reg.close()
    store.close()


def _prm(capi, method):
    return getattr(capi, "default_%s_params" % method)(max_corr_dist=1.0)


def _rb(capi, method, robust):
    if robust == "plain":
        return None
    return capi.default_robust_params(kind=2, scale=SCALE[method], scale_start=4.0 * SCALE[method], anneal=0.5)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("robust,rpass", MODES)
def test_rows_equal_the_single_pair_entries_bit_for_bit(capi, dev, method, robust, rpass):
    rows = EC.MIXED
    reg, id_of = dev["reg"], dev["id"]
    prm, rb = _prm(capi, method), _rb(capi, method, robust)
    T = np.stack([r["T"] for r in rows])
    src = [id_of(r["src"]) for r in rows]
    tgt = [None if r["tgt"] is None else id_of(r["tgt"]) for r in rows]
    got = getattr(reg, method + "_pairs_system")(src, tgt, T, prm, robust=rb, robust_pass=rpass)
    assert len(got) == (4 if rb is None else 5) and got[0].shape == (len(rows), 6, 6) and got[3].dtype == np.uint64
    single = getattr(reg, method + "_system")
    counts = []
    for c, r in enumerate(rows):
        t = id_of("empty") if tgt[c] is None else tgt[c]        # no target: the row of an empty target scan
        want = single(src[c], t, T[c], prm, robust=rb, robust_pass=rpass)
        row = tuple(o[c] for o in got)
        assert _same(want, row), (c, r["src"], r["tgt"])
        if r["tgt"] in (None, "empty"):
            assert not any(np.asarray(o).any() for o in row)
        counts.append(int(row[3]))
    print(f"{method} {robust} pass {rpass}: pairs {counts}")
    assert sum(k > 0 for k in counts) >= 6 and (got[0] == got[0].transpose(0, 2, 1)).all()
    a, b = EC.TWICE
    assert _same(tuple(o[a] for o in got), tuple(o[b] for o in got))
    # another order, and a list of one: the same rows
    idx = list(range(len(rows)))[::-1]
    back = getattr(reg, method + "_pairs_system")([src[c] for c in idx], [tgt[c] for c in idx], T[idx], prm, robust=rb, robust_pass=rpass)
    assert _same(tuple(o[idx] for o in got), back)
    one = getattr(reg, method + "_pairs_system")(src[2:3], tgt[2:3], T[2:3], prm, robust=rb, robust_pass=rpass)
    assert _same(tuple(o[2:3] for o in got), one)
    if rb is not None and rpass == 3:                             # the two passes weigh differently
        other = getattr(reg, method + "_pairs_system")(src, tgt, T, prm, robust=rb, robust_pass=0)
        assert (other[4][2] != got[4][2]) and (other[3] == got[3]).all()


@pytest.mark.parametrize("method", METHODS)
def test_refusals_leave_the_outputs_and_the_handle_alone(capi, dev, method):
    import ctypes as C
    rows = EC.MIXED[:4]
    reg, id_of = dev["reg"], dev["id"]
    prm = _prm(capi, method)
    T = np.ascontiguousarray(np.stack([r["T"] for r in rows]), np.float32)
    src = [id_of(r["src"]) for r in rows]
    tgt = [capi.NO_SCAN if r["tgt"] is None else id_of(r["tgt"]) for r in rows]
    call = lambda: getattr(reg, method + "_pairs_system")(src, [None if t == capi.NO_SCAN else t for t in tgt], T, prm)
    want = call()
    fn = getattr(capi.lib(), "gloc_reg_%s_pairs_system" % method)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bad = list(src)
    bad[1] = 123456
    for s, t in ((bad, tgt), (src, [123456] + tgt[1:]), ([id_of("empty")] + src[1:], tgt)):
        s, t = np.ascontiguousarray(s, np.uint32), np.ascontiguousarray(t, np.uint32)
        H, g, sm, cnt = np.full((4, 36), 7.0), np.full((4, 6), 7.0), np.full(4, 7.0), np.full(4, 77, np.uint64)
        rc = fn(reg._h, p(s), p(t), 4, p(T), C.byref(prm), None, 0, p(H), p(g), p(sm), p(cnt), None)
        assert rc == 1 and (H == 7.0).all() and (g == 7.0).all() and (sm == 7.0).all() and (cnt == 77).all()
        assert _same(want, call())
