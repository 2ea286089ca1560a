"""GPU: gloc_scan_store_cluster against tests/cluster_ref.py on the case table tests/cluster_cases.py and on 30 seeded
random clouds.  Everything is exact: == on the uint32 outputs, bit-equal float32 corners and float64 centroids (E4 states
the order of every sum).  The labels are defined without reference to any order of execution, so the same call twice, and
the same scan with a target index, must give the same arrays."""
import ctypes as C

import numpy as np
import pytest

import cluster_cases as K
from util import bits

pytestmark = pytest.mark.gpu
INV = 1                 # GLOC_ERR_INVALID (include/gloc3d.h)
FIELDS_U32 = ("root", "cluster", "size", "cluster_root")


@pytest.fixture(scope="module")
def store(capi):
    s = capi.ScanStore()
    yield s
    s.close()


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, ref):
    """Where two answers differ, as a list of words (empty: equal in every bit)."""
    off = [f for f in FIELDS_U32 if got.__dict__[f].shape != ref[f].shape or (got.__dict__[f] != ref[f]).any()]
    off += [f for f in ("n_components", "n_kept") if got.__dict__[f] != ref[f]]
    if "centroid" in ref and not off:
        off += ["centroid"] if (_bits64(got.centroid) != _bits64(ref["centroid"])).any() else []
        off += [f for f in ("lo", "hi") if (bits(got.__dict__[f]) != bits(ref[f])).any()]
    return off


def _as_ref(got):
    return dict(got.__dict__)


@pytest.mark.parametrize("name", list(K.CASES))
def test_cases_equal_the_restatement(store, capi, name):
    xyz, prm, ref = K.cloud(name), capi.default_cluster_params(**K.CASES[name][1]), K.ref(name)
    sid = store.add(xyz)
    got = store.cluster(sid, prm)
    print(name, "points", len(xyz), "components", got.n_components, "kept", got.n_kept, "largest", got.size[:1], "off", _same(got, ref))
    assert _same(got, ref) == []
    again = store.cluster(sid, prm)                        # run to run
    assert _same(again, _as_ref(got)) == []
    store.build_target_index(sid)                          # other chunks and boxes, the same graph
    assert _same(store.cluster(sid, prm), _as_ref(got)) == []
    assert _same(store.cluster(sid, prm, figures=False), {k: v for k, v in ref.items() if k not in ("centroid", "lo", "hi")}) == []
    store.release(sid)


@pytest.mark.parametrize("seed", range(K.N_FUZZ))
def test_fuzz_equals_the_restatement(store, capi, seed):
    (xyz, tol), ref = K.fuzz(seed), K.fuzz_ref(seed)
    sid = store.add(xyz)
    got = store.cluster(sid, capi.default_cluster_params(tolerance=tol))
    print("seed", seed, "points", len(xyz), "tolerance", tol, "components", got.n_components, "off", _same(got, ref))
    assert _same(got, ref) == []
    assert _same(store.cluster(sid, capi.default_cluster_params(tolerance=tol)), _as_ref(got)) == []
    store.release(sid)


def test_counts_come_back_where_a_buffer_is_too_small(store, capi):
    L, name = capi.lib(), "sizes_all"
    xyz, ref, prm = K.cloud(name), K.ref(name), capi.default_cluster_params(**K.CASES[name][1])
    sid = store.add(xyz)
    n, kept = len(xyz), ref["n_kept"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    root, size, cent = np.full(n, 7, np.uint32), np.full(kept, 7, np.uint32), np.full((kept, 3), 7.0)
    nc, nk = C.c_uint32(0), C.c_uint32(0)
    # the cluster buffers one row short: refused, the counts are there, the point buffer (large enough) is written
    rc = L.gloc_scan_store_cluster(store._h, sid, C.byref(prm), p(root), None, n, p(size), None, p(cent), None, None, kept - 1, C.byref(nc), C.byref(nk))
    assert rc == INV and (nc.value, nk.value) == (ref["n_components"], kept)
    assert (root == ref["root"]).all() and (size == 7).all() and (cent == 7.0).all()
    # the point buffer one entry short
    root[:] = 7
    nc.value = nk.value = 0
    rc = L.gloc_scan_store_cluster(store._h, sid, C.byref(prm), p(root), None, n - 1, p(size), None, None, None, None, kept, C.byref(nc), C.byref(nk))
    assert rc == INV and (nc.value, nk.value) == (ref["n_components"], kept) and (root == 7).all() and (size == ref["size"]).all()
    # no buffer at all asks for the counts
    nc.value = nk.value = 0
    rc = L.gloc_scan_store_cluster(store._h, sid, C.byref(prm), None, None, 0, None, None, None, None, None, 0, C.byref(nc), C.byref(nk))
    assert rc == 0 and (nc.value, nk.value) == (ref["n_components"], kept)
    # only the roots
    rc = L.gloc_scan_store_cluster(store._h, sid, C.byref(prm), p(root), None, n, None, None, None, None, None, 0, None, None)
    assert rc == 0 and (root == ref["root"]).all()
    store.release(sid)
    assert L.gloc_scan_store_cluster(store._h, sid, C.byref(prm), None, None, 0, None, None, None, None, None, 0, C.byref(nc), C.byref(nk)) == INV


def test_an_empty_scan_has_no_component(store, capi):
    sid = store.add(np.zeros((0, 3), np.float32))
    got = store.cluster(sid)
    assert (got.n_components, got.n_kept, len(got.root), len(got.size)) == (0, 0, 0, 0)
    store.release(sid)
