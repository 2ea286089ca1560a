"""CPU: the C ABI of the Euclidean clusters and outlier filters -- symbols, struct sizes and offsets, defaults, and every
refusal that comes before the handle, with the outputs untouched (a null store stands in for the handle)."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gloc_cluster_default_params", "gloc_scan_store_cluster", "gloc_scan_filter_default_params", "gloc_scan_store_add_filtered",
       "gloc_scan_store_add_subset")
INV = 1                 # GLOC_ERR_INVALID (include/gloc3d.h)
NAN, INF = float("nan"), float("inf")


def _err(L):
    L.gloc_last_error.restype = C.c_char_p
    return L.gloc_last_error()


def _cluster(L, prm, st=None):
    """gloc_scan_store_cluster with every output given: (return code, True iff no output was written)."""
    root, label = np.full(4, 7, np.uint32), np.full(4, 7, np.uint32)
    size, croot = np.full(4, 7, np.uint32), np.full(4, 7, np.uint32)
    cent, lo, hi = np.full((4, 3), 7.0), np.full((4, 3), 7, np.float32), np.full((4, 3), 7, np.float32)
    nc, nk = C.c_uint32(7), C.c_uint32(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = L.gloc_scan_store_cluster(st, 0, None if prm is None else C.byref(prm), p(root), p(label), 4, p(size), p(croot), p(cent), p(lo), p(hi), 4,
                                   C.byref(nc), C.byref(nk))
    untouched = all((a == 7).all() for a in (root, label, size, croot, cent, lo, hi)) and nc.value == 7 and nk.value == 7
    return rc, untouched


def _filtered(L, prm, st=None):
    sid, info = C.c_uint32(7), (C.c_uint32 * 5)(7, 7, 7, 7, 7)
    rc = L.gloc_scan_store_add_filtered(st, 0, None if prm is None else C.byref(prm), C.cast(C.pointer(sid), C.c_void_p),
                                        C.cast(info, C.c_void_p))
    return rc, sid.value == 7 and list(info) == [7] * 5


def test_symbols_exported(capi):
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.gloc_abi_version() == 6


def test_struct_sizes_and_offsets(capi):
    cp, fp, fi = capi.ClusterParams, capi.ScanFilterParams, capi.ScanFilterInfo
    assert C.sizeof(cp) == 16 and [getattr(cp, f).offset for f in ("tolerance", "min_size", "max_size", "reserved_")] == [0, 4, 8, 12]
    assert C.sizeof(fp) == 40
    assert [getattr(fp, f).offset for f in ("min_range", "max_range", "ror_radius", "ror_min_neighbors", "sor_mean_k", "sor_std_mul", "cluster")] == \
        [0, 4, 8, 12, 16, 20, 24]
    assert C.sizeof(fi) == 20 and [getattr(fi, f).offset for f in ("points_in", "after_range", "after_ror", "after_sor", "after_cluster")] == \
        [0, 4, 8, 12, 16]


def test_defaults(capi):
    p = capi.default_cluster_params()
    assert (p.tolerance, p.min_size, p.max_size, p.reserved_) == (0.5, 1, 0, 0)
    f = capi.default_scan_filter_params()                  # everything off
    assert (f.min_range, f.max_range, f.ror_radius, f.ror_min_neighbors, f.sor_mean_k) == (0.0, 0.0, 0.0, 0, 0)
    assert np.isfinite(f.sor_std_mul)
    assert (f.cluster.tolerance, f.cluster.min_size, f.cluster.max_size, f.cluster.reserved_) == (0.0, 1, 0, 0)
    assert capi.default_cluster_params(min_size=5).min_size == 5
    g = capi.default_scan_filter_params(ror_radius=0.5, cluster_tolerance=0.7, cluster_min_size=9)
    assert (g.ror_radius, g.cluster.min_size) == (0.5, 9) and g.cluster.tolerance == np.float32(0.7)
    capi.lib().gloc_cluster_default_params(None)           # a null block is ignored
    capi.lib().gloc_scan_filter_default_params(None)


# the refusals of gloc_scan_store_cluster, in the order the entry checks them: (fields, word of the message)
CLUSTER_BAD = [(None, b"null"), (dict(tolerance=-0.5), b"tolerance"), (dict(tolerance=NAN), b"tolerance"), (dict(tolerance=INF), b"tolerance"),
               (dict(tolerance=-INF), b"tolerance"), (dict(tolerance=0.0), b"tolerance"), (dict(min_size=5, max_size=4), b"min_size"),
               (dict(reserved_=1), b"reserved_")]


@pytest.mark.parametrize("over,word", CLUSTER_BAD)
def test_cluster_refusals_before_the_handle(capi, over, word):
    L = capi.lib()
    rc, untouched = _cluster(L, None if over is None else capi.default_cluster_params(**over))
    assert rc == INV and word in _err(L) and untouched


# ... and of gloc_scan_store_add_filtered
FILTER_BAD = [(None, b"null"), (dict(ror_radius=-1.0), b"ror_radius"), (dict(ror_radius=NAN), b"ror_radius"), (dict(ror_radius=INF), b"ror_radius"),
              (dict(cluster_tolerance=-1.0), b"tolerance"), (dict(cluster_tolerance=NAN), b"tolerance"), (dict(cluster_tolerance=INF), b"tolerance"),
              (dict(cluster_tolerance=0.5, cluster_min_size=3, cluster_max_size=2), b"min_size"),
              (dict(cluster_min_size=3, cluster_max_size=2), b"min_size"),
              (dict(sor_mean_k=16), b"sor_mean_k"), (dict(sor_mean_k=4, sor_std_mul=NAN), b"sor_std_mul"), (dict(sor_std_mul=INF), b"sor_std_mul"),
              (dict(cluster_reserved_=2), b"reserved_"), (dict(min_range=NAN), b"range"), (dict(max_range=INF), b"range"),
              (dict(min_range=5.0, max_range=4.0), b"min_range")]


@pytest.mark.parametrize("over,word", FILTER_BAD)
def test_filter_refusals_before_the_handle(capi, over, word):
    L = capi.lib()
    rc, untouched = _filtered(L, None if over is None else capi.default_scan_filter_params(**over))
    assert rc == INV and word in _err(L) and untouched


def test_the_first_fault_in_the_stated_order_is_the_one_reported(capi):
    L = capi.lib()
    rc, _ = _cluster(L, capi.default_cluster_params(tolerance=-1.0, min_size=5, max_size=4, reserved_=1))
    assert rc == INV and b"tolerance" in _err(L)
    rc, _ = _cluster(L, capi.default_cluster_params(min_size=5, max_size=4, reserved_=1))
    assert rc == INV and b"min_size" in _err(L)
    every = dict(ror_radius=-1.0, cluster_min_size=3, cluster_max_size=2, sor_mean_k=16, sor_std_mul=NAN, cluster_reserved_=1, min_range=5.0, max_range=4.0)
    for key, word, mended in (("ror_radius", b"ror_radius", 0.5), ("cluster_max_size", b"min_size", 0), ("sor_mean_k", b"sor_mean_k", 4),
                              ("sor_std_mul", b"sor_std_mul", 1.0), ("cluster_reserved_", b"reserved_", 0), ("min_range", b"min_range", 0.0)):
        rc, untouched = _filtered(L, capi.default_scan_filter_params(**every))
        assert rc == INV and word in _err(L) and untouched, word
        every[key] = mended                                # ... and the next fault in line shows
    rc, _ = _filtered(L, capi.default_scan_filter_params(**every))
    assert rc == INV and b"null" in _err(L)


def test_the_edges_of_the_ranges_are_inside(capi):
    """What the parameter check lets through is refused for the null handle."""
    L = capi.lib()
    for over in (dict(min_size=0), dict(min_size=4, max_size=4), dict(min_size=9, max_size=0), dict(tolerance=1e-30), dict(tolerance=3e38)):
        rc, untouched = _cluster(L, capi.default_cluster_params(**over))
        assert rc == INV and b"null store" in _err(L) and untouched
    for over in (dict(), dict(sor_mean_k=15), dict(sor_mean_k=1, sor_std_mul=-2.0), dict(min_range=4.0, max_range=4.0), dict(min_range=5.0),
                 dict(min_range=5.0, max_range=-1.0), dict(ror_radius=0.5, ror_min_neighbors=4000000000), dict(cluster_tolerance=0.5, cluster_min_size=0)):
        rc, untouched = _filtered(L, capi.default_scan_filter_params(**over))
        assert rc == INV and b"null" in _err(L) and untouched
    prm = capi.default_scan_filter_params()
    assert L.gloc_scan_store_add_filtered(None, 0, C.byref(prm), None, None) == INV and b"null" in _err(L)


def test_subset_refusals_before_the_handle(capi):
    L = capi.lib()
    idx, sid = np.zeros(3, np.uint32), C.c_uint32(7)
    ip, sp = idx.ctypes.data_as(C.c_void_p), C.cast(C.pointer(sid), C.c_void_p)
    assert L.gloc_scan_store_add_subset(None, 0, None, 3, sp) == INV and b"null" in _err(L)
    assert L.gloc_scan_store_add_subset(None, 0, ip, 3, None) == INV and b"null" in _err(L)
    assert L.gloc_scan_store_add_subset(None, 0, ip, 0, sp) == INV and b"0 rows" in _err(L)
    assert L.gloc_scan_store_add_subset(None, 0, ip, 1 << 31, sp) == INV and b"rows" in _err(L)
    assert L.gloc_scan_store_add_subset(None, 0, ip, 3, sp) == INV and b"null store" in _err(L)
    assert sid.value == 7
