"""CPU: the local-submap additions to the C ABI -- symbols, wrappers, default parameters, no CPU fallback."""
import ctypes as C


def test_submap_symbols_exported(capi):
    L = capi.lib()
    for name in ("gloc_submap_default_params", "gloc_scan_store_add_submap", "gloc_scan_store_add_submaps",
                 "gloc_reg_scan_add_submaps"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS, name
    for name in ("add_submap", "add_submaps"):
        assert callable(getattr(capi.ScanStore, name))
    assert callable(capi.Registrar.scan_add_submaps)
    assert callable(capi.default_submap_params)
    assert [n for n, _ in capi.SubmapInfo._fields_] == ["points_in", "points_used", "cells", "kept"]


def test_submap_default_params(capi):
    p = capi.default_submap_params()
    assert (p.leaf, p.min_points, p.min_scans, p.max_range, p.group_points) == (C.c_float(0.2).value, 1, 1, 0.0, 0)
    q = capi.default_submap_params(leaf=0.5, min_scans=2)
    assert q.leaf == 0.5 and q.min_scans == 2 and q.min_points == 1
    assert C.sizeof(capi.SubmapParams) == 20 and C.sizeof(capi.SubmapInfo) == 24


def test_submap_calls_refuse_a_null_store(capi):
    L = capi.lib()
    prm = capi.default_submap_params()
    ids, T = (C.c_uint32 * 1)(0), (C.c_float * 16)(*([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]))
    first, new = (C.c_uint32 * 2)(0, 1), C.c_uint32()
    assert L.gloc_scan_store_add_submap(None, ids, T, 1, C.byref(prm), C.byref(new), None) == 1
    assert L.gloc_scan_store_add_submaps(None, ids, T, first, 1, C.byref(prm), C.byref(new), None) == 1
    assert L.gloc_reg_scan_add_submaps(None, ids, T, first, 1, C.byref(prm), C.byref(new), None) == 1
    assert b"null" in L.gloc_last_error()


def test_abi_version_unchanged(capi):
    assert capi.lib().gloc_abi_version() == 6
