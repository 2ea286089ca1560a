"""CPU: the C ABI of the radius-support FPFH -- symbols, defaults, struct size, refusals before the handle."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gloc_fpfh_radius_default_params", "gloc_scan_store_radius_neighbors", "gloc_scan_store_build_normals_radius",
       "gloc_scan_store_build_fpfh_radius", "gloc_scan_store_spfh_radius", "gloc_reg_fpfh_batch_ids_radius",
       "gloc_reg_fpfh_graph_batch_ids_radius")
INV, STATE = 1, 5       # GLOC_ERR_INVALID, GLOC_ERR_STATE (include/gloc3d.h)
BAD = [("normal_radius", 0.0), ("normal_radius", -1.0), ("normal_radius", float("nan")), ("normal_radius", float("inf")),
       ("feature_radius", 0.0), ("feature_radius", float("nan")), ("feature_radius", float("inf")), ("normal_max_nn", 129),
       ("normal_max_nn", 4), ("normal_min_nn", 3), ("normal_min_nn", 31), ("feature_max_nn", 3), ("feature_max_nn", 129), ("reserved_", 1)]


def _err(L):
    L.gloc_last_error.restype = C.c_char_p
    return L.gloc_last_error()


def test_symbols_exported(capi):
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.gloc_abi_version() == 6


def test_defaults_and_size(capi):
    p = capi.default_fpfh_radius_params()
    assert (p.normal_radius, p.normal_max_nn, p.normal_min_nn, p.feature_radius, p.feature_max_nn, p.reserved_) == (1.0, 30, 5, 2.5, 100, 0)
    assert C.sizeof(capi.FpfhRadiusParams) == 24 and capi.FpfhRadiusParams.feature_radius.offset == 12
    assert capi.default_fpfh_radius_params(feature_max_nn=64).feature_max_nn == 64
    capi.lib().gloc_fpfh_radius_default_params(None)       # a null block is ignored


@pytest.mark.parametrize("field,value", BAD)
def test_bad_supports_are_refused_before_the_handle(capi, field, value):
    L = capi.lib()
    sup = capi.default_fpfh_radius_params(**{field: value})
    T, ids = np.empty(16, np.float32), np.zeros(1, np.uint32)
    tp, ip = T.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p)
    name = field.encode()
    assert L.gloc_scan_store_build_fpfh_radius(None, 0, C.byref(sup)) == INV and name in _err(L)
    prm = capi.default_fpfh_params()
    assert L.gloc_reg_fpfh_batch_ids_radius(None, 0, ip, 1, None, C.byref(prm), C.byref(sup), tp, None, None, None) == INV
    assert name in _err(L)
    gprm = capi.default_fpfh_graph_params()
    assert L.gloc_reg_fpfh_graph_batch_ids_radius(None, 0, ip, 1, C.byref(gprm), C.byref(sup), tp, None, None, None) == INV
    assert name in _err(L)


def test_the_k_blocks_are_still_checked(capi):
    L = capi.lib()
    sup = capi.default_fpfh_radius_params()
    T, ids = np.empty(16, np.float32), np.zeros(1, np.uint32)
    tp, ip = T.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p)
    prm = capi.default_fpfh_params(feature_k=17)
    assert L.gloc_reg_fpfh_batch_ids_radius(None, 0, ip, 1, None, C.byref(prm), C.byref(sup), tp, None, None, None) == INV
    assert b"feature_k" in _err(L)
    gprm = capi.default_fpfh_graph_params(n_seeds=0)
    assert L.gloc_reg_fpfh_graph_batch_ids_radius(None, 0, ip, 1, C.byref(gprm), C.byref(sup), tp, None, None, None) == INV


def test_null_arguments_and_scalar_ranges(capi):
    L = capi.lib()
    T, ids = np.empty(16, np.float32), np.zeros(1, np.uint32)
    tp, ip = T.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p)
    prm, gprm, sup = capi.default_fpfh_params(), capi.default_fpfh_graph_params(), capi.default_fpfh_radius_params()
    # null blocks, then a null handle behind good blocks
    assert L.gloc_scan_store_build_fpfh_radius(None, 0, None) == INV and b"params" in _err(L)
    assert L.gloc_reg_fpfh_batch_ids_radius(None, 0, ip, 1, None, C.byref(prm), None, tp, None, None, None) == INV and b"params" in _err(L)
    assert L.gloc_reg_fpfh_batch_ids_radius(None, 0, ip, 1, None, None, C.byref(sup), tp, None, None, None) == INV and b"params" in _err(L)
    assert L.gloc_reg_fpfh_graph_batch_ids_radius(None, 0, ip, 1, C.byref(gprm), None, tp, None, None, None) == INV and b"params" in _err(L)
    assert L.gloc_reg_fpfh_graph_batch_ids_radius(None, 0, ip, 1, None, C.byref(sup), tp, None, None, None) == INV
    assert L.gloc_scan_store_build_fpfh_radius(None, 0, C.byref(sup)) == INV and b"null" in _err(L)
    assert L.gloc_reg_fpfh_batch_ids_radius(None, 0, ip, 1, None, C.byref(prm), C.byref(sup), tp, None, None, None) == INV and b"null" in _err(L)
    assert L.gloc_reg_fpfh_graph_batch_ids_radius(None, 0, ip, 1, C.byref(gprm), C.byref(sup), tp, None, None, None) == INV and b"null" in _err(L)
    # the scalar entries: ranges before the handle
    for r in (0.0, -2.0, float("nan"), float("inf")):
        assert L.gloc_scan_store_radius_neighbors(None, 0, r, 16, None, None, None, 0) == INV and b"radius" in _err(L)
        assert L.gloc_scan_store_build_normals_radius(None, 0, r, 30, 5) == INV and b"radius" in _err(L)
        assert L.gloc_scan_store_spfh_radius(None, 0, r, 100, None, None, 0) == INV and b"radius" in _err(L)
    for m in (0, 129):
        assert L.gloc_scan_store_radius_neighbors(None, 0, 1.0, m, None, None, None, 0) == INV and b"max_nn" in _err(L)
    for m in (3, 129):
        assert L.gloc_scan_store_spfh_radius(None, 0, 1.0, m, None, None, 0) == INV and b"max_nn" in _err(L)
    assert L.gloc_scan_store_build_normals_radius(None, 0, 1.0, 129, 5) == INV and b"max_nn" in _err(L)
    assert L.gloc_scan_store_build_normals_radius(None, 0, 1.0, 30, 3) == INV and b"min_nn" in _err(L)
    assert L.gloc_scan_store_build_normals_radius(None, 0, 1.0, 30, 31) == INV and b"min_nn" in _err(L)
    assert L.gloc_scan_store_radius_neighbors(None, 0, 1.0, 16, None, None, None, 0) == INV and b"null" in _err(L)
    assert L.gloc_scan_store_build_normals_radius(None, 0, 1.0, 30, 5) == INV and b"null" in _err(L)
    assert L.gloc_scan_store_spfh_radius(None, 0, 1.0, 100, None, None, 0) == INV and b"null" in _err(L)
