"""CPU: the C ABI of the FPFH feature-based global registration -- symbols, defaults, struct size, refusals."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gloc_fpfh_default_params", "gloc_scan_store_build_fpfh", "gloc_scan_store_fpfh", "gloc_scan_store_spfh", "gloc_reg_fpfh_match",
       "gloc_reg_fpfh_batch_ids")


def test_symbols_exported(capi):
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.gloc_abi_version() == 6


def test_defaults_and_size(capi):
    p = capi.default_fpfh_params()
    assert (p.normal_k, p.feature_k, p.mutual, p.ransac_iters, p.seed) == (10, 16, 1, 3000, 1234)
    assert p.inlier_thresh == np.float32(0.6) and p.min_inlier_ratio == 0.0 and p.ransac_confidence == np.float32(0.99)
    assert C.sizeof(capi.FpfhParams) == 40 and capi.FpfhParams.seed.offset == 32
    assert capi.default_fpfh_params(feature_k=8).feature_k == 8
    capi.lib().gloc_fpfh_default_params(None)             # a null block is ignored


@pytest.mark.parametrize("field,value", [("normal_k", 2), ("normal_k", 17), ("feature_k", 3), ("feature_k", 17), ("ransac_iters", 0)])
def test_bad_params_are_refused_before_the_handle(capi, field, value):
    L = capi.lib()
    L.gloc_last_error.restype = C.c_char_p
    prm = capi.default_fpfh_params(**{field: value})
    T = np.empty(16, np.float32)
    ids = np.zeros(1, np.uint32)
    rc = L.gloc_reg_fpfh_batch_ids(None, 0, ids.ctypes.data_as(C.c_void_p), 1, None, C.byref(prm), T.ctypes.data_as(C.c_void_p), None, None, None)
    assert rc == capi.GLOC_ERR_INVALID if hasattr(capi, "GLOC_ERR_INVALID") else rc != 0
    assert field.encode() in L.gloc_last_error()


def test_null_arguments(capi):
    L = capi.lib()
    L.gloc_last_error.restype = C.c_char_p
    T = np.empty(16, np.float32)
    ids = np.zeros(1, np.uint32)
    prm = capi.default_fpfh_params()
    assert L.gloc_reg_fpfh_batch_ids(None, 0, ids.ctypes.data_as(C.c_void_p), 1, None, None, T.ctypes.data_as(C.c_void_p), None, None, None) != 0
    assert b"params" in L.gloc_last_error()
    assert L.gloc_reg_fpfh_batch_ids(None, 0, ids.ctypes.data_as(C.c_void_p), 1, None, C.byref(prm), T.ctypes.data_as(C.c_void_p), None, None, None) != 0
    assert L.gloc_scan_store_build_fpfh(None, 0, 10, 16) != 0
    assert L.gloc_scan_store_build_fpfh(None, 0, 2, 16) != 0 and b"normal_k" in L.gloc_last_error()
    assert L.gloc_scan_store_build_fpfh(None, 0, 10, 3) != 0 and b"feature_k" in L.gloc_last_error()
    assert L.gloc_scan_store_fpfh(None, 0, None, 0) != 0
    assert L.gloc_scan_store_spfh(None, 0, 16, None, None, 0) != 0
    assert L.gloc_reg_fpfh_match(None, None, 0, None, 0, 1, None, None) != 0
