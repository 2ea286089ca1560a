"""CPU: the C ABI of the Fast Global Registration -- symbols, defaults, struct size, refusals."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gloc_fgr_default_params", "gloc_reg_fpfh_fgr_batch_ids", "gloc_reg_fpfh_fgr_batch_ids_radius", "gloc_reg_fpfh_fgr_batch_ids_keypoints",
       "gloc_reg_fgr_pairs")


def test_symbols_exported(capi):
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.gloc_abi_version() == 6


def test_defaults_and_size(capi):
    p = capi.default_fgr_params()
    assert (p.normal_k, p.feature_k, p.mutual, p.tuple_tries, p.max_tuples, p.max_iters, p.anneal_every, p.seed) == (10, 16, 1, 10000, 1000, 64, 4, 1234)
    assert p.tuple_scale == np.float32(0.9) and p.anneal_div == np.float32(1.4) and p.max_corr_dist == np.float32(0.6)
    assert p.inlier_thresh == np.float32(0.6) and p.min_inlier_ratio == 0.0
    assert C.sizeof(capi.FgrParams) == 56 and capi.FgrParams.seed.offset == 48
    assert capi.default_fgr_params(max_iters=8).max_iters == 8
    capi.lib().gloc_fgr_default_params(None)                    # a null block is ignored


BAD = [("normal_k", 2), ("normal_k", 17), ("feature_k", 3), ("feature_k", 17), ("tuple_tries", (1 << 20) + 1), ("max_tuples", 0),
       ("max_tuples", (1 << 20) + 1), ("tuple_scale", 0.0), ("tuple_scale", 1.5), ("tuple_scale", float("nan")), ("max_iters", 0),
       ("max_iters", 1025), ("anneal_every", 0), ("anneal_div", 1.0), ("anneal_div", float("nan")), ("anneal_div", float("inf")),
       ("max_corr_dist", 0.0), ("max_corr_dist", float("nan")), ("inlier_thresh", -1.0), ("inlier_thresh", float("nan"))]


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("field,value", BAD)
def test_bad_params_are_refused_before_the_handle(capi, field, value):
    L = capi.lib()
    L.gloc_last_error.restype = C.c_char_p
    prm = capi.default_fgr_params(**{field: value})
    support, iss = capi.default_fpfh_radius_params(), capi.default_iss_params()
    T = np.empty(16, np.float32)
    ids = np.zeros(1, np.uint32)
    P = np.zeros((4, 3), np.float32)
    word = field.encode()
    rc = L.gloc_reg_fpfh_fgr_batch_ids(None, 0, _ptr(ids), 1, None, C.byref(prm), _ptr(T), None, None, None)
    assert rc == 1 and word in L.gloc_last_error()                                   # GLOC_ERR_INVALID, naming the field
    rc = L.gloc_reg_fpfh_fgr_batch_ids_radius(None, 0, _ptr(ids), 1, None, C.byref(prm), C.byref(support), _ptr(T), None, None, None)
    assert rc == 1 and word in L.gloc_last_error()
    rc = L.gloc_reg_fpfh_fgr_batch_ids_keypoints(None, 0, _ptr(ids), 1, None, C.byref(prm), None, C.byref(iss), _ptr(T), None, None, None)
    assert rc == 1 and word in L.gloc_last_error()
    rc = L.gloc_reg_fgr_pairs(None, _ptr(P), _ptr(P), 4, 0, C.byref(prm), None, None, None, None, _ptr(T), None, None, None)
    assert rc == 1 and word in L.gloc_last_error()


def test_null_arguments(capi):
    L = capi.lib()
    L.gloc_last_error.restype = C.c_char_p
    T = np.empty(16, np.float32)
    ids = np.zeros(1, np.uint32)
    prm = capi.default_fgr_params()
    support, iss = capi.default_fpfh_radius_params(), capi.default_iss_params()
    assert L.gloc_reg_fpfh_fgr_batch_ids(None, 0, _ptr(ids), 1, None, None, _ptr(T), None, None, None) != 0
    assert b"params" in L.gloc_last_error()
    assert L.gloc_reg_fpfh_fgr_batch_ids(None, 0, _ptr(ids), 1, None, C.byref(prm), _ptr(T), None, None, None) != 0
    assert b"null" in L.gloc_last_error()
    assert L.gloc_reg_fpfh_fgr_batch_ids_radius(None, 0, _ptr(ids), 1, None, C.byref(prm), None, _ptr(T), None, None, None) != 0
    assert L.gloc_reg_fpfh_fgr_batch_ids_radius(None, 0, _ptr(ids), 1, None, C.byref(prm), C.byref(support), _ptr(T), None, None, None) != 0
    assert b"null" in L.gloc_last_error()
    assert L.gloc_reg_fpfh_fgr_batch_ids_keypoints(None, 0, _ptr(ids), 1, None, C.byref(prm), None, None, _ptr(T), None, None, None) != 0
    assert L.gloc_reg_fpfh_fgr_batch_ids_keypoints(None, 0, _ptr(ids), 1, None, C.byref(prm), None, C.byref(iss), _ptr(T), None, None, None) != 0
    assert b"null" in L.gloc_last_error()
    assert L.gloc_reg_fgr_pairs(None, None, None, 0, 0, None, None, None, None, None, _ptr(T), None, None, None) != 0
    assert b"params" in L.gloc_last_error()
    assert L.gloc_reg_fgr_pairs(None, None, None, 0, 0, C.byref(prm), None, None, None, None, _ptr(T), None, None, None) != 0
    assert b"null" in L.gloc_last_error()
