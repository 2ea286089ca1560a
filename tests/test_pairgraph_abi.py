"""CPU: the C ABI of the correspondence-graph global registration -- symbols, defaults, struct size, refusals."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gloc_fpfh_graph_default_params", "gloc_reg_fpfh_graph_batch_ids", "gloc_reg_pair_graph")


def test_symbols_exported(capi):
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.gloc_abi_version() == 6


def test_defaults_and_size(capi):
    p = capi.default_fpfh_graph_params()
    assert (p.normal_k, p.feature_k, p.mutual, p.n_seeds, p.theta_num, p.theta_den, p.reserved_) == (10, 16, 1, 64, 1, 2, 0)
    assert p.compat_thresh == np.float32(0.6) and p.inlier_thresh == np.float32(0.6) and p.min_inlier_ratio == 0.0
    assert C.sizeof(capi.FpfhGraphParams) == 40 and capi.FpfhGraphParams.reserved_.offset == 36
    assert capi.default_fpfh_graph_params(n_seeds=8).n_seeds == 8
    capi.lib().gloc_fpfh_graph_default_params(None)             # a null block is ignored
    assert capi.REG_OPT_PAIRGRAPH_BUDGET == 12


BAD = [("normal_k", 2), ("normal_k", 17), ("feature_k", 3), ("feature_k", 17), ("n_seeds", 0), ("n_seeds", 1025), ("compat_thresh", 0.0),
       ("compat_thresh", float("nan")), ("inlier_thresh", -1.0), ("theta_num", 0), ("theta_num", 3), ("theta_den", 0)]


@pytest.mark.parametrize("field,value", BAD)
def test_bad_params_are_refused_before_the_handle(capi, field, value):
    L = capi.lib()
    L.gloc_last_error.restype = C.c_char_p
    prm = capi.default_fpfh_graph_params(**{field: value})
    T = np.empty(16, np.float32)
    ids = np.zeros(1, np.uint32)
    P = np.zeros((4, 3), np.float32)
    word = field.split("_")[0].encode() if field.startswith("theta") else field.encode()
    rc = L.gloc_reg_fpfh_graph_batch_ids(None, 0, ids.ctypes.data_as(C.c_void_p), 1, C.byref(prm), T.ctypes.data_as(C.c_void_p), None, None, None)
    assert rc == 1 and word in L.gloc_last_error()                                   # GLOC_ERR_INVALID, naming the field
    rc = L.gloc_reg_pair_graph(None, P.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p), 4, C.byref(prm), None, None, None, None, None,
                               T.ctypes.data_as(C.c_void_p), None, None, None)
    assert rc == 1 and word in L.gloc_last_error()


def test_null_arguments(capi):
    L = capi.lib()
    L.gloc_last_error.restype = C.c_char_p
    T = np.empty(16, np.float32)
    ids = np.zeros(1, np.uint32)
    prm = capi.default_fpfh_graph_params()
    assert L.gloc_reg_fpfh_graph_batch_ids(None, 0, ids.ctypes.data_as(C.c_void_p), 1, None, T.ctypes.data_as(C.c_void_p), None, None, None) != 0
    assert b"params" in L.gloc_last_error()
    assert L.gloc_reg_fpfh_graph_batch_ids(None, 0, ids.ctypes.data_as(C.c_void_p), 1, C.byref(prm), T.ctypes.data_as(C.c_void_p), None, None, None) != 0
    assert b"null" in L.gloc_last_error()
    assert L.gloc_reg_pair_graph(None, None, None, 0, None, None, None, None, None, None, None, None, None, None) != 0
    assert b"params" in L.gloc_last_error()
    assert L.gloc_reg_pair_graph(None, None, None, 0, C.byref(prm), None, None, None, None, None, None, None, None, None) != 0
    assert b"null" in L.gloc_last_error()
