"""CPU: the C ABI of the ISS keypoints -- symbols, defaults, struct size, refusals before the handle."""
import ctypes as C

import numpy as np
import pytest

NEW = ("gloc_iss_default_params", "gloc_scan_store_iss_saliency", "gloc_scan_store_build_keypoints", "gloc_scan_store_keypoint_count",
       "gloc_scan_store_keypoints", "gloc_scan_store_keypoint_fpfh", "gloc_reg_fpfh_batch_ids_keypoints",
       "gloc_reg_fpfh_graph_batch_ids_keypoints")
INV = 1                 # GLOC_ERR_INVALID (include/gloc3d.h)
BAD = [("salient_radius", 0.0), ("salient_radius", -1.0), ("salient_radius", float("nan")), ("salient_radius", float("inf")),
       ("non_max_radius", 0.0), ("non_max_radius", -2.0), ("non_max_radius", float("nan")), ("non_max_radius", float("inf")),
       ("max_nn", 0), ("max_nn", 129), ("max_nn", 4), ("min_nn", 2), ("min_nn", 129),
       ("gamma_21", 0.0), ("gamma_21", -0.5), ("gamma_21", 1.5), ("gamma_21", float("nan")),
       ("gamma_32", 0.0), ("gamma_32", 1.0000001), ("gamma_32", float("nan"))]


def _err(L):
    L.gloc_last_error.restype = C.c_char_p
    return L.gloc_last_error()


def _bufs():
    T, ids = np.empty(16, np.float32), np.zeros(1, np.uint32)
    return T.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), (T, ids)


def test_symbols_exported(capi):
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED_SYMBOLS and hasattr(L, name)
    assert L.gloc_abi_version() == 6


def test_defaults_and_size(capi):
    p = capi.default_iss_params()
    assert (p.salient_radius, p.max_nn, p.min_nn, p.non_max_radius) == (3.0, 128, 5, 2.0)
    assert p.gamma_21 == np.float32(0.975) and p.gamma_32 == np.float32(0.975)
    assert C.sizeof(capi.IssParams) == 24 and capi.IssParams.non_max_radius.offset == 12 and capi.IssParams.gamma_32.offset == 20
    assert capi.default_iss_params(max_nn=64).max_nn == 64
    capi.lib().gloc_iss_default_params(None)               # a null block is ignored


def test_the_edges_of_the_ranges_are_inside(capi):
    """min_nn = 3, min_nn = max_nn, max_nn = 128 and gamma = 1 pass the parameter check: the refusal is then the null handle's."""
    L = capi.lib()
    for over in (dict(min_nn=3), dict(min_nn=128), dict(max_nn=5), dict(max_nn=3, min_nn=3), dict(gamma_21=1.0, gamma_32=1.0)):
        iss = capi.default_iss_params(**over)
        assert L.gloc_scan_store_build_keypoints(None, 0, C.byref(iss)) == INV and b"null" in _err(L)


@pytest.mark.parametrize("field,value", BAD)
def test_bad_parameters_are_refused_before_the_handle(capi, field, value):
    L = capi.lib()
    iss = capi.default_iss_params(**{field: value})
    tp, ip, _keep = _bufs()
    # (max_nn below min_nn is told about min_nn, the field whose range depends on the other)
    name = b"min_nn" if (field, value) == ("max_nn", 4) else field.encode()
    prm, gprm, sup = capi.default_fpfh_params(), capi.default_fpfh_graph_params(), capi.default_fpfh_radius_params()
    assert L.gloc_scan_store_build_keypoints(None, 0, C.byref(iss)) == INV and name in _err(L)
    assert L.gloc_scan_store_iss_saliency(None, 0, C.byref(iss), None, None, 0) == INV and name in _err(L)
    for s in (None, C.byref(sup)):
        assert L.gloc_reg_fpfh_batch_ids_keypoints(None, 0, ip, 1, None, C.byref(prm), s, C.byref(iss), tp, None, None, None) == INV
        assert name in _err(L)
        assert L.gloc_reg_fpfh_graph_batch_ids_keypoints(None, 0, ip, 1, C.byref(gprm), s, C.byref(iss), tp, None, None, None) == INV
        assert name in _err(L)


def test_the_other_blocks_are_still_checked(capi):
    L = capi.lib()
    tp, ip, _keep = _bufs()
    iss = capi.default_iss_params()
    prm = capi.default_fpfh_params(feature_k=17)
    assert L.gloc_reg_fpfh_batch_ids_keypoints(None, 0, ip, 1, None, C.byref(prm), None, C.byref(iss), tp, None, None, None) == INV
    assert b"feature_k" in _err(L)
    gprm = capi.default_fpfh_graph_params(n_seeds=0)
    assert L.gloc_reg_fpfh_graph_batch_ids_keypoints(None, 0, ip, 1, C.byref(gprm), None, C.byref(iss), tp, None, None, None) == INV
    sup = capi.default_fpfh_radius_params(feature_max_nn=129)
    prm, gprm = capi.default_fpfh_params(), capi.default_fpfh_graph_params()
    assert L.gloc_reg_fpfh_batch_ids_keypoints(None, 0, ip, 1, None, C.byref(prm), C.byref(sup), C.byref(iss), tp, None, None, None) == INV
    assert b"feature_max_nn" in _err(L)
    assert L.gloc_reg_fpfh_graph_batch_ids_keypoints(None, 0, ip, 1, C.byref(gprm), C.byref(sup), C.byref(iss), tp, None, None, None) == INV
    assert b"feature_max_nn" in _err(L)


def test_null_arguments(capi):
    L = capi.lib()
    tp, ip, _keep = _bufs()
    prm, gprm, iss = capi.default_fpfh_params(), capi.default_fpfh_graph_params(), capi.default_iss_params()
    k = C.c_size_t(0)
    # a null keypoint block, then a null handle behind good blocks
    assert L.gloc_scan_store_build_keypoints(None, 0, None) == INV and b"params" in _err(L)
    assert L.gloc_scan_store_iss_saliency(None, 0, None, None, None, 0) == INV and b"params" in _err(L)
    assert L.gloc_reg_fpfh_batch_ids_keypoints(None, 0, ip, 1, None, C.byref(prm), None, None, tp, None, None, None) == INV and b"params" in _err(L)
    assert L.gloc_reg_fpfh_graph_batch_ids_keypoints(None, 0, ip, 1, C.byref(gprm), None, None, tp, None, None, None) == INV and b"params" in _err(L)
    assert L.gloc_reg_fpfh_batch_ids_keypoints(None, 0, ip, 1, None, None, None, C.byref(iss), tp, None, None, None) == INV and b"params" in _err(L)
    assert L.gloc_scan_store_build_keypoints(None, 0, C.byref(iss)) == INV and b"null" in _err(L)
    assert L.gloc_scan_store_iss_saliency(None, 0, C.byref(iss), None, None, 0) == INV and b"null" in _err(L)
    assert L.gloc_scan_store_keypoint_count(None, 0, C.byref(k)) == INV and b"null" in _err(L)
    assert L.gloc_scan_store_keypoints(None, 0, None, 0) == INV and b"null" in _err(L)
    assert L.gloc_scan_store_keypoint_fpfh(None, 0, None, 0) == INV and b"null" in _err(L)
    assert L.gloc_reg_fpfh_batch_ids_keypoints(None, 0, ip, 1, None, C.byref(prm), None, C.byref(iss), tp, None, None, None) == INV
    assert b"null" in _err(L)
    assert L.gloc_reg_fpfh_graph_batch_ids_keypoints(None, 0, ip, 1, C.byref(gprm), None, C.byref(iss), tp, None, None, None) == INV
    assert b"null" in _err(L)
