"""CPU: the point-to-plane additions to the C ABI -- exported symbols, documented defaults, error codes that need no
device."""
import ctypes as C


def test_p2l_symbols_exported(capi):
    L = capi.lib()
    for name in ("gloc_scan_store_build_normals", "gloc_scan_store_normals", "gloc_p2l_default_params",
                 "gloc_reg_p2l_batch_ids", "gloc_reg_p2l_system"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS, name
    for name in ("p2l_batch", "p2l_system"):
        assert callable(getattr(capi.Registrar, name))
    for name in ("build_normals", "normals"):
        assert callable(getattr(capi.ScanStore, name))


def test_p2l_default_params(capi):
    p = capi.default_p2l_params()
    assert p.max_iters == 30                      # registration/global_registration.cpp:242
    assert p.max_corr_dist == 0.0                 # no rejection
    assert p.trans_eps == 0.0 and p.rot_eps == 0.0
    assert p.normal_k == 10                       # registration/ground_estimator.cpp:79
    assert p.reserved_ == 0
    assert C.sizeof(capi.P2lParams) == 24
    q = capi.default_p2l_params(max_iters=5, trans_eps=1e-4)
    assert q.max_iters == 5 and q.trans_eps == C.c_float(1e-4).value and q.normal_k == 10
    capi.lib().gloc_p2l_default_params(None)      # a null pointer is ignored


def test_p2l_null_arguments_and_bad_k(capi):
    L = capi.lib()
    prm = capi.default_p2l_params()
    INVALID = 1
    assert L.gloc_scan_store_build_normals(None, 0, 10) == INVALID
    assert b"null" in L.gloc_last_error()
    for k in (0, 2, 17):
        assert L.gloc_scan_store_build_normals(None, 0, k) == INVALID
        assert b"outside [3, 16]" in L.gloc_last_error()
    bad = capi.default_p2l_params(normal_k=2)
    assert bad.normal_k == 2                      # (refused by the call, on the device: tests/test_p2l_gpu.py)
    buf = (C.c_float * 3)()
    assert L.gloc_scan_store_normals(None, 0, buf, 1) == INVALID
    T = (C.c_float * 16)()
    ids = (C.c_uint32 * 1)(0)
    assert L.gloc_reg_p2l_batch_ids(None, 0, ids, 1, None, C.byref(prm), T, None, None, None) == INVALID
    H, g, s, c = (C.c_double * 36)(), (C.c_double * 6)(), C.c_double(), C.c_uint64()
    assert L.gloc_reg_p2l_system(None, 0, 0, None, C.byref(prm), H, g, C.byref(s), C.byref(c)) == INVALID
