"""CPU: the generalized ICP additions to the C ABI -- exported symbols, documented defaults, error codes that need no
device."""
import ctypes as C


def test_gicp_symbols_exported(capi):
    L = capi.lib()
    for name in ("gloc_gicp_default_params", "gloc_reg_gicp_batch_ids", "gloc_reg_gicp_system"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS, name
    for name in ("gicp_batch", "gicp_system"):
        assert callable(getattr(capi.Registrar, name))
    assert L.gloc_abi_version() == 6              # symbols are only added


def test_gicp_default_params(capi):
    p = capi.default_gicp_params()
    assert p.max_iters == 30                      # registration/global_registration.cpp:242
    assert p.max_corr_dist == 0.0                 # no rejection
    assert p.trans_eps == 0.0 and p.rot_eps == 0.0
    assert p.normal_k == 10                       # registration/ground_estimator.cpp:79
    assert p.plane_eps == C.c_float(1e-3).value   # pcl::GeneralizedIterativeClosestPoint's gicp_epsilon_
    assert C.sizeof(capi.GicpParams) == 24
    q = capi.default_gicp_params(max_iters=5, plane_eps=0.5)
    assert q.max_iters == 5 and q.plane_eps == 0.5 and q.normal_k == 10
    capi.lib().gloc_gicp_default_params(None)     # a null pointer is ignored


def test_gicp_null_arguments_bad_k_and_bad_plane_eps(capi):
    L = capi.lib()
    INVALID = 1
    T = (C.c_float * 16)()
    ids = (C.c_uint32 * 1)(0)
    H, g, s, c = (C.c_double * 36)(), (C.c_double * 6)(), C.c_double(), C.c_uint64()

    def both(prm):
        a = L.gloc_reg_gicp_batch_ids(None, 0, ids, 1, None, prm, T, None, None, None)
        ea = L.gloc_last_error()
        b = L.gloc_reg_gicp_system(None, 0, 0, None, prm, H, g, C.byref(s), C.byref(c))
        return a, b, ea, L.gloc_last_error()

    a, b, ea, eb = both(C.byref(capi.default_gicp_params()))
    assert a == INVALID and b == INVALID and b"null" in ea and b"null" in eb        # a null handle
    a, b, ea, eb = both(None)
    assert a == INVALID and b == INVALID and b"null" in ea and b"null" in eb        # null params
    # a bad parameter block is refused for what it is, whatever the handle
    for k in (0, 2, 17):
        a, b, ea, eb = both(C.byref(capi.default_gicp_params(normal_k=k)))
        assert a == INVALID and b == INVALID and b"normal_k" in ea and b"normal_k" in eb, k
    for e in (0.0, -1e-3, 1.0001, float("nan")):
        a, b, ea, eb = both(C.byref(capi.default_gicp_params(plane_eps=e)))
        assert a == INVALID and b == INVALID and b"plane_eps" in ea and b"plane_eps" in eb, e
    a, b, ea, eb = both(C.byref(capi.default_gicp_params(max_iters=0)))
    assert a == INVALID and b == INVALID and b"max_iters" in ea
    a, _, ea, _ = both(C.byref(capi.default_gicp_params(plane_eps=1.0)))                # 1 is allowed: the handle is what is missing
    assert a == INVALID and b"null" in ea
