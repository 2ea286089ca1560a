"""CPU: the voxelized generalized ICP additions to the C ABI -- exported symbols, documented defaults, error codes that
need no device."""
import ctypes as C


def test_vgicp_symbols_exported(capi):
    L = capi.lib()
    for name in ("gloc_vgicp_default_params", "gloc_reg_vgicp_batch_ids", "gloc_reg_vgicp_system", "gloc_reg_vgicp_voxels"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS, name
    for name in ("vgicp_batch", "vgicp_system", "vgicp_voxels"):
        assert callable(getattr(capi.Registrar, name))
    assert L.gloc_abi_version() == 6              # symbols are only added


def test_vgicp_default_params(capi):
    p = capi.default_vgicp_params()
    assert p.max_iters == 30
    assert p.max_corr_dist == 0.0                 # no rejection
    assert p.trans_eps == 0.0 and p.rot_eps == 0.0
    assert p.normal_k == 10
    assert p.plane_eps == C.c_float(1e-3).value
    assert p.resolution == 1.0                    # fast_gicp's voxel resolution
    assert p.neighbors == 7 and p.min_points == 1 and p.reserved_ == 0
    assert C.sizeof(capi.VgicpParams) == 40
    q = capi.default_vgicp_params(max_iters=5, resolution=0.5, neighbors=27)
    assert q.max_iters == 5 and q.resolution == 0.5 and q.neighbors == 27 and q.normal_k == 10
    capi.lib().gloc_vgicp_default_params(None)    # a null pointer is ignored


def test_vgicp_null_arguments_and_bad_parameters(capi):
    L = capi.lib()
    INVALID = 1
    T = (C.c_float * 16)()
    ids = (C.c_uint32 * 1)(0)
    H, g, s, c = (C.c_double * 36)(), (C.c_double * 6)(), C.c_double(), C.c_uint64()
    nv = C.c_size_t()

    def every(prm):
        a = L.gloc_reg_vgicp_batch_ids(None, 0, ids, 1, None, prm, T, None, None, None)
        ea = L.gloc_last_error()
        b = L.gloc_reg_vgicp_system(None, 0, 0, None, prm, H, g, C.byref(s), C.byref(c))
        eb = L.gloc_last_error()
        v = L.gloc_reg_vgicp_voxels(None, 0, prm, 0, None, None, None, None, C.byref(nv))
        return (a, b, v), (ea, eb, L.gloc_last_error())

    def refused(prm, word):
        codes, errs = every(prm)
        assert codes == (INVALID,) * 3, (word, codes)
        assert all(word in e for e in errs), (word, errs)

    refused(C.byref(capi.default_vgicp_params()), b"null")          # a null handle
    refused(None, b"null")                                          # null params
    # a bad parameter block is refused for what it is, whatever the handle
    for k in (0, 2, 17):
        refused(C.byref(capi.default_vgicp_params(normal_k=k)), b"normal_k")
    for e in (0.0, -1e-3, 1.0001, float("nan")):
        refused(C.byref(capi.default_vgicp_params(plane_eps=e)), b"plane_eps")
    refused(C.byref(capi.default_vgicp_params(max_iters=0)), b"max_iters")
    for r in (0.0, -1.0, float("nan"), float("inf")):
        refused(C.byref(capi.default_vgicp_params(resolution=r)), b"resolution")
    for n in (0, 2, 6, 8, 26, 28):
        refused(C.byref(capi.default_vgicp_params(neighbors=n)), b"neighbors")
    refused(C.byref(capi.default_vgicp_params(min_points=0)), b"min_points")
    for ok in (dict(plane_eps=1.0), dict(neighbors=1), dict(neighbors=27), dict(min_points=3, resolution=0.25)):
        refused(C.byref(capi.default_vgicp_params(**ok)), b"null")   # allowed: the handle is what is missing
