"""CPU: the resident voxel maps' additions to the C ABI -- exported symbols, struct sizes and documented defaults, the
refusals that need no device."""
import ctypes as C

INVALID = 1
SYMBOLS = ("gloc_vmap_default_params", "gloc_reg_vmap_create", "gloc_reg_vmap_destroy", "gloc_reg_vmap_insert", "gloc_reg_vmap_prune",
           "gloc_reg_vmap_info", "gloc_reg_vmap_voxels", "gloc_reg_vgicp_vmap", "gloc_reg_vgicp_vmap_system")


def test_vmap_symbols_exported(capi):
    L = capi.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS, name
    for name in ("vmap_create", "vmap_destroy", "vmap_insert", "vmap_prune", "vmap_info", "vmap_voxels", "vgicp_vmap", "vgicp_vmap_system"):
        assert callable(getattr(capi.Registrar, name)), name
    assert L.gloc_abi_version() == 6              # symbols are only added
    from gloc3d_amd import tracking
    assert callable(tracking.ScanToMapTracker.track)


def test_vmap_struct_sizes_and_defaults(capi):
    assert C.sizeof(capi.VmapParams) == 16 and C.sizeof(capi.VmapInfo) == 24
    assert capi.VmapInfo.n_points.offset == 16 and capi.VmapInfo.resolution.offset == 12
    p = capi.default_vmap_params()
    assert p.resolution == 1.0 and p.capacity == 1 << 18 and p.normal_k == 10 and p.reserved_ == 0
    q = capi.default_vmap_params(resolution=0.5, capacity=64)
    assert q.resolution == 0.5 and q.capacity == 64 and q.normal_k == 10
    assert capi.default_vgicp_params().resolution == p.resolution and capi.default_vgicp_params().min_points == 1   # usable together
    capi.lib().gloc_vmap_default_params(None)     # a null pointer is ignored


def test_vmap_refusals_that_need_no_device(capi):
    L = capi.lib()
    mid, removed, nv = C.c_uint32(77), C.c_uint32(77), C.c_size_t(77)
    ids = (C.c_uint32 * 1)(0)
    info = capi.VmapInfo()

    def refused(rc, word):
        assert rc == INVALID and word in L.gloc_last_error(), (rc, word, L.gloc_last_error())

    ok = C.byref(capi.default_vmap_params())
    refused(L.gloc_reg_vmap_create(None, ok, C.byref(mid)), b"null")
    refused(L.gloc_reg_vmap_create(None, None, C.byref(mid)), b"null")
    # a bad parameter block is refused for what it is, whatever the handle
    for r in (0.0, -1.0, float("nan"), float("inf")):
        refused(L.gloc_reg_vmap_create(None, C.byref(capi.default_vmap_params(resolution=r)), C.byref(mid)), b"resolution")
    for c in (0, (1 << 24) + 1, 0xFFFFFFFF):
        refused(L.gloc_reg_vmap_create(None, C.byref(capi.default_vmap_params(capacity=c)), C.byref(mid)), b"capacity")
    for k in (0, 2, 17):
        refused(L.gloc_reg_vmap_create(None, C.byref(capi.default_vmap_params(normal_k=k)), C.byref(mid)), b"normal_k")
    for good in (dict(capacity=1), dict(capacity=1 << 24), dict(normal_k=3), dict(normal_k=16), dict(resolution=0.05)):
        refused(L.gloc_reg_vmap_create(None, C.byref(capi.default_vmap_params(**good)), C.byref(mid)), b"null")   # the handle is what is missing
    assert mid.value == 77                        # outputs untouched
    refused(L.gloc_reg_vmap_destroy(None, 0), b"null")
    refused(L.gloc_reg_vmap_insert(None, 0, None, 1, None), b"null")
    refused(L.gloc_reg_vmap_insert(None, 0, ids, 0, None), b"n = 0")
    refused(L.gloc_reg_vmap_insert(None, 0, ids, 1, None), b"null")
    for d in (-1.0, float("nan"), float("inf")):
        refused(L.gloc_reg_vmap_prune(None, 0, (C.c_float * 3)(), d, 0, C.byref(removed)), b"max_dist")
    refused(L.gloc_reg_vmap_prune(None, 0, None, -1.0, 0, C.byref(removed)), b"null")      # (the rule is off: its radius is not looked at)
    refused(L.gloc_reg_vmap_info(None, 0, C.byref(info)), b"null")
    refused(L.gloc_reg_vmap_info(None, 0, None), b"null")
    refused(L.gloc_reg_vmap_voxels(None, 0, 0, None, None, None, None, None, None), b"null")
    refused(L.gloc_reg_vmap_voxels(None, 0, 0, None, None, None, None, None, C.byref(nv)), b"null")
    assert removed.value == 77 and nv.value == 77

    T = (C.c_float * 16)()
    H, g, s, c = (C.c_double * 36)(), (C.c_double * 6)(), C.c_double(), C.c_uint64()

    def both(prm, word, n=1, src=ids, maps=ids):
        refused(L.gloc_reg_vgicp_vmap(None, src, maps, n, None, prm, None, T, None, None, None, None), word)
        refused(L.gloc_reg_vgicp_vmap_system(None, src, maps, n, None, prm, None, 0, H, g, C.byref(s), C.byref(c), None), word)

    both(C.byref(capi.default_vgicp_params()), b"null")
    both(None, b"null")
    both(C.byref(capi.default_vgicp_params(resolution=0.0)), b"resolution")
    both(C.byref(capi.default_vgicp_params(neighbors=6)), b"neighbors")
    both(C.byref(capi.default_vgicp_params(min_points=0)), b"min_points")
    both(C.byref(capi.default_vgicp_params()), b"n = 0", n=0)
    both(C.byref(capi.default_vgicp_params()), b"null", maps=None)
    both(C.byref(capi.default_vgicp_params()), b"null", src=None)
    refused(L.gloc_reg_vgicp_vmap(None, ids, ids, 1, None, C.byref(capi.default_vgicp_params()), None, None, None, None, None, None), b"null")
    bad = capi.default_robust_params(kind=99)
    refused(L.gloc_reg_vgicp_vmap(None, ids, ids, 1, None, C.byref(capi.default_vgicp_params()), C.byref(bad), T, None, None, None, None), b"kind")
