"""CPU: the NDT additions to the C ABI -- parameters and their defaults, exported symbols, no CPU fallback."""
import ctypes as C

import pytest


def test_ndt_default_params(capi):
    p = capi.default_ndt_params()
    f32 = lambda v: C.c_float(v).value
    assert p.source_leaf == f32(0.2)             # registration/global_registration.cpp:256
    assert p.resolution == f32(0.5)              # :271
    assert p.step_size == f32(0.1)               # :268
    assert p.trans_eps == f32(0.01)              # :266
    assert p.max_iters == 35                     # :274
    assert p.outlier_ratio == f32(0.55)          # PCL's defaults [upstream]
    assert p.min_points_per_cell == 6
    assert p.min_covar_eigvalue_mult == f32(0.01)
    q = capi.default_ndt_params(max_iters=10, resolution=1.0)
    assert q.max_iters == 10 and q.resolution == 1.0 and q.step_size == f32(0.1)


def test_ndt_symbols_exported(capi):
    L = capi.lib()
    for name in ("gloc_ndt_default_params", "gloc_reg_ndt_batch_ids", "gloc_reg_ndt_derivatives", "gloc_reg_ndt_cells",
                 "gloc_scan_store_add_approx_voxel"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS
    for name in ("ndt_batch", "ndt_derivatives", "ndt_cells"):
        assert callable(getattr(capi.Registrar, name))
    assert callable(capi.ScanStore.add_approx_voxel)


def test_ndt_calls_refuse_without_gpu(capi):
    if capi.lib().gloc_device_count() > 0:
        pytest.skip("a GPU is visible")
    # the handles the NDT calls need cannot be made: GLOC_ERR_NODEVICE, and no CPU path behind them
    for make in (capi.Registrar, capi.ScanStore):
        with pytest.raises(capi.GlocError) as e:
            make()
        assert e.value.code == 4
    # the calls themselves refuse a missing handle instead of computing anything on the host
    L = capi.lib()
    prm = capi.default_ndt_params()
    sid = C.c_uint32()
    assert L.gloc_scan_store_add_approx_voxel(None, 0, 0.2, C.byref(sid)) == 1
    assert L.gloc_reg_ndt_batch_ids(None, 0, None, 1, None, C.byref(prm), None, None, None, None) == 1
    n = C.c_size_t()
    assert L.gloc_reg_ndt_cells(None, 0, C.byref(prm), 0, None, None, None, None, C.byref(n)) == 1
