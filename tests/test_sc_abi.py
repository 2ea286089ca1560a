"""CPU: the Scan Context additions to the C ABI -- parameters and their defaults, exported symbols, what is refused
before a device is looked for, and no CPU fallback."""
import ctypes as C

import numpy as np
import pytest


def test_sc_default_params(capi):
    p = capi.default_sc_params()
    assert (p.n_rings, p.n_sectors, p.max_radius, p.sensor_height, p.min_common_columns) == (20, 60, 80.0, 2.0, 1)
    q = capi.default_sc_params(n_rings=8, n_sectors=24, min_common_columns=3)
    assert (q.n_rings, q.n_sectors, q.max_radius, q.min_common_columns) == (8, 24, 80.0, 3)
    assert C.sizeof(capi.ScParams) == 24


def test_sc_symbols_exported(capi):
    L = capi.lib()
    names = [n for n in capi.EXPORTED_SYMBOLS if n.startswith("gloc_sc_")]
    assert len(names) == 24 and all(hasattr(L, n) for n in names)
    for name in ("describe", "describe_store_scans", "add", "add_scan", "add_store_scans", "rows", "ring_keys", "save", "load",
                 "search", "search_store_scans", "distances", "shift_to_yaw", "set_stream", "synchronize", "set_profile",
                 "profile", "profile_reset", "clear", "reserve"):
        assert callable(getattr(capi.ScanContext, name))
    assert L.gloc_abi_version() == 6


def test_sc_invalid_params_refused_before_the_device(capi):
    """gloc_sc_create checks the parameter block before it selects the device, so these are GLOC_ERR_INVALID with or
    without a GPU; gloc_sc_shift_to_yaw is host-only and checks the same block."""
    for bad in (dict(n_rings=0), dict(n_rings=33), dict(n_sectors=1), dict(n_sectors=65), dict(max_radius=0.0),
                dict(max_radius=-1.0), dict(max_radius=float("inf")), dict(max_radius=float("nan")),
                dict(sensor_height=float("nan")), dict(sensor_height=float("inf"))):
        with pytest.raises(capi.GlocError) as e:
            capi.ScanContext(params=capi.default_sc_params(**bad))
        assert e.value.code == 1, bad
        with pytest.raises(capi.GlocError) as e:
            capi.sc_shift_to_yaw(capi.default_sc_params(**bad), 0)
        assert e.value.code == 1, bad
    h = C.c_void_p(1)
    assert capi.lib().gloc_sc_create(0, None, C.byref(h)) == 1 and not h.value      # null block; *out is cleared


def test_sc_shift_to_yaw_on_the_host(capi):
    p = capi.default_sc_params()
    assert capi.sc_shift_to_yaw(p, 0) == 0.0
    assert abs(capi.sc_shift_to_yaw(p, 15) - np.pi / 2) < 1e-6
    assert abs(capi.sc_shift_to_yaw(p, 30) - np.pi) < 1e-6            # (-pi, pi]: half a turn is +pi
    assert abs(capi.sc_shift_to_yaw(p, 52) - np.deg2rad(-48.0)) < 1e-6
    with pytest.raises(capi.GlocError):
        capi.sc_shift_to_yaw(p, 60)


def test_sc_refuses_without_gpu(capi):
    if capi.lib().gloc_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(capi.GlocError) as e:
        capi.ScanContext()
    assert e.value.code == 4                                          # GLOC_ERR_NODEVICE
    L = capi.lib()
    out = np.zeros((20, 60), np.float32)
    pts = np.zeros((4, 3), np.float32)
    assert L.gloc_sc_describe(None, pts.ctypes.data, 4, 3, out.ctypes.data) == 1     # no handle, nothing computed on the host
    assert L.gloc_sc_add(None, out.ctypes.data, 1) == 1
    assert L.gloc_sc_search(None, out.ctypes.data, 1, 1, 0, 1, None, None, None) == 1
