"""CPU: the M2DP additions to the C ABI -- parameters and their defaults, exported symbols, what is refused before a
device is looked for, the host-only seed, and no CPU fallback."""
import ctypes as C

import numpy as np
import pytest

import m2dp_ref as R

SYMBOLS = ("default_params", "dim", "create", "destroy", "set_stream", "synchronize", "describe", "describe_store_scans",
           "describe_store_scans_device", "signature_svd", "frame_to_seed", "set_profile", "profile", "profile_reset")


def test_m2dp_default_params_and_dim(capi):
    p = capi.default_m2dp_params()
    assert (p.n_azimuth, p.n_elevation, p.n_rings, p.n_sectors, p.max_range, p.min_points, p.reserved_) == (4, 16, 8, 16, 80.0, 16, 0)
    assert C.sizeof(capi.M2dpParams) == 28
    assert capi.m2dp_dim(p) == 192 == R.dim()
    q = capi.default_m2dp_params(n_azimuth=2, n_elevation=3, n_rings=4, n_sectors=5)
    assert capi.m2dp_dim(q) == 26
    assert capi.m2dp_dim(capi.default_m2dp_params(n_azimuth=1, n_elevation=1, n_rings=1, n_sectors=2)) == 3
    assert capi.m2dp_dim(capi.default_m2dp_params(n_azimuth=64, n_elevation=1, n_rings=2, n_sectors=64)) == 192


def test_m2dp_symbols_exported(capi):
    L = capi.lib()
    names = [n for n in capi.EXPORTED_SYMBOLS if n.startswith("gloc_m2dp_")]
    assert sorted(names) == sorted("gloc_m2dp_" + s for s in SYMBOLS) and all(hasattr(L, n) for n in names)
    for name in ("describe", "describe_store_scans", "describe_store_scans_device", "signature_svd", "set_stream",
                 "synchronize", "set_profile", "profile", "profile_reset"):
        assert callable(getattr(capi.M2dp, name))
    assert L.gloc_abi_version() == 6
    from gloc3d_amd.m2dp import M2DPLoopDetector
    for name in ("add_keyframe", "add_store_keyframes", "detect", "detect_slam", "match"):
        assert callable(getattr(M2DPLoopDetector, name))


def test_m2dp_invalid_params_refused_before_the_device(capi):
    """gloc_m2dp_create checks the parameter block before it selects the device, so these are GLOC_ERR_INVALID with or
    without a GPU; gloc_m2dp_dim is host-only and checks the same block."""
    for bad in (dict(n_azimuth=0), dict(n_elevation=0), dict(n_azimuth=5), dict(n_azimuth=65, n_elevation=1),
                dict(n_azimuth=2**31, n_elevation=2), dict(n_rings=0), dict(n_sectors=1), dict(n_rings=9),
                dict(n_rings=1, n_sectors=129), dict(n_rings=2**31, n_sectors=2), dict(max_range=0.0), dict(max_range=-1.0),
                dict(max_range=float("inf")), dict(max_range=float("nan")), dict(min_points=3), dict(min_points=0),
                dict(reserved_=1)):
        with pytest.raises(capi.GlocError) as e:
            capi.M2dp(params=capi.default_m2dp_params(**bad))
        assert e.value.code == 1, bad
        with pytest.raises(capi.GlocError) as e:
            capi.m2dp_dim(capi.default_m2dp_params(**bad))
        assert e.value.code == 1, bad
    h = C.c_void_p(1)
    assert capi.lib().gloc_m2dp_create(0, None, C.byref(h)) == 1 and not h.value       # null block; *out is cleared


def test_m2dp_frame_to_seed_on_the_host(capi):
    rng = np.random.default_rng(12)
    for _ in range(5):
        fr = []
        for _ in range(2):
            Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
            Q *= np.sign(np.linalg.det(Q))
            fr.append(np.concatenate([Q.ravel(), rng.uniform(-20, 20, 3)]))
        T = capi.m2dp_frame_to_seed(fr[0], fr[1])
        ref = R.frame_to_seed(fr[0], fr[1])
        assert T.dtype == np.float32 and np.abs(T - ref).max() <= 2.0 ** -24 * 128   # one fp32 rounding of values below 128
        assert (T[3] == [0, 0, 0, 1]).all()
    same = capi.m2dp_frame_to_seed(fr[0], fr[0])
    assert np.abs(same - np.eye(4)).max() < 1e-6
    L = capi.lib()
    assert L.gloc_m2dp_frame_to_seed(None, fr[0].ctypes.data, same.ctypes.data) == 1
    assert L.gloc_m2dp_frame_to_seed(fr[0].ctypes.data, fr[1].ctypes.data, None) == 1


def test_m2dp_refuses_without_gpu(capi):
    if capi.lib().gloc_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(capi.GlocError) as e:
        capi.M2dp()
    assert e.value.code == 4                                          # GLOC_ERR_NODEVICE
    L = capi.lib()
    out = np.zeros(192, np.float32)
    pts = np.zeros((20, 3), np.float32)
    assert L.gloc_m2dp_describe(None, pts.ctypes.data, 20, 3, out.ctypes.data, None, None) == 1   # no handle, nothing computed on the host
    assert L.gloc_m2dp_describe_store_scans(None, None, None, 0, None, None, None) == 1
    assert L.gloc_m2dp_signature_svd(None, None, None, 1, out.ctypes.data, None) == 1
