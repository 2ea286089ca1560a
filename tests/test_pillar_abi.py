"""CPU: the PointPillar additions to the C ABI -- parameters and their defaults, exported symbols, no CPU fallback."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest


def test_pillar_default_params(capi):
    p = capi.default_pillar_params()
    assert list(p.xbound) == [-35.0, 35.0, 0.5]      # s2s_libtorch/gen_libtorch_pointpillar.py:27
    assert list(p.ybound) == [-20.0, 20.0, 0.5]      # :28
    assert list(p.zbound) == [-10.0, 10.0, 20.0]     # :29
    assert p.num_points == 122480                    # dataset/kitti_s2s.py:222-227
    assert p.mask_mode == capi.PILLAR_MASK_INPUT == 0
    assert p.grid() == (140, 80, 1)
    q = capi.default_pillar_params(num_points=2048, xbound=(-2.0, 2.0, 0.5), mask_mode=capi.PILLAR_MASK_VALID)
    assert q.num_points == 2048 and list(q.xbound) == [-2.0, 2.0, 0.5] and q.mask_mode == 1
    assert list(q.ybound) == [-20.0, 20.0, 0.5] and q.grid() == (8, 80, 1)


def test_pillar_params_layout(capi):
    assert C.sizeof(capi.PillarParams) == 44


def test_pillar_symbols_exported(capi):
    L = capi.lib()
    for name in ("gloc_pillar_default_params", "gloc_pillar_create", "gloc_pillar_destroy", "gloc_pillar_set_stream",
                 "gloc_pillar_synchronize", "gloc_pillar_set_pointnet", "gloc_pillar_inputs", "gloc_pillar_inputs_device",
                 "gloc_pillar_canvas", "gloc_pillar_canvas_device"):
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS
    for name in ("inputs", "canvas", "inputs_device", "canvas_device", "set_pointnet", "set_stream"):
        assert callable(getattr(capi.PillarEncoder, name))
    assert L.gloc_abi_version() == 6


def test_pillar_calls_refuse_without_gpu(capi):
    if capi.lib().gloc_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(capi.GlocError) as e:
        capi.PillarEncoder()
    assert e.value.code == 4                          # GLOC_ERR_NODEVICE
    L = capi.lib()
    p = capi.default_pillar_params()
    pts = np.zeros((4, 4), np.float32)
    off = np.array([0, 4], np.uint64)
    out = np.zeros(16 * p.num_points, np.float32)
    # no handle, no host computation behind it
    assert L.gloc_pillar_inputs(None, pts.ctypes.data, off.ctypes.data, 1, 4, C.byref(p), out.ctypes.data) == 1
    assert L.gloc_pillar_canvas(None, pts.ctypes.data, off.ctypes.data, 1, 4, C.byref(p), out.ctypes.data) == 1
    assert L.gloc_pillar_inputs_device(None, None, off.ctypes.data, 1, 4, C.byref(p), None) == 1
    assert L.gloc_pillar_set_pointnet(None, None, None, None, None, None, 1e-5) == 1


def test_import_does_not_pull_torch():
    code = "import sys, gloc3d_amd, gloc3d_amd.capi; assert 'torch' not in sys.modules, 'torch imported'"
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([sys.executable, "-c", code], cwd=root)
