"""CPU: the VGG16 encoder's additions to the C ABI -- exported symbols, the layer table, no CPU fallback."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

NAMES = ("gloc_vgg_create", "gloc_vgg_destroy", "gloc_vgg_set_stream", "gloc_vgg_synchronize", "gloc_vgg_layer_shape",
         "gloc_vgg_set_layer", "gloc_vgg_forward", "gloc_vgg_forward_device", "gloc_vgg_forward_layer",
         "gloc_vgg_set_profile", "gloc_vgg_profile", "gloc_vgg_profile_reset")


def test_vgg_symbols_exported(capi):
    L = capi.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS
    for name in ("set_layer", "set_layers", "forward", "forward_device", "forward_layer_device", "set_stream",
                 "synchronize", "profile", "profile_reset"):
        assert callable(getattr(capi.VggEncoder, name))
    assert L.gloc_abi_version() == 6


def test_vgg_layer_table(capi):
    """VGG16 features[:-2]: 13 convolutions, pools after conv1_2, conv2_2, conv3_3 and conv4_3, none after conv5_3,
    and conv5_3 without its ReLU."""
    table = [capi.vgg_layer_shape(i) for i in range(13)]
    assert [t[:2] for t in table] == [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256),
                                      (256, 512), (512, 512), (512, 512), (512, 512), (512, 512), (512, 512)]
    assert [i for i, t in enumerate(table) if t[3]] == [1, 3, 6, 9]
    assert [i for i, t in enumerate(table) if not t[2]] == [12]
    assert capi.lib().gloc_vgg_layer_shape(13, None, None, None, None) == 1
    assert capi.lib().gloc_vgg_layer_shape(-1, None, None, None, None) == 1


def test_vgg_calls_refuse_without_gpu(capi):
    if capi.lib().gloc_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(capi.GlocError) as e:
        capi.VggEncoder()
    assert e.value.code == 4                          # GLOC_ERR_NODEVICE
    L = capi.lib()
    h = C.c_void_p()
    assert L.gloc_vgg_create(0, C.byref(h)) == 4 and not h.value
    x = np.zeros((1, 3, 16, 16), np.float32)
    out = np.zeros(512, np.float32)
    w = np.zeros((64, 3, 3, 3), np.float32)
    b = np.zeros(64, np.float32)
    # no handle, no host computation behind it
    assert L.gloc_vgg_forward(None, x.ctypes.data, 1, 16, 16, out.ctypes.data) == 1
    assert L.gloc_vgg_forward_device(None, x.ctypes.data, 1, 16, 16, out.ctypes.data) == 1
    assert L.gloc_vgg_forward_layer(None, 0, x.ctypes.data, 1, 16, 16, out.ctypes.data) == 1
    assert L.gloc_vgg_set_layer(None, 0, w.ctypes.data, b.ctypes.data) == 1
    assert L.gloc_vgg_set_stream(None, None) == 1 and L.gloc_vgg_synchronize(None) == 1
    assert L.gloc_vgg_set_profile(None, 1) == 1 and L.gloc_vgg_profile_reset(None) == 1
    assert L.gloc_vgg_profile(None, b"vgg_conv0", None, None) == 1
    assert L.gloc_vgg_destroy(None) == 0


def test_capi_import_does_not_pull_torch():
    code = ("import sys, gloc3d_amd, gloc3d_amd.capi, gloc3d_amd.loop_detector; "
            "assert 'torch' not in sys.modules, 'torch imported'")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call([sys.executable, "-c", code], cwd=root)
