"""CPU: the PointPillar backbone additions to the C ABI -- exported symbols, the layer table against PillarBackbone, no
CPU fallback, the GLOCPPW weights file, and the s2s_feature_extract command line's refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pillar_ref as R  # noqa: E402

NEW_SYMBOLS = ("gloc_pillar_backbone_layer_shape", "gloc_pillar_set_backbone_layer", "gloc_pillar_backbone_device",
               "gloc_pillar_backbone_layer_device", "gloc_pillar_upsample_device", "gloc_pillar_features",
               "gloc_pillar_features_device")


def seeded_pillar_vlad_sd():
    """A PointPillarVLAD state_dict under the seeded weights of tests/pillar_ref.py (conv_out_pose included, as a real
    checkpoint has it)."""
    from gloc3d_amd.pillar import PillarBackbone
    shapes = {"encoder." + k: tuple(t.shape) for k, t in PillarBackbone(140, 80).state_dict().items()}
    shapes.update({"encoder.pn.pointnet.0.weight": (64, 14, 1), "encoder.pn.pointnet.1.weight": (64,),
                   "encoder.pn.pointnet.1.bias": (64,), "encoder.pn.pointnet.1.running_mean": (64,),
                   "encoder.pn.pointnet.1.running_var": (64,), "encoder.pn.pointnet.1.num_batches_tracked": (),
                   "pool.conv.weight": (64, 128, 1, 1), "pool.centroids": (64, 128), "pool.hidden1_weights": (8192, 128),
                   "encoder.conv_out_pose.0.weight": (256, 448, 3, 3)})
    return R.seeded_state_dict(shapes)


def test_backbone_symbols_exported(capi):
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in capi.EXPORTED_SYMBOLS, name
    for name in ("set_backbone_layer", "backbone_device", "backbone_layer_device", "upsample_device", "features",
                 "features_device"):
        assert callable(getattr(capi.PillarEncoder, name)), name
    assert L.gloc_abi_version() == 6


def test_layer_shape_matches_pillar_backbone(capi):
    import torch.nn as nn
    from gloc3d_amd.pillar import BACKBONE_KEYS, PillarBackbone
    m = PillarBackbone(140, 80)
    sd = m.state_dict()
    mods = dict(m.named_modules())
    assert capi.PILLAR_BACKBONE_LAYERS == len(BACKBONE_KEYS) == 13
    convs = [k for k, v in mods.items() if isinstance(v, nn.Conv2d)]
    assert sorted(convs) == sorted(c for c, _ in BACKBONE_KEYS)       # every convolution of the module, once
    for layer, (conv, bn) in enumerate(BACKBONE_KEYS):
        ci, co, stride, relu = capi.pillar_backbone_layer_shape(layer)
        assert tuple(sd[conv + ".weight"].shape) == (co, ci, 3, 3), layer
        assert tuple(sd[bn + ".running_var"].shape) == (co,), layer
        assert mods[conv].stride == (stride, stride) and mods[conv].padding == (1, 1) and mods[conv].bias is None
        assert isinstance(mods[bn], nn.BatchNorm2d)
        assert relu == (layer != 12), layer                              # conv_out.3 has no ReLU
    L = capi.lib()
    assert L.gloc_pillar_backbone_layer_shape(13, None, None, None, None) == 1
    assert L.gloc_pillar_backbone_layer_shape(-1, None, None, None, None) == 1


def test_backbone_calls_refuse_without_gpu(capi):
    if capi.lib().gloc_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(capi.GlocError) as e:
        capi.PillarEncoder()
    assert e.value.code == 4                          # GLOC_ERR_NODEVICE
    L = capi.lib()
    p = capi.default_pillar_params()
    pts = np.zeros((4, 4), np.float32)
    off = np.array([0, 4], np.uint64)
    out = np.zeros(128 * 140 * 80, np.float32)
    w = np.zeros(64 * 64 * 9, np.float32)
    # no handle, no host computation behind it
    assert L.gloc_pillar_features(None, pts.ctypes.data, off.ctypes.data, 1, 4, C.byref(p), out.ctypes.data) == 1
    assert L.gloc_pillar_features_device(None, None, off.ctypes.data, 1, 4, C.byref(p), None) == 1
    assert L.gloc_pillar_backbone_device(None, None, 1, 140, 80, None) == 1
    assert L.gloc_pillar_backbone_layer_device(None, 0, None, 1, 140, 80, None) == 1
    assert L.gloc_pillar_upsample_device(None, None, 1, 1, 4, 4, 2, None) == 1
    assert L.gloc_pillar_set_backbone_layer(None, 0, w.ctypes.data, w.ctypes.data, w.ctypes.data, w.ctypes.data,
                                            w.ctypes.data, 1e-5) == 1


def test_glocppw_round_trip(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_pillar_weights as X
    import torch
    sd = seeded_pillar_vlad_sd()
    w = X.pillar_weights({"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}})
    path = tmp_path / "s2s.bin"
    X.write(str(path), w)
    back = X.read(str(path))
    assert open(path, "rb").read(8) == b"GLOCPPW\0"
    pn = "encoder.pn.pointnet."
    exp_pn = [sd[pn + "0.weight"].reshape(64, 14)] + [sd[pn + "1." + k] for k in
                                                     ("weight", "bias", "running_mean", "running_var")]
    for a, b in zip(back["pointnet"][:5], exp_pn):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert back["pointnet"][5] == np.float32(1e-5)
    from gloc3d_amd.pillar import BACKBONE_KEYS
    assert len(back["backbone"]) == 13
    for layer, (conv, bn) in zip(back["backbone"], BACKBONE_KEYS):
        exp = [sd["encoder." + conv + ".weight"]] + [sd["encoder." + bn + "." + k] for k in
                                                    ("weight", "bias", "running_mean", "running_var")]
        for a, b in zip(layer[:5], exp):
            assert a.shape == b.shape and np.array_equal(a, b)
        assert layer[5] == np.float32(1e-5)
    assert np.array_equal(back["conv_w"], sd["pool.conv.weight"].reshape(64, 128)) and back["conv_b"] is None
    assert np.array_equal(back["centroids"], sd["pool.centroids"])
    assert np.array_equal(back["fc_w"], sd["pool.hidden1_weights"])
    # a bare state_dict of numpy arrays gives the same file
    X.write(str(tmp_path / "bare.bin"), X.pillar_weights(sd))
    assert open(tmp_path / "bare.bin", "rb").read() == open(path, "rb").read()


def test_s2s_feature_extract_refusals(tmp_path):
    from gloc3d_amd import build
    exe = [e for e in build.build_cli() if os.path.basename(e) == "s2s_feature_extract"]
    assert len(exe) == 1 and os.access(exe[0], os.X_OK)
    run = lambda *a: subprocess.run([exe[0], *map(str, a)], capture_output=True, text=True, timeout=120)
    p = run()
    assert p.returncode != 0 and "usage" in p.stderr
    p = run(tmp_path / "missing.bin")
    assert p.returncode != 0 and "usage" in p.stderr
    bad = tmp_path / "not_weights.bin"
    bad.write_bytes(b"GLOCI2IW" + bytes(64))
    scan = tmp_path / "000000.bin"
    np.zeros((10, 4), np.float32).tofile(scan)
    p = run(bad, scan)
    assert p.returncode != 0 and "GLOCPPW" in p.stderr
    p = run(tmp_path / "missing.bin", scan)
    assert p.returncode != 0
