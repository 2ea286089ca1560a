"""GPU: the PointPillar backbone (gloc_pillar_backbone*, gloc_pillar_features*).  Each layer alone against F.conv2d +
eval BatchNorm (+ ReLU) in fp32 on the CPU, the upsample against F.interpolate, the whole backbone against PillarBackbone
on the CPU, the descriptor against the reference module's golden and the torch backbone, batches and streams bit for
bit, and the s2s_feature_extract command line against PillarVladDescriptor(backbone="hip")."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pillar_ref as R  # noqa: E402
from test_pillar_backbone_abi import seeded_pillar_vlad_sd  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden")
TOL = 1e-4   # relative to max|ref| (the numerical contract, include/gloc3d.h)


@pytest.fixture(scope="module")
def sd():
    return seeded_pillar_vlad_sd()


def make_encoder(capi, sd, skip=()):
    from gloc3d_amd.pillar import backbone_layers
    e = capi.PillarEncoder()
    e.set_pointnet(*R.pn_params_from_state(sd))
    for layer, args in enumerate(backbone_layers(sd)):
        if layer not in skip:
            e.set_backbone_layer(layer, *args)
    return e


@pytest.fixture(scope="module")
def enc(capi, sd):
    e = make_encoder(capi, sd)
    yield e
    e.close()


@pytest.fixture(scope="module")
def lidar():
    from gloc3d_amd import synth
    w = synth.make_world(7)
    return [synth.lidar_scan(w, synth.se3(25.0 * k, (4.0 * k, -1.5 * k, 0)), 7 + k) for k in range(3)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rel_err(a, ref):
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / np.abs(ref).max())


def torch_layer(sd, layer, x):
    import torch
    import torch.nn.functional as F
    from gloc3d_amd import capi
    from gloc3d_amd.pillar import BACKBONE_KEYS
    conv, bn = BACKBONE_KEYS[layer]
    g = lambda k: torch.from_numpy(np.asarray(sd["encoder." + k]))
    t = torch.from_numpy(x)
    if layer in (9, 10):
        t = F.interpolate(t, scale_factor=2 if layer == 9 else 4, mode="bilinear", align_corners=True)
    _, _, stride, relu = capi.pillar_backbone_layer_shape(layer)
    y = F.conv2d(t, g(conv + ".weight"), stride=stride, padding=1)
    y = F.batch_norm(y, g(bn + ".running_mean"), g(bn + ".running_var"), g(bn + ".weight"), g(bn + ".bias"),
                     training=False, eps=1e-5)
    return (torch.relu(y) if relu else y).numpy()


def gpu_layer(enc, layer, x):
    import torch
    from gloc3d_amd import capi
    n, _, H, W = x.shape
    _, co, stride, _ = capi.pillar_backbone_layer_shape(layer)
    up = {9: 2, 10: 4}.get(layer, 1)
    Ho, Wo = ((H * up - 1) // stride + 1, (W * up - 1) // stride + 1)
    d_in = torch.from_numpy(x).cuda()
    out = torch.full((n, co, Ho, Wo), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    enc.backbone_layer_device(layer, d_in.data_ptr(), n, H, W, out.data_ptr())
    enc.synchronize()
    return out.cpu().numpy()


# the input sizes each layer sees in the network (H = gx = 140, W = gy = 80), then odd small ones: both stride-2
# layers at odd H / W and at 1 x 1, the upsampled layers at odd sizes, conv_out.3's signed output
REAL = {0: (140, 80), 1: (140, 80), 2: (140, 80), 3: (70, 40), 4: (70, 40), 5: (70, 40), 6: (35, 20), 7: (35, 20),
        8: (140, 80), 9: (70, 40), 10: (35, 20), 11: (140, 80), 12: (140, 80)}
CASES = [(layer, 1, *hw) for layer, hw in REAL.items()] + [
    (0, 2, 13, 7), (2, 3, 13, 7), (2, 1, 1, 1), (2, 2, 9, 35), (5, 2, 35, 21), (5, 1, 1, 1), (5, 3, 7, 3),
    (6, 2, 5, 33), (9, 2, 3, 5), (10, 1, 1, 1), (10, 2, 5, 3), (11, 1, 9, 17), (12, 3, 7, 19), (12, 1, 1, 1)]


@pytest.mark.parametrize("layer,n,H,W", CASES)
def test_single_layer_random_fp32(sd, enc, layer, n, H, W):
    from gloc3d_amd import capi
    ci, _, _, _ = capi.pillar_backbone_layer_shape(layer)
    rng = np.random.default_rng(2000 + 31 * layer + 7 * n + H)
    x = rng.standard_normal((n, ci, H, W)).astype(np.float32)
    if layer > 0:
        x = np.maximum(x, 0) * 2.0      # a post-ReLU input, as inside the network (the canvas of layer 0 is signed)
    g, r = gpu_layer(enc, layer, x), torch_layer(sd, layer, x)
    assert g.shape == r.shape and not np.isnan(g).any()
    assert rel_err(g, r) <= TOL, rel_err(g, r)
    if layer == 12:
        assert (g < 0).any() and (r < 0).any()    # no ReLU after conv_out.3


def test_single_layer_signed_inputs(sd, enc):
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 256, 11, 9)) * np.exp(rng.uniform(-3, 3, (2, 256, 11, 9)))).astype(np.float32)
    for layer in (6, 12):
        g, r = gpu_layer(enc, layer, x), torch_layer(sd, layer, x)
        assert rel_err(g, r) <= TOL, (layer, rel_err(g, r))


@pytest.mark.parametrize("n,C,H,W,s", [(1, 128, 70, 40, 2), (1, 256, 35, 20, 4), (2, 3, 1, 1, 4), (3, 5, 7, 2, 2),
                                       (1, 2, 2, 9, 4)])
def test_upsample_matches_interpolate(enc, n, C, H, W, s):
    import torch
    import torch.nn.functional as F
    x = np.random.default_rng(n * 100 + C + H).standard_normal((n, C, H, W)).astype(np.float32)
    d_in = torch.from_numpy(x).cuda()
    out = torch.full((n, C, H * s, W * s), float("nan"), device="cuda")
    torch.cuda.synchronize()
    enc.upsample_device(d_in.data_ptr(), n, C, H, W, s, out.data_ptr())
    enc.synchronize()
    ref = F.interpolate(torch.from_numpy(x), scale_factor=s, mode="bilinear", align_corners=True).numpy()
    g = out.cpu().numpy()
    assert rel_err(g, ref) <= 1e-6, rel_err(g, ref)


def canvases(enc, scans, params=None):
    return enc.canvas(scans, params)


def hip_backbone(enc, canvas):
    import torch
    c = torch.from_numpy(np.ascontiguousarray(canvas)).cuda()
    out = torch.full((c.shape[0], 128, 140 * 80), float("nan"), device="cuda")
    torch.cuda.synchronize()
    enc.backbone_device(c.data_ptr(), c.shape[0], 140, 80, out.data_ptr())
    enc.synchronize()
    return out.cpu().numpy()


def test_whole_backbone_on_real_canvas(sd, enc, lidar):
    import torch
    from gloc3d_amd.pillar import PillarBackbone
    cv = canvases(enc, lidar[:2])
    assert (cv != 0).any(axis=(1, 2)).all()
    m = PillarBackbone(140, 80).eval()
    m.load_state_dict({k[len("encoder."):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()
                       if k.startswith("encoder.") and not k.startswith(("encoder.pn.", "encoder.conv_out_pose."))})
    with torch.no_grad():
        ref = m(torch.from_numpy(cv)).contiguous().numpy().reshape(2, 128, -1)   # [B, 128, gy, gx]
    g = hip_backbone(enc, cv)
    assert rel_err(g, ref) <= TOL, rel_err(g, ref)


def test_descriptor_matches_golden_and_torch(capi, sd):
    import importlib.util
    import torch
    from gloc3d_amd.pillar import PillarVladDescriptor
    spec = importlib.util.spec_from_file_location("make_pillar_goldens", os.path.join(GOLDEN, "make_pillar_goldens.py"))
    MK = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(MK)
    g = np.load(os.path.join(GOLDEN, "pillar_descriptor.npz"))
    tsd = {"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}
    p = capi.default_pillar_params(num_points=int(g["P"]))
    hip = PillarVladDescriptor.from_state_dict(tsd, params=p, backbone="hip")
    tor = PillarVladDescriptor.from_state_dict(tsd, params=p)
    assert hip.backbone is None and tor.backbone is not None
    scans = MK.descriptor_scans()
    out, ref_t = hip(scans), tor(scans)
    assert out.shape == g["desc"].shape
    assert np.abs(out - g["desc"]).max() <= 1e-3
    assert np.abs(out - ref_t).max() <= 1e-4, np.abs(out - ref_t).max()
    one = hip(scans[1])
    assert (bits(one[0]) == bits(hip(scans[1])[0])).all()     # the same bits on every run
    hip.close()
    tor.close()


@pytest.mark.parametrize("B", [5, 11, 17])
def test_batch_equals_single_calls(enc, B):
    """17 > the 16 scans of one pass: the chunking too."""
    rng = np.random.default_rng(B)
    cv = (rng.standard_normal((B, 64, 140 * 80)) * (rng.random((B, 64, 140 * 80)) < 0.3)).astype(np.float32)
    full = hip_backbone(enc, cv)
    for k in range(B):
        assert (bits(hip_backbone(enc, cv[k:k + 1])[0]) == bits(full[k])).all(), k


def test_device_path_on_torch_stream(enc, lidar):
    import torch
    p = capi_params()
    scans = lidar[:2]
    host = enc.features(scans, p)
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(scans))).cuda()
    off = np.array([0, len(scans[0]), len(scans[0]) + len(scans[1])], np.uint64)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = torch.empty((2, 128, 140 * 80), device="cuda")
        enc.set_stream(s.cuda_stream)
        enc.features_device(pts.data_ptr(), off, 4, out.data_ptr(), p)
    s.synchronize()
    enc.set_stream(0)
    assert (bits(out.cpu().numpy()) == bits(host)).all()


def capi_params(**kw):
    from gloc3d_amd import capi
    return capi.default_pillar_params(**kw)


def test_features_equal_canvas_then_backbone(enc, lidar):
    p = capi_params()
    f = enc.features(lidar, p)
    assert (bits(f) == bits(hip_backbone(enc, canvases(enc, lidar, p)))).all()


def test_refusals(capi, sd, enc):
    e = make_encoder(capi, sd, skip=(7,))
    with pytest.raises(capi.GlocError) as err:
        e.features(np.zeros((3, 4), np.float32))
    assert err.value.code == 5                                       # GLOC_ERR_STATE: layer 7 unset
    with pytest.raises(capi.GlocError) as err:
        e.backbone_layer_device(7, 16, 1, 4, 4, 16)
    assert err.value.code == 5
    e.close()
    e = capi.PillarEncoder()
    from gloc3d_amd.pillar import backbone_layers
    for layer, args in enumerate(backbone_layers(sd)):
        e.set_backbone_layer(layer, *args)
    with pytest.raises(capi.GlocError) as err:
        e.features(np.zeros((3, 4), np.float32))
    assert err.value.code == 5                                       # no PointNet
    e.close()
    with pytest.raises(capi.GlocError) as err:                       # gz = 2
        enc.features(np.zeros((3, 4), np.float32), capi_params(zbound=(-10.0, 10.0, 10.0)))
    assert err.value.code == 1
    with pytest.raises(capi.GlocError) as err:                       # gx = 70 / 4 is not whole
        enc.features(np.zeros((3, 4), np.float32), capi_params(xbound=(-35.0, 35.0, 1.0)))
    assert err.value.code == 1
    with pytest.raises(capi.GlocError) as err:
        enc.backbone_device(16, 1, 142, 80, 16)
    assert err.value.code == 1


def test_command_line_matches_descriptor(capi, sd, lidar, tmp_path):
    """s2s_feature_extract WEIGHTS SCAN.bin ... (GLOCPPW exported from the same weights) gives the descriptors of
    PillarVladDescriptor(backbone="hip") on the same scans, bit for bit."""
    import torch
    from gloc3d_amd import build, gloc_io, synth
    from gloc3d_amd.pillar import PillarVladDescriptor
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_pillar_weights as X
    X.write(str(tmp_path / "s2s.bin"), X.pillar_weights(sd))
    files = []
    for k, s in enumerate(lidar + [lidar[0][:5000]]):
        files.append(str(tmp_path / f"{k:06d}.bin"))
        synth.write_kitti_bin(files[-1], s)
    exe = [e for e in build.build_cli() if os.path.basename(e) == "s2s_feature_extract"][0]
    env = dict(os.environ, GLOC_DUMP_DESCRIPTORS=str(tmp_path / "desc.bin"))
    p = subprocess.run([exe, str(tmp_path / "s2s.bin")] + files, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Processing time per frame = " in p.stdout and p.stdout.strip().endswith("sec")
    got = gloc_io.read_descriptors(tmp_path / "desc.bin")
    d = PillarVladDescriptor.from_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()},
                                             backbone="hip")
    ref = np.stack([d(synth.read_kitti_bin(f))[0] for f in files])
    d.close()
    assert got.shape == ref.shape == (len(files), 128)
    assert (bits(got) == bits(ref)).all()
