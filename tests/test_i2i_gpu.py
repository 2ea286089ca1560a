"""GPU: the VGG16 encoder (gloc_vgg_*) and the i2i descriptor.  Single layers against torch's fp32 Conv2d on the CPU on
random fp32 inputs, the whole encoder and descriptor against the goldens of tests/golden/make_i2i_goldens.py (the
reference's NetVLAD head), batches equal to single calls bit for bit, refusals, I2iVladDescriptor on synthetic scans,
and the command line's MODEL mode against its descriptor-file mode."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import i2i_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden")
FEAT_TOL, DESC_TOL = 1e-4, 5e-4   # relative to max|ref| (the numerical contract, include/gloc3d.h)


@pytest.fixture(scope="module")
def sd():
    return R.make_state_dict(R.SEED)


@pytest.fixture(scope="module")
def enc(capi, sd):
    from gloc3d_amd import i2i
    e = capi.VggEncoder()
    e.set_layers(i2i.i2i_weights(sd)["encoder"])
    yield e
    e.close()


def torch_layer(sd, layer, x):
    import torch
    import torch.nn.functional as F
    from gloc3d_amd import i2i
    i = i2i.ENCODER_CONV_IDX[layer]
    _, _, relu, pool = i2i._shape(layer)
    y = F.conv2d(torch.from_numpy(x), torch.from_numpy(sd[f"encoder.{i}.weight"]),
                 torch.from_numpy(sd[f"encoder.{i}.bias"]), padding=1)
    if relu:
        y = torch.relu(y)
    if pool:
        y = F.max_pool2d(y, 2, 2)
    return y.numpy()


def gpu_layer(enc, layer, x):
    import torch
    from gloc3d_amd import i2i
    n, _, H, W = x.shape
    _, co, _, pool = i2i._shape(layer)
    d_in = torch.from_numpy(x).cuda()
    out = torch.empty((n, co, H // 2 if pool else H, W // 2 if pool else W), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    enc.forward_layer_device(layer, d_in.data_ptr(), n, H, W, out.data_ptr())
    enc.synchronize()
    return out.cpu().numpy()


def rel_err(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


# layer 0 (Cin = 3), a pooled 64-channel layer, a pooled 128-channel layer, a 256 -> 512 layer, a 512-channel layer and
# conv5_3 (no ReLU); H x W not a multiple of the 16 x 8 tile, n = 1 and 3
@pytest.mark.parametrize("layer,n,H,W", [(0, 1, 37, 29), (0, 3, 20, 50), (1, 3, 18, 34), (3, 1, 22, 14), (7, 1, 9, 13),
                                         (8, 3, 11, 21), (9, 1, 10, 6), (12, 3, 7, 19), (12, 1, 1, 1)])
def test_single_layer_random_fp32(enc, sd, layer, n, H, W):
    from gloc3d_amd import i2i
    ci, _, _, _ = i2i._shape(layer)
    rng = np.random.default_rng(1000 + layer * 7 + n)
    x = rng.standard_normal((n, ci, H, W)).astype(np.float32)
    if layer > 0:
        x = np.maximum(x, 0) * 2.0  # a post-ReLU input, as inside the network (signed inputs are the layer-0 case)
    g, r = gpu_layer(enc, layer, x), torch_layer(sd, layer, x)
    assert g.shape == r.shape
    assert rel_err(g, r) <= FEAT_TOL, rel_err(g, r)
    if layer == 12:
        assert (g < 0).any()   # conv5_3 keeps its sign


def test_single_layer_signed_inputs(enc, sd):
    """Arbitrary fp32 input for a deep layer: signed values over several orders of magnitude."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((2, 256, 12, 10)) * np.exp(rng.uniform(-3, 3, (2, 256, 12, 10)))).astype(np.float32)
    g, r = gpu_layer(enc, 6, x), torch_layer(sd, 6, x)
    assert rel_err(g, r) <= FEAT_TOL, rel_err(g, r)


def test_encoder_and_descriptor_small_golden(enc, sd):
    from gloc3d_amd import i2i
    g = np.load(os.path.join(GOLDEN, "i2i_small.npz"))
    assert int(g["seed"]) == R.SEED
    x = g["x"].astype(np.float32)
    f = enc.forward(x)
    assert f.shape == g["feat"].shape
    assert rel_err(f, g["feat"]) <= FEAT_TOL, rel_err(f, g["feat"])
    d = i2i.I2iVladDescriptor.from_state_dict(sd, width=x.shape[3], height=x.shape[2])
    try:
        import torch
        feat, desc = d.describe_images(torch.from_numpy(x).cuda())
        assert (feat.cpu().numpy().view(np.uint32) == f.view(np.uint32)).all()
        assert rel_err(desc.cpu().numpy(), g["desc"]) <= DESC_TOL
    finally:
        d.close()


def test_encoder_and_descriptor_full_size_golden(enc, sd):
    import torch
    from gloc3d_amd import i2i
    g = np.load(os.path.join(GOLDEN, "i2i_full.npz"))
    shape = tuple(int(v) for v in g["shape"])
    x = np.unpackbits(g["bits"])[:int(np.prod(shape))].reshape(shape).astype(np.float32)
    d = i2i.I2iVladDescriptor.from_state_dict(sd)
    try:
        feat, desc = d.describe_images(torch.from_numpy(x).cuda())
        f = feat.cpu().numpy()
        assert f.shape == (1, 512, 48, 48)
        err = float(np.abs(f.reshape(-1)[g["idx"]] - g["feat_sample"]).max() / g["feat_absmax"])
        assert err <= FEAT_TOL, err
        assert abs(float(np.abs(f).max()) - float(g["feat_absmax"])) <= FEAT_TOL * float(g["feat_absmax"])
        assert rel_err(desc.cpu().numpy(), g["desc"]) <= DESC_TOL
    finally:
        d.close()


def test_batch_equals_single_calls(enc):
    rng = np.random.default_rng(11)
    x = R.binary_image(rng, 5, 64, 48)
    x[:, :, 10:30, 5:20] = rng.standard_normal((5, 3, 20, 15)).astype(np.float32)  # not only binary values
    batch = enc.forward(x)
    for i in range(5):
        one = enc.forward(x[i:i + 1])
        assert (one.view(np.uint32) == batch[i:i + 1].view(np.uint32)).all(), i


def test_more_images_than_one_pass(enc):
    """Batches beyond the internal pass of 8 images: still the single calls' bits."""
    rng = np.random.default_rng(12)
    x = rng.standard_normal((11, 3, 32, 16)).astype(np.float32)
    batch = enc.forward(x)
    for i in (0, 7, 8, 10):
        assert (enc.forward(x[i:i + 1]).view(np.uint32) == batch[i:i + 1].view(np.uint32)).all(), i


def test_refusals(capi, enc, sd):
    import torch
    L = capi.lib()
    x = np.zeros((1, 3, 40, 32), np.float32)
    with pytest.raises(capi.GlocError) as e:
        enc.forward(x)                      # 40 is no multiple of 16
    assert e.value.code == 1
    with pytest.raises(capi.GlocError) as e:
        enc.forward(np.zeros((1, 3, 32, 24), np.float32))
    assert e.value.code == 1
    d = torch.zeros(40000, device="cuda")   # 160 KB: every call below stays inside it
    assert L.gloc_vgg_forward_layer(enc._h, 1, capi.C.c_void_p(d.data_ptr()), 1, 9, 10,
                                    capi.C.c_void_p(d.data_ptr())) == 1   # odd H for a pooled layer
    assert L.gloc_vgg_forward_layer(enc._h, 13, capi.C.c_void_p(d.data_ptr()), 1, 8, 8,
                                    capi.C.c_void_p(d.data_ptr())) == 1
    fresh = capi.VggEncoder()
    try:
        from gloc3d_amd import i2i
        w = i2i.i2i_weights(sd)["encoder"]
        for li in range(12):                # conv5_3 never set
            fresh.set_layer(li, *w[li])
        with pytest.raises(capi.GlocError) as e:
            fresh.forward(np.zeros((1, 3, 32, 32), np.float32))
        assert e.value.code == 5            # GLOC_ERR_STATE
        assert L.gloc_vgg_forward_layer(fresh._h, 12, capi.C.c_void_p(d.data_ptr()), 1, 4, 4,
                                        capi.C.c_void_p(d.data_ptr())) == 5
        fresh.forward_layer_device(11, d.data_ptr(), 1, 4, 4, d.data_ptr() + 4 * 512 * 16)  # a set layer runs
        fresh.synchronize()
    finally:
        fresh.close()


def _scans(n, seed=3, n_az=600):
    from gloc3d_amd import synth
    w = synth.make_world(seed)
    return [np.ascontiguousarray(synth.lidar_scan(w, synth.se3(0.2 * i, (4.0 * i, 1.5 * np.sin(i), 0.0)), seed + i,
                                                  n_az=n_az)) for i in range(n)]


def test_descriptor_on_synthetic_scans(sd):
    """I2iVladDescriptor (HIP BEV -> HIP VGG -> HIP NetVLAD-FC) against the torch restatement fed with the same HIP BEV
    images; one call for the batch equals one call per scan."""
    import torch
    from gloc3d_amd import i2i
    scans = _scans(3)
    d = i2i.I2iVladDescriptor.from_state_dict(sd, width=256, height=192)
    try:
        imgs = d.images(scans)
        x = imgs.cpu().numpy()
        assert set(np.unique(x)) <= {0.0, 1.0} and (x[:, 0] == 0).any()
        out = d(scans)
        assert out.shape == (3, 512)
        with torch.no_grad():
            ref = R.netvlad(R.encoder(sd)(torch.from_numpy(x)), sd).numpy()
        assert rel_err(out, ref) <= DESC_TOL, rel_err(out, ref)
        for i in range(3):
            assert (d(scans[i]).view(np.uint32) == out[i:i + 1].view(np.uint32)).all()
        desc, grid, xy_res = d.place_feature(scans[0])
        assert (desc.view(np.uint32) == out[0].view(np.uint32)).all()
        assert grid.dtype == np.uint8 and grid.ndim == 2 and len(xy_res) == 3
    finally:
        d.close()


def test_loop_detector_place_feature(sd):
    from gloc3d_amd import i2i, loop_detector
    scans = _scans(1)
    model = i2i.I2iVladDescriptor.from_state_dict(sd)
    det = loop_detector.RpyPCLoopDetector(512)
    try:
        with pytest.raises(RuntimeError):
            det.get_place_feature(scans[0])      # no descriptor model attached
        det.set_descriptor_model(model)
        desc, grid, xy_res = det.get_place_feature(scans[0])
        g2, xy2 = det.get_projected_grid(scans[0])
        assert (grid == g2).all() and np.allclose(xy_res, xy2)
        assert (desc.view(np.uint32) == model(scans[0])[0].view(np.uint32)).all()
    finally:
        det.close()
        model.close()


@pytest.fixture(scope="module")
def drive(tmp_path_factory, sd):
    """A synthetic valset of 52 places (more than the reference's 30 + 20 guard) and 3 queries, the GLOCI2IW file of
    the seeded weights, and the command line."""
    from gloc3d_amd import build, gloc_io, i2i, synth
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_i2i_weights as X
    d = tmp_path_factory.mktemp("i2i_drive")
    n_db, q_at = 52, [9, 26, 44]
    w = synth.make_world(2024)
    files, poses = [], []
    for i in range(n_db):
        T = synth.se3(0.5 * (i - 26), (0.7 * i - 18.0, 0.1 * i, 0.0))
        f = str(d / f"db_{i:06d}.bin")
        synth.write_kitti_bin(f, synth.lidar_scan(w, T, seed=300 + i, n_az=360))
        files.append(f)
        poses.append(T)
    qfiles = []
    for qi, j in enumerate(q_at):
        T = synth.se3(0.5 * (j - 26) + 1.0, (0.7 * j - 18.0 + 0.25, 0.1 * j - 0.2, 0.02))
        f = str(d / f"q_{qi:06d}.bin")
        synth.write_kitti_bin(f, synth.lidar_scan(w, T, seed=700 + qi, n_az=360))
        qfiles.append(f)
        poses.append(T)
    gloc_io.write_valset(d / "valset.txt", files, qfiles, [[j - 1, j, j + 1] for j in q_at])
    gloc_io.write_poses(d / "poses.txt", poses)
    X.write(str(d / "i2i.bin"), i2i.i2i_weights(sd))
    return dict(dir=d, scans=[synth.read_kitti_bin(f) for f in files + qfiles], exe=build.build_cli()[0])


def _describe(sd, scans):
    from gloc3d_amd import i2i
    model = i2i.I2iVladDescriptor.from_state_dict(sd)
    try:
        return np.concatenate([model(scans[i:i + 8]) for i in range(0, len(scans), 8)])
    finally:
        model.close()


def _run_cli(drive, model_file, extra, tag):
    """The report lines and failure files of one run, and the descriptors it retrieved with (GLOC_DUMP_DESCRIPTORS)."""
    from gloc3d_amd import gloc_io
    d = drive["dir"]
    run_dir = d / tag
    run_dir.mkdir()
    env = dict(os.environ, GLOC_DUMP_DESCRIPTORS=str(run_dir / "used.bin"))
    p = subprocess.run([drive["exe"], str(d / "valset.txt"), str(d / "poses.txt"), str(model_file)] + extra,
                       cwd=run_dir, capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    keys = ("Recall @", "Success rate", "Rot error", "Pos error")
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith(keys) or re.fullmatch(r"\d+, \d+", ln)]
    assert len(lines) == 8, p.stdout
    report = (lines, (run_dir / "failed_detect_indices.txt").read_text(),
              (run_dir / "failed_registration_indices.txt").read_text())
    return report, gloc_io.read_descriptors(run_dir / "used.bin"), p.stdout


def test_command_line_model_mode_matches_descriptor_file(drive, sd):
    """global_localization VALSET POSES MODEL with a GLOCI2IW file (the command line describes the db scans in batches
    and each query on its own, through gloc_host::I2iModel) retrieves with the same bits as I2iVladDescriptor, and
    prints the same report as a run given those descriptors in a GLOCDESC file."""
    from gloc3d_amd import gloc_io
    desc = _describe(sd, drive["scans"])
    gloc_io.write_descriptors(drive["dir"] / "desc.bin", desc)
    rep_file, used_file, _ = _run_cli(drive, drive["dir"] / "desc.bin", [], "plain_desc")
    rep_model, used_model, out = _run_cli(drive, drive["dir"] / "i2i.bin", [], "plain_model")
    assert "time cost for the db descriptors" in out
    assert (used_file.view(np.uint32) == desc.view(np.uint32)).all()
    assert used_model.shape == desc.shape and (used_model.view(np.uint32) == desc.view(np.uint32)).all()
    assert rep_model == rep_file


def test_command_line_model_mode_describes_ground_aligned_scans(drive, sd):
    """With the 4th argument the reference describes the ground-aligned clouds (global_localization.cpp:431-440 and
    :495-499 give them to add_keyframe / detect): MODEL mode's descriptors equal I2iVladDescriptor's of the scans
    aligned by gloc_ground, bit for bit, and the report equals a GLOCDESC run of those descriptors with alignment."""
    from gloc3d_amd import capi, gloc_io
    ground = capi.GroundEstimator()
    try:
        aligned = [ground.estimate(s, want_cloud=True)[2] for s in drive["scans"]]
    finally:
        ground.close()
    desc = _describe(sd, aligned)
    raw = _describe(sd, drive["scans"])
    assert not (desc.view(np.uint32) == raw.view(np.uint32)).all()   # alignment moves the BEV images
    gloc_io.write_descriptors(drive["dir"] / "desc_aligned.bin", desc)
    rep_file, _, out_file = _run_cli(drive, drive["dir"] / "desc_aligned.bin", ["x"], "aligned_desc")
    rep_model, used_model, out = _run_cli(drive, drive["dir"] / "i2i.bin", ["x"], "aligned_model")
    assert "time cost for align to ground" in out and "time cost for align to ground" in out_file
    assert used_model.shape == desc.shape and (used_model.view(np.uint32) == desc.view(np.uint32)).all()
    assert rep_model == rep_file
