"""GPU: the PointPillar front end (gloc_pillar_*) against the reference module's goldens and the numpy restatement
tests/pillar_ref.py: the 16 channels bit for bit, the canvas to 2e-6 relative, batches equal to single calls, the
descriptor of PillarVladDescriptor to 1e-3 absolute."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pillar_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden")
_spec = importlib.util.spec_from_file_location("make_pillar_goldens", os.path.join(GOLDEN, "make_pillar_goldens.py"))
MK = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MK)
CASES = ["small_pad", "small_trim", "flat_pad", "flat_empty", "refgrid_p2048"]


def load(name):
    g = np.load(os.path.join(GOLDEN, f"pillar_{name}.npz"))
    b = g["bounds"]
    return g, R.Grid(b[0], b[1], b[2]), int(g["P"])


def params(capi, grid, P, mm=0):
    b = grid.bounds
    return capi.default_pillar_params(xbound=b[0], ybound=b[1], zbound=b[2], num_points=P, mask_mode=mm)


def pn_shapes():
    return {"encoder.pn.pointnet.0.weight": (64, 14, 1), "encoder.pn.pointnet.1.weight": (64,),
            "encoder.pn.pointnet.1.bias": (64,), "encoder.pn.pointnet.1.running_mean": (64,),
            "encoder.pn.pointnet.1.running_var": (64,)}


@pytest.fixture(scope="module")
def enc(capi):
    e = capi.PillarEncoder()
    e.set_pointnet(*R.pn_params_from_state(R.seeded_state_dict(pn_shapes())))
    yield e
    e.close()


@pytest.fixture(scope="module")
def lidar():
    """64 x 2000 rays to 80 m: more than P returns, many of them outside the 70 x 40 m grid."""
    from gloc3d_amd import synth
    w = synth.make_world(7)
    return synth.lidar_scan(w, synth.se3(0.3, (5, 2, 0)), 7)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", CASES)
def test_inputs_bit_equal_to_goldens(capi, enc, name):
    g, grid, P = load(name)
    out = enc.inputs(g["scan"], params(capi, grid, P))[0]
    pts, mask = R.pad_scan(g["scan"], P)
    ref = R.inputs16(pts, mask, grid)[0]
    for want in (g["inputs"], ref):
        diff = np.flatnonzero((bits(out) != bits(want)).any(0))
        assert diff.size == 0, f"channels {diff.tolist()} differ"


def test_inputs_bit_equal_full_size(capi, enc, lidar):
    grid = R.Grid()
    assert lidar.shape[0] > R.REF_P
    for scan in (lidar, lidar[:90000]):
        out = enc.inputs(scan, capi.default_pillar_params())[0]
        pts, mask = R.pad_scan(scan, R.REF_P)
        ref, v = R.inputs16(pts, mask, grid)
        if scan is lidar:                                     # a large voxel 0: the long in-order chain
            assert ((mask > 0) & v["pad"]).sum() > 10000
        diff = np.flatnonzero((bits(out) != bits(ref)).any(0))
        assert diff.size == 0, f"channels {diff.tolist()} differ"


@pytest.mark.parametrize("mm", [R.MASK_INPUT, R.MASK_VALID])
@pytest.mark.parametrize("name", CASES)
def test_canvas_close_to_restatement(capi, enc, name, mm):
    g, grid, P = load(name)
    out = enc.canvas(g["scan"], params(capi, grid, P, mm))[0]
    pts, mask = R.pad_scan(g["scan"], P)
    inp, v = R.inputs16(pts, mask, grid)
    pn = R.pn_params_from_state(R.seeded_state_dict(pn_shapes()))
    assert R.rel_err(out, R.canvas(inp, v["pad"], grid, pn, mm)) <= 2e-6
    empty = np.bincount(inp[:, 14].astype(np.int64), minlength=grid.nv) == 0
    assert (out[:, empty] == 0).all()


@pytest.mark.parametrize("mm", [R.MASK_INPUT, R.MASK_VALID])
def test_canvas_full_size(capi, enc, lidar, mm):
    grid = R.Grid()
    out = enc.canvas(lidar, capi.default_pillar_params(mask_mode=mm))[0]
    pts, mask = R.pad_scan(lidar, R.REF_P)
    inp, v = R.inputs16(pts, mask, grid)
    pn = R.pn_params_from_state(R.seeded_state_dict(pn_shapes()))
    assert R.rel_err(out, R.canvas(inp, v["pad"], grid, pn, mm)) <= 2e-6


def test_batch_equals_single_calls(capi, enc, lidar):
    P = 30000
    scans = [lidar[:0], lidar[:1000], lidar[5000:29000], lidar[:P + 5000], lidar[40000:41000], lidar[:P],
             lidar[60000:], lidar[::7]]
    p = capi.default_pillar_params(num_points=P)
    bi, bc = enc.inputs(scans, p), enc.canvas(scans, p)
    for k, s in enumerate(scans):
        assert (bits(enc.inputs(s, p)[0]) == bits(bi[k])).all(), k
        assert (bits(enc.canvas(s, p)[0]) == bits(bc[k])).all(), k
    assert (bits(enc.inputs(scans, p)) == bits(bi)).all()
    assert (bits(enc.canvas(scans, p)) == bits(bc)).all()


def test_device_path_on_torch_stream(capi, enc, lidar):
    import torch
    p = capi.default_pillar_params()
    scans = [lidar[:100000], lidar[1000:]]
    host_i, host_c = enc.inputs(scans, p), enc.canvas(scans, p)
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(scans))).cuda()
    off = np.array([0, 100000, 100000 + scans[1].shape[0]], np.uint64)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        oi = torch.empty((2, p.num_points, 16), device="cuda")
        oc = torch.empty((2, 64, 140 * 80), device="cuda")
        enc.set_stream(s.cuda_stream)
        enc.inputs_device(pts.data_ptr(), off, 4, oi.data_ptr(), p)
        enc.canvas_device(pts.data_ptr(), off, 4, oc.data_ptr(), p)
    s.synchronize()
    enc.set_stream(0)
    assert (bits(oi.cpu().numpy()) == bits(host_i)).all()
    assert (bits(oc.cpu().numpy()) == bits(host_c)).all()


def test_canvas_needs_pointnet(capi):
    e = capi.PillarEncoder()
    with pytest.raises(capi.GlocError) as err:
        e.canvas(np.zeros((3, 4), np.float32))
    assert err.value.code == 5
    e.close()


def test_descriptor_matches_reference(capi):
    import torch
    from gloc3d_amd.pillar import PillarBackbone, PillarVladDescriptor
    g = np.load(os.path.join(GOLDEN, "pillar_descriptor.npz"))
    shapes = {"encoder." + k: tuple(t.shape) for k, t in PillarBackbone(140, 80).state_dict().items()}
    shapes.update(pn_shapes())
    shapes.update({"pool.conv.weight": (64, 128, 1, 1), "pool.centroids": (64, 128), "pool.hidden1_weights": (8192, 128),
                   "encoder.conv_out_pose.0.weight": (256, 448, 3, 3), "encoder.conv_out_pose.1.running_var": (256,)})
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in R.seeded_state_dict(shapes).items()}
    d = PillarVladDescriptor.from_state_dict({"state_dict": sd},
                                             params=capi.default_pillar_params(num_points=int(g["P"])))
    scans = MK.descriptor_scans()
    assert [len(s) for s in scans] == [int(g["n0"]), int(g["n1"])]
    out = d(scans)
    assert out.shape == g["desc"].shape
    assert np.abs(out - g["desc"]).max() <= 1e-3
    one = d(scans[1])                                  # a batch of one gives the same descriptor
    assert np.abs(one[0] - out[1]).max() <= 1e-5
    d.close()
