"""CPU: the numpy restatement tests/pillar_ref.py against the reference module's goldens (tests/golden/pillar_*.npz), a
literal per-row loop, and the layout quirk Q3."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pillar_ref as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
DENSE = ["small_pad", "small_trim", "flat_pad", "flat_empty"]


def load(name):
    g = np.load(os.path.join(GOLDEN, f"pillar_{name}.npz"))
    b = g["bounds"]
    return g, R.Grid(b[0], b[1], b[2]), int(g["P"])


def golden_canvas(g, grid, mm):
    if f"canvas{mm}" in g.files:
        return g[f"canvas{mm}"]
    c = np.zeros((64, grid.nv), np.float32)
    c[:, g[f"canvas{mm}_voxels"]] = g[f"canvas{mm}_values"]
    return c


def pn_params():
    shapes = {"encoder.pn.pointnet.0.weight": (64, 14, 1), "encoder.pn.pointnet.1.weight": (64,),
              "encoder.pn.pointnet.1.bias": (64,), "encoder.pn.pointnet.1.running_mean": (64,),
              "encoder.pn.pointnet.1.running_var": (64,)}
    return R.pn_params_from_state(R.seeded_state_dict(shapes))


@pytest.mark.parametrize("name", DENSE + ["refgrid_p2048"])
def test_inputs_bit_equal_to_reference(name):
    g, grid, P = load(name)
    pts, mask = R.pad_scan(g["scan"], P)
    inp, v = R.inputs16(pts, mask, grid)
    assert inp.shape == g["inputs"].shape
    diff = np.flatnonzero((inp.view(np.uint32) != g["inputs"].view(np.uint32)).any(0))
    assert diff.size == 0, f"channels {diff.tolist()} differ"
    assert (v["pad"] == g["padding"].astype(bool)).all()


@pytest.mark.parametrize("name", DENSE + ["refgrid_p2048"])
@pytest.mark.parametrize("mm", [R.MASK_INPUT, R.MASK_VALID])
def test_canvas_close_to_reference(name, mm):
    g, grid, P = load(name)
    pts, mask = R.pad_scan(g["scan"], P)
    inp, v = R.inputs16(pts, mask, grid)
    ref = golden_canvas(g, grid, mm)
    for acc in ("fp32", "fp64"):
        c = R.canvas(inp, v["pad"], grid, pn_params(), mm, accumulate=acc)
        assert R.rel_err(c, ref) <= 1e-6, acc


def test_goldens_cover_the_edges():
    g, grid, P = load("small_pad")
    inp = g["inputs"]
    n = g["scan"].shape[0]
    assert (inp[n:, 15] == 0).all() and (inp[:n, 15] == 1).all()             # padding rows
    assert np.isnan(inp[:, 0]).any()                                          # a NaN row (Q9)
    assert np.isnan(inp[inp[:, 14] == 0, 8]).all()                            # ... poisons voxel 0's centroid
    assert (g["padding"][:n] == 1).sum() > 10                                 # out-of-range rows
    t, _, Pt = load("small_trim")
    assert t["scan"].shape[0] > Pt and (t["inputs"][:, 15] == 1).all()       # n > P


@pytest.mark.parametrize("name", ["small_pad", "small_trim", "flat_pad", "flat_empty"])
def test_restatement_equals_row_loop(name):
    g, grid, P = load(name)
    pts, mask = R.pad_scan(g["scan"], P)
    a = R.inputs16(pts, mask, grid)[0]
    b = R.inputs16_loop(pts, mask, grid)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_row_loop_on_reference_grid():
    g, grid, P = load("refgrid_p2048")
    pts, mask = R.pad_scan(g["scan"], 512)
    a = R.inputs16(pts, mask, grid)[0]
    b = R.inputs16_loop(pts, mask, grid)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_index_is_x_major():
    """Q3: +0.5 m in x moves the index by gy * gz = 80 on the reference grid; +0.5 m in y by 1."""
    grid = R.Grid()
    p = np.array([[1.1, 2.2, 0.3, 0], [1.6, 2.2, 0.3, 0], [1.1, 2.7, 0.3, 0]], np.float32)
    inp = R.inputs16(p, np.ones(3, np.float32), grid)[0]
    i0, ix, iy = inp[:, 14].astype(int)
    assert ix - i0 == 80 and iy - i0 == 1
    small = R.Grid(*([-2.0, 2.0, 0.5], [-1.0, 1.0, 0.25], [-1.0, 1.0, 1.0]))
    p = np.array([[0.1, 0.1, 0.1, 0], [0.6, 0.1, 0.1, 0], [0.1, 0.1, -0.9, 0]], np.float32)
    inp = R.inputs16(p, np.ones(3, np.float32), small)[0]
    i0, ix, iz = inp[:, 14].astype(int)
    assert ix - i0 == 8 * 2 and i0 - iz == 1


def test_truncation_band_lands_in_cell_zero():
    """Q1: a point up to one cell below the lower bound truncates to coordinate 0 and is not padding."""
    grid = R.Grid()
    p = np.array([[-35.3, 0.1, 0.0, 0], [-35.6, 0.1, 0.0, 0]], np.float32)
    inp, v = R.inputs16(p, np.ones(2, np.float32), grid)
    assert not v["pad"][0] and v["pad"][1]
    assert inp[0, 14] == 40 and inp[1, 14] == 0


def test_seeded_weights_are_stable():
    a = R.seeded_param("encoder.block1.layers.0.weight", (64, 64, 3, 3))
    b = R.seeded_param("encoder.block1.layers.0.weight", (64, 64, 3, 3))
    assert (a == b).all() and a.dtype == np.float32
    assert (R.seeded_param("encoder.pn.pointnet.1.running_var", (64,)) > 0).all()
