"""numpy restatement of the PointPillar scan front end (gloc_pillar_*): points_to_voxels + the traced model's 16-channel
input (model/voxel.py:23-133, s2s_libtorch/gen_libtorch_pointpillar.py:47-62) and the PointNet + scatter-mean canvas of
PointPillarTest.forward (model/s2s_merged.py:113-127,204-222).  The 16 channels are pinned bit for bit to the reference
module (tests/golden/pillar_*.npz, made by make_pillar_goldens.py); the canvas to a tolerance.  Quirks Q1-Q9 are those of
the issue that introduced the feature; DESIGN.md section 8 restates them.

Also the seeded weights recipe the descriptor goldens were made with: every parameter is a function of its name and
shape only, so the tests regenerate the state_dict instead of storing it.
"""
import zlib

import numpy as np

F32 = np.float32
INT_MIN = np.int32(-2**31)
MASK_INPUT, MASK_VALID = 0, 1          # include/gloc3d.h GLOC_PILLAR_MASK_*
REF_BOUNDS = ([-35.0, 35.0, 0.5], [-20.0, 20.0, 0.5], [-10.0, 10.0, 20.0])   # gen_libtorch_pointpillar.py:27-29
REF_P = 122480                                                                 # dataset/kitti_s2s.py:222-227


class Grid:
    """[lo, hi, res] per axis as the reference builds them: the sizes from the float64 bounds, truncated
    (voxel.py:40-45); offset and voxel size as float32 tensors (:46-49)."""

    def __init__(self, xb=REF_BOUNDS[0], yb=REF_BOUNDS[1], zb=REF_BOUNDS[2]):
        self.bounds = (tuple(xb), tuple(yb), tuple(zb))
        self.size = np.array([int((b[1] - b[0]) / b[2]) for b in self.bounds], np.int64)
        self.offset = np.array([b[0] for b in self.bounds], F32)
        self.res = np.array([b[2] for b in self.bounds], F32)
        self.nv = int(self.size.prod())


def pad_scan(scan, P):
    """Scan [n, >=4] -> points [P, 4] float32 and mask [P] float32: the first P points, zero rows with mask 0 after them
    (pad_or_trim_to_np, voxel.py:6-11; kitti_s2s.py:222-227)."""
    s = np.asarray(scan, F32).reshape(-1, np.shape(scan)[-1] if np.ndim(scan) == 2 else 4)[:, :4]
    n = min(s.shape[0], P)
    pts = np.zeros((P, 4), F32)
    pts[:n] = s[:n]
    mask = np.zeros(P, F32)
    mask[:n] = 1
    return pts, mask


def trunc_i32(v):
    """float32 -> int32 as x86 cvttss2si: toward zero; NaN and |v| >= 2^31 give INT_MIN (Q1, Q9)."""
    v = np.asarray(v, F32)
    ok = (v >= F32(-2.0**31)) & (v < F32(2.0**31))          # False for NaN
    out = np.full(v.shape, INT_MIN, np.int32)
    out[ok] = np.trunc(v[ok]).astype(np.int32)
    return out


def voxelize(pts, mask, g):
    """points [P, 4], mask [P] -> dict of the per-row quantities of points_to_voxels."""
    xyz = np.ascontiguousarray(pts[:, :3], F32)
    shifted = xyz - g.offset                                   # fp32 subtraction
    vxyz = shifted / g.res                                     # Q1: fp32 division, not a multiply by 1/res
    coords = trunc_i32(vxyz)
    pad = (mask < 1) | np.any((coords >= g.size) | (coords < 0), axis=1)     # Q2
    gy, gz = int(g.size[1]), int(g.size[2])
    c64 = coords.astype(np.int64)
    index = np.where(pad, 0, c64[:, 0] * (gy * gz) + c64[:, 1] * gz + c64[:, 2])   # Q3: x-major
    centre = (F32(0.5) + coords.astype(F32)) * g.res + g.offset                   # Q4: coords before padding
    count = np.zeros(g.nv, F32)
    np.add.at(count, index, (~pad).astype(F32))                                    # Q5: unpadded rows only
    sums = np.zeros((g.nv, 3), F32)
    np.add.at(sums, index, xyz)                               # Q6: every row, in row order, fp32 (ufunc.at is unbuffered)
    n_all = np.bincount(index, minlength=g.nv).astype(F32)
    centroid = sums / np.maximum(n_all, F32(1))[:, None]
    return dict(xyz=xyz, coords=coords, pad=pad, index=index, centre=centre, count=count, centroid=centroid,
                n_all=n_all)


def inputs16(pts, mask, g):
    """[P, 16] float32: x y z i, count, p - centroid, centroid, p - centre, index, mask (Q7)."""
    v = voxelize(pts, mask, g)
    idx = v["index"]
    pc = v["centroid"][idx]
    out = np.empty((pts.shape[0], 16), F32)
    out[:, 0:4] = pts
    out[:, 4] = v["count"][idx]
    out[:, 5:8] = v["xyz"] - pc
    out[:, 8:11] = pc
    out[:, 11:14] = v["xyz"] - v["centre"]
    out[:, 14] = idx.astype(F32)
    out[:, 15] = mask
    return out, v


def inputs16_loop(pts, mask, g):
    """The same, one row at a time with Python floats rounded to float32 after every operation: a literal transcription
    of voxel.py's arithmetic (and of the C++ demo's loop, i2i_feature_extract.cpp:86-137, with Python's index)."""
    P = pts.shape[0]
    f = lambda x: float(F32(x))
    off = [float(o) for o in g.offset]
    res = [float(r) for r in g.res]
    gx, gy, gz = (int(s) for s in g.size)

    def trunc(x):
        if x != x or not (-2.0**31 <= x < 2.0**31):
            return -2**31
        return int(x)  # toward zero

    rows = []
    cnt = [0.0] * g.nv
    sums = [[0.0, 0.0, 0.0] for _ in range(g.nv)]
    nall = [0] * g.nv
    for p in range(P):
        xyz = [float(pts[p, k]) for k in range(3)]
        c = [trunc(f(f(xyz[k] - off[k]) / res[k])) for k in range(3)]
        pad = mask[p] < 1 or c[0] >= gx or c[1] >= gy or c[2] >= gz or min(c) < 0
        idx = 0 if pad else c[0] * gy * gz + c[1] * gz + c[2]
        centre = [f(f(f(0.5 + f(c[k])) * res[k]) + off[k]) for k in range(3)]
        if not pad:
            cnt[idx] = f(cnt[idx] + 1.0)
        sums[idx] = [f(sums[idx][k] + xyz[k]) for k in range(3)]
        nall[idx] += 1
        rows.append((xyz, centre, idx))
    out = np.empty((P, 16), F32)
    for p, (xyz, centre, idx) in enumerate(rows):
        cen = [f(sums[idx][k] / float(max(nall[idx], 1))) for k in range(3)]
        out[p, 0:4] = pts[p]
        out[p, 4] = cnt[idx]
        out[p, 5:8] = [f(xyz[k] - cen[k]) for k in range(3)]
        out[p, 8:11] = cen
        out[p, 11:14] = [f(xyz[k] - centre[k]) for k in range(3)]
        out[p, 14] = float(idx)
        out[p, 15] = mask[p]
    return out


def pointnet(inp, pad, w, bn_w, bn_b, bn_mean, bn_var, eps=1e-5, mask_mode=MASK_INPUT):
    """PointNet (Conv1d 14 -> 64 without bias, BatchNorm1d in eval mode, ReLU) times the row mask (Q8), float64.
    mask_mode MASK_INPUT: input channel 15 (the traced model, s2s_merged.py:204-206); MASK_VALID: 1 - padding
    (the training forward, pointpillar.py:199).  -> [P, 64]."""
    x = inp[:, :14].astype(np.float64)
    y = x @ np.asarray(w, np.float64).T
    y = (y - np.asarray(bn_mean, np.float64)) / np.sqrt(np.asarray(bn_var, np.float64) + eps) \
        * np.asarray(bn_w, np.float64) + np.asarray(bn_b, np.float64)
    y = np.where(y < 0, 0.0, y)               # ReLU (NaN stays NaN, as torch.relu)
    m = inp[:, 15].astype(np.float64) if mask_mode == MASK_INPUT else (~np.asarray(pad)).astype(np.float64)
    return y * m[:, None]


def canvas(inp, pad, g, pn_params, mask_mode=MASK_INPUT, accumulate="fp64"):
    """scatter_mean of the PointNet features over input channel 14 into [64, nv]; the divisor counts every row of the
    voxel (padding included), empty voxels are 0.  accumulate="fp64": exact-ish sums (what the device approximates);
    "fp32": float32 features summed in row order in float32, as the reference's torch_scatter on the CPU."""
    feat = pointnet(inp, pad, *pn_params, mask_mode=mask_mode)
    idx = inp[:, 14].astype(np.int64)
    dt = np.float64 if accumulate == "fp64" else F32
    sums = np.zeros((g.nv, feat.shape[1]), dt)
    np.add.at(sums, idx, feat.astype(dt))
    n = np.bincount(idx, minlength=g.nv).astype(dt)
    return (sums / np.maximum(n, 1)[:, None]).T.astype(F32)


def rel_err(a, ref):
    """max |a - ref| / max |ref| over the finite entries (NaN must sit in the same places)."""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert (np.isnan(a) == np.isnan(ref)).all(), "NaN in different places"
    ok = ~np.isnan(ref)
    scale = np.abs(ref[ok]).max() if ok.any() else 0.0
    d = np.abs(a[ok] - ref[ok]).max() if ok.any() else 0.0
    return d / scale if scale > 0 else d


# ---- the seeded weights recipe ------------------------------------------------------------------------------------

def seeded_param(name, shape):
    """A parameter / buffer of a PointPillarVLAD state_dict from its name and shape alone (crc32 of the name seeds it)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    shape = tuple(int(s) for s in shape)
    leaf = name.rsplit(".", 1)[-1]
    if leaf == "num_batches_tracked":
        return np.zeros(shape, np.int64)
    r = rng.standard_normal(shape)
    if leaf == "running_var":
        v = 0.5 + 0.5 * np.abs(r)
    elif leaf == "running_mean":
        v = 0.1 * r
    elif leaf == "bias":
        v = 0.1 * r
    elif name.endswith("centroids"):
        v = rng.random(shape)                        # torch.rand in the module's constructor (netvlad_fc.py:36)
    elif name.endswith("hidden1_weights"):
        v = r / np.sqrt(shape[1])                    # netvlad_fc.py:38-39
    elif len(shape) == 1:                            # a BatchNorm weight
        v = 1.0 + 0.1 * r
    else:                                            # a convolution: 1 / sqrt(fan_in)
        v = r / np.sqrt(np.prod(shape[1:]))
    return v.astype(F32)


def seeded_state_dict(shapes):
    """{name: shape} -> {name: numpy array}."""
    return {k: seeded_param(k, s) for k, s in shapes.items()}


def pn_params_from_state(sd, prefix="encoder.pn.pointnet."):
    """(w [64, 14], bn weight, bias, running mean, running var) of the PointNet in a state_dict."""
    g = lambda k: np.asarray(sd[prefix + k], F32)
    return (g("0.weight").reshape(64, 14), g("1.weight"), g("1.bias"), g("1.running_mean"), g("1.running_var"))
